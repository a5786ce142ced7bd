"""The adaptive-render part of the C ABI (include/rt_abi.h rt_adaptive,
rt_render_camera_adaptive_async, rt_render_camera_adaptive_plan): declared,
exported, laid out as the ctypes mirror says, and reached by the CLI flags. No
device calls (CPU-only)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import go_raytracer_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_abi.h")
FUNCS = ["rt_render_camera_adaptive_async", "rt_render_camera_adaptive_plan"]
FIELDS = ["min_samples", "reserved", "tolerance"]


def test_header_declares_the_functions_and_the_record():
    src = open(HEADER).read()
    names = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(rt_\w+)\s*\(", src, re.M))
    for n in FUNCS:
        assert n in names
    assert re.search(r"typedef struct rt_adaptive\s*\{", src)
    assert "#define RT_ABI_VERSION 6" in src  # additive: the version stays


def test_library_exports_the_functions():
    lib = rt.load_library()
    for n in FUNCS:
        assert hasattr(lib, n), n


def test_adaptive_layout_matches_header(tmp_path):
    prog = tmp_path / "alayout.c"
    lines = ['printf("%zu\\n", sizeof(rt_adaptive));']
    lines += ['printf("%%zu\\n", offsetof(rt_adaptive, %s));' % f for f in FIELDS]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0;\n}\n'
                    % (HEADER, "\n".join(lines)))
    exe = tmp_path / "alayout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    a = rt.abi
    assert got[0] == C.sizeof(a.rt_adaptive) == 16
    assert got[1:] == [getattr(a.rt_adaptive, f).offset for f in FIELDS] == [0, 4, 8]
    assert [n for n, _ in a.rt_adaptive._fields_] == FIELDS
    ad = rt.RenderContext.adaptive(0.005, 3)
    assert (ad.min_samples, ad.reserved, ad.tolerance) == (3, 0, 0.005)
    assert rt.RenderContext.adaptive(0.25).min_samples == 0


def test_null_context_is_invalid_without_a_device():
    lib = rt.load_library()
    buf = (C.c_char * 256)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    cam = rt.abi.rt_camera()
    cam.samples = 16
    ad = rt.RenderContext.adaptive(0.005, 2)
    chunks, passes = C.c_int(-7), C.c_int(-7)
    for c in (None, C.byref(cam)):
        for a in (None, C.byref(ad)):
            assert lib.rt_render_camera_adaptive_async(None, c, a, 0, 1, p, p, p, None) == rt.abi.RT_E_INVALID
            msg = lib.rt_last_error()
            assert b"NULL context" in msg and b"rt_render_camera_adaptive_async" in msg
            assert lib.rt_render_camera_adaptive_plan(None, c, a, 0, 1, C.byref(chunks), C.byref(passes)) \
                == rt.abi.RT_E_INVALID
            msg = lib.rt_last_error()
            assert b"NULL context" in msg and b"rt_render_camera_adaptive_plan" in msg
    assert (chunks.value, passes.value) == (-7, -7)


def test_cli_flags_reach_rt_adaptive_and_nothing_without_them():
    from go_raytracer_amd import cli
    ap = cli.build_parser()
    for argv in (["x.gml"], ["--samples", "16", "x.gml"], ["--stats", "--camera", "ortho", "--extent", "3", "x.gml"]):
        assert cli.adaptive_from_args(ap.parse_args(argv)) is None
    a = ap.parse_args(["--adaptive", "0.005", "x.gml"])
    ad = cli.adaptive_from_args(a)
    assert isinstance(ad, rt.abi.rt_adaptive) and (ad.tolerance, ad.min_samples, ad.reserved) == (0.005, 0, 0)
    assert cli.camera_from_args(a) is None and a.samples_map is None  # the camera flags stay what they were
    a = ap.parse_args(["--adaptive", "0.02", "--min-samples", "3", "--samples", "20", "--samples-map", "n.png", "x.gml"])
    ad = cli.adaptive_from_args(a)
    assert (ad.tolerance, ad.min_samples, ad.reserved) == (0.02, 3, 0)
    assert cli.camera_from_args(a).samples == 20 and a.samples_map == "n.png"
    # the other two flags mean nothing without --adaptive
    for argv in (["--min-samples", "3", "x.gml"], ["--samples-map", "n.png", "x.gml"]):
        with pytest.raises(SystemExit):
            cli.adaptive_from_args(ap.parse_args(argv))


def test_samples_map_scales_to_the_cap():
    import numpy as np
    from go_raytracer_amd import cli
    g = cli.samples_image(np.array([[2, 4], [8, 16]], dtype=np.int32), 16)
    assert g.shape == (2, 2, 3) and g.dtype == np.uint8
    assert g[..., 0].tolist() == [[31, 63], [127, 255]] and (g[..., 0] == g[..., 1]).all() and (g[..., 1] == g[..., 2]).all()
