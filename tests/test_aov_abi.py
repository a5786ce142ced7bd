"""The feature-buffer and denoiser part of the C ABI (include/rt_abi.h
rt_aov_out, rt_render_camera_aov_async, rt_denoise, rt_denoise_atrous_async):
declared, exported, laid out as the ctypes mirror says, and reached by the CLI
flags. No device calls (CPU-only)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import go_raytracer_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_abi.h")
FUNCS = ["rt_render_camera_aov_async", "rt_denoise_atrous_async"]
AOV_FIELDS = ["depth", "normal", "albedo", "coverage", "ids"]
DN_FIELDS = ["iterations", "reserved", "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"]


def test_header_declares_the_functions_and_the_records():
    src = open(HEADER).read()
    names = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(rt_\w+)\s*\(", src, re.M))
    for n in FUNCS:
        assert n in names
    assert re.search(r"typedef struct rt_aov_out\s*\{", src)
    assert re.search(r"typedef struct rt_denoise\s*\{", src)
    assert "#define RT_ABI_VERSION 6" in src  # additive: the version stays
    # the rule's fixed points are in the header's text
    for text in ("1/16, 1/4, 3/8, 1/4, 1/16", "kern(x) = x < 1.0 ? (1.0 - x) * (1.0 - x) : 0.0", "step = 1 << i",
                 "coverage = (double)h * inv", "depth = h > 0 ? zt / (double)h : +inf"):
        assert text in src, text


def test_library_exports_the_functions():
    lib = rt.load_library()
    for n in FUNCS:
        assert hasattr(lib, n), n
    assert lib.rt_abi_version() == 6


def test_layouts_match_header(tmp_path):
    prog = tmp_path / "layout.c"
    lines = ['printf("%zu\\n", sizeof(rt_aov_out));']
    lines += ['printf("%%zu\\n", offsetof(rt_aov_out, %s));' % f for f in AOV_FIELDS]
    lines += ['printf("%zu\\n", sizeof(rt_denoise));']
    lines += ['printf("%%zu\\n", offsetof(rt_denoise, %s));' % f for f in DN_FIELDS]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0;\n}\n'
                    % (HEADER, "\n".join(lines)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    a = rt.abi
    assert got[0] == C.sizeof(a.rt_aov_out) == 40
    assert got[1:6] == [getattr(a.rt_aov_out, f).offset for f in AOV_FIELDS] == [0, 8, 16, 24, 32]
    assert [n for n, _ in a.rt_aov_out._fields_] == AOV_FIELDS
    assert got[6] == C.sizeof(a.rt_denoise) == 40
    assert got[7:] == [getattr(a.rt_denoise, f).offset for f in DN_FIELDS] == [0, 4, 8, 16, 24, 32]
    assert [n for n, _ in a.rt_denoise._fields_] == DN_FIELDS
    assert a.AOV_IDS_DTYPE.itemsize == 16 and a.AOV_IDS_DTYPE.names == ("object", "face", "kind", "material")
    assert a.AOV_NAMES == tuple(AOV_FIELDS)
    dn = rt.RenderContext.denoise_params(3, 0.5, 0.25, 2.0, 0.125)
    assert (dn.iterations, dn.reserved, dn.sigma_color, dn.sigma_normal, dn.sigma_depth, dn.sigma_albedo) \
        == (3, 0, 0.5, 0.25, 2.0, 0.125)
    z = rt.RenderContext.denoise_params()
    assert (z.iterations, z.sigma_color, z.sigma_normal, z.sigma_depth, z.sigma_albedo) == (0, 0.0, 0.0, 0.0, 0.0)


def test_null_context_is_invalid_without_a_device():
    lib = rt.load_library()
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    q = C.c_void_p(p.value + 1024)
    cam = rt.abi.rt_camera()
    out = rt.abi.rt_aov_out()
    out.depth = p.value
    for c in (None, C.byref(cam)):
        for o in (None, C.byref(out)):
            assert lib.rt_render_camera_aov_async(None, c, 0, 1, o, None) == rt.abi.RT_E_INVALID
            msg = lib.rt_last_error()
            assert b"NULL context" in msg and b"rt_render_camera_aov_async" in msg
    dn = rt.RenderContext.denoise_params(1, 0.5)
    for d in (None, C.byref(dn)):
        assert lib.rt_denoise_atrous_async(None, d, 4, 4, p, None, None, None, q, None, None, None) \
            == rt.abi.RT_E_INVALID
        msg = lib.rt_last_error()
        assert b"NULL context" in msg and b"rt_denoise_atrous_async" in msg


def test_cli_flags_parse_and_mean_nothing_without_them():
    from go_raytracer_amd import cli
    ap = cli.build_parser()
    for argv in (["x.gml"], ["--samples", "16", "x.gml"], ["--adaptive", "0.01", "x.gml"]):
        a = ap.parse_args(argv)
        assert cli.aov_from_args(a) is None and cli.denoise_from_args(a) is None
    a = ap.parse_args(["--aov", "depth,normal,ids", "x.gml"])
    assert cli.aov_from_args(a) == ("depth", "normal", "ids")
    assert cli.camera_from_args(a) is None and cli.adaptive_from_args(a) is None  # the other flags stay what they were
    a = ap.parse_args(["--aov", "albedo, coverage", "--denoise", "x.gml"])
    assert cli.aov_from_args(a) == ("albedo", "coverage")
    dn = cli.denoise_from_args(a)
    d = rt.render.DENOISE_DEFAULTS
    assert isinstance(dn, rt.abi.rt_denoise) and dn.iterations == 0 and dn.reserved == 0
    assert (dn.sigma_color, dn.sigma_normal, dn.sigma_depth, dn.sigma_albedo) \
        == (d["color"], d["normal"], d["depth"], d["albedo"])
    a = ap.parse_args(["--denoise", "--denoise-iterations", "3", "--denoise-sigmas", "0.5,0,2,0.125", "x.gml"])
    dn = cli.denoise_from_args(a)
    assert (dn.iterations, dn.sigma_color, dn.sigma_normal, dn.sigma_depth, dn.sigma_albedo) == (3, 0.5, 0.0, 2.0, 0.125)
    for argv in (["--aov", "depth,colour", "x.gml"], ["--aov", ",", "x.gml"], ["--denoise-iterations", "3", "x.gml"],
                 ["--denoise-sigmas", "1,1,1,1", "x.gml"], ["--denoise", "--denoise-sigmas", "1,1,1", "x.gml"]):
        a = ap.parse_args(argv)
        with pytest.raises(SystemExit):
            cli.aov_from_args(a)
            cli.denoise_from_args(a)


def test_views_are_opaque_8_bit_frames():
    from go_raytracer_amd import cli
    depth = np.array([[2.0, 4.0], [np.inf, 3.0]])
    g = cli.aov_view("depth", depth)
    assert g.shape == (2, 2, 3) and g.dtype == np.uint8
    assert g[0, 0, 0] == 255 and g[1, 0, 0] == 0 and g[0, 0, 0] > g[1, 1, 0] > g[0, 1, 0] > 0  # near is bright
    n = cli.aov_view("normal", np.array([[[0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]]))
    assert n.tolist() == [[[127, 127, 0], [255, 127, 127]]]
    assert cli.aov_view("albedo", np.array([[[0.5, 2.0, -1.0]]])).tolist() == [[[127, 255, 0]]]
    assert cli.aov_view("coverage", np.array([[0.0, 1.0]])).tolist() == [[[0, 0, 0], [255, 255, 255]]]
