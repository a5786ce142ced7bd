"""The camera-render part of the C ABI (include/rt_abi.h rt_camera,
rt_camera_rays_async, rt_render_camera_async, rt_render_camera_chunks):
declared, exported, laid out as the ctypes mirror says. No device calls
(CPU-only)."""
import ctypes as C
import os
import re
import subprocess

import go_raytracer_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_abi.h")
FUNCS = ["rt_camera_rays_async", "rt_render_camera_async", "rt_render_camera_chunks"]
FIELDS = ["model", "flags", "samples", "width", "height", "depth", "chunk_pixels", "reserved", "fov", "extent",
          "aperture", "focus", "eye", "look_at", "up"]
CONSTS = ["RT_CAMERA_PINHOLE", "RT_CAMERA_ORTHO", "RT_CAMERA_EQUIRECT", "RT_CAMERA_THINLENS", "RT_CAMERA_POSED",
          "RT_CAMERA_MAX_SAMPLES"]


def test_header_declares_the_functions_and_the_record():
    src = open(HEADER).read()
    names = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(rt_\w+)\s*\(", src, re.M))
    for n in FUNCS:
        assert n in names
    assert re.search(r"typedef struct rt_camera\s*\{", src)
    assert "#define RT_ABI_VERSION 6" in src  # additive: the version stays
    # the older export stays as it is
    assert "rt_query_camera_rays_async" in names


def test_library_exports_the_functions():
    lib = rt.load_library()
    for n in FUNCS:
        assert hasattr(lib, n), n


def test_camera_layout_matches_header(tmp_path):
    prog = tmp_path / "clayout.c"
    lines = ['printf("%zu\\n", sizeof(rt_camera));']
    lines += ['printf("%%zu\\n", offsetof(rt_camera, %s));' % f for f in FIELDS]
    lines += ['printf("%%d\\n", %s);' % c for c in CONSTS]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0;\n}\n'
                    % (HEADER, "\n".join(lines)))
    exe = tmp_path / "clayout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    a = rt.abi
    assert got[0] == C.sizeof(a.rt_camera) == 8 * 4 + 4 * 8 + 9 * 8
    assert got[1:1 + len(FIELDS)] == [getattr(a.rt_camera, f).offset for f in FIELDS]
    assert [n for n, _ in a.rt_camera._fields_] == FIELDS
    assert got[1 + len(FIELDS):] == [getattr(a, c) for c in CONSTS] == [0, 1, 2, 3, 1, 1024]
    assert a.CAMERA_MODELS == {"pinhole": 0, "ortho": 1, "equirect": 2, "thinlens": 3}
    # the zero camera is what a fresh record holds
    assert bytes(a.rt_camera()) == b"\0" * got[0]


def test_null_context_is_invalid_without_a_device():
    lib = rt.load_library()
    buf = (C.c_char * 256)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    cam = rt.abi.rt_camera()
    for c in (None, C.byref(cam)):
        assert lib.rt_camera_rays_async(None, c, 0, 1, p, None) == rt.abi.RT_E_INVALID
        assert b"NULL context" in lib.rt_last_error() and b"rt_camera_rays_async" in lib.rt_last_error()
        assert lib.rt_render_camera_async(None, c, 0, 1, p, p, None) == rt.abi.RT_E_INVALID
        assert b"NULL context" in lib.rt_last_error() and b"rt_render_camera_async" in lib.rt_last_error()
        assert lib.rt_render_camera_chunks(None, c, 0, 1) == rt.abi.RT_E_INVALID
        assert b"NULL context" in lib.rt_last_error() and b"rt_render_camera_chunks" in lib.rt_last_error()


def test_cli_flags_build_the_camera_and_none_without_them():
    from go_raytracer_amd import cli
    a = rt.abi
    ap = cli.build_parser()
    assert cli.camera_from_args(ap.parse_args(["x.gml"])) is None
    assert cli.camera_from_args(ap.parse_args(["--stats", "--out-dir", "o", "--extensions", "x.gml"])) is None
    cam = cli.camera_from_args(ap.parse_args(["--samples", "16", "x.gml"]))
    assert (cam.model, cam.samples, cam.flags, cam.width, cam.height) == (a.RT_CAMERA_PINHOLE, 16, 0, 0, 0)
    cam = cli.camera_from_args(ap.parse_args(
        ["--camera", "thinlens", "--aperture", "0.25", "--focus", "6", "--eye", "1", "2", "-3", "--up", "0.1", "1", "0",
         "--fov", "40", "--size", "64x48", "x.gml"]))
    assert (cam.model, cam.samples, cam.flags) == (a.RT_CAMERA_THINLENS, 0, a.RT_CAMERA_POSED)
    assert (cam.width, cam.height, cam.fov, cam.aperture, cam.focus) == (64, 48, 40.0, 0.25, 6.0)
    assert list(cam.eye) == [1.0, 2.0, -3.0] and list(cam.look_at) == [0.0, 0.0, 0.0] and list(cam.up) == [0.1, 1.0, 0.0]
    cam = cli.camera_from_args(ap.parse_args(["--camera", "ortho", "--extent", "7.5", "--look-at", "0", "1", "5", "x.gml"]))
    assert (cam.model, cam.extent, cam.flags) == (a.RT_CAMERA_ORTHO, 7.5, a.RT_CAMERA_POSED)
    assert list(cam.eye) == [0.0, 0.0, -1.0] and list(cam.look_at) == [0.0, 1.0, 5.0]
    assert cli.camera_from_args(ap.parse_args(["--camera", "equirect", "x.gml"])).model == a.RT_CAMERA_EQUIRECT
