"""The radiance-query part of the C ABI (include/rt_abi.h rt_radiance,
rt_query_radiance_async, rt_query_camera_rays_async): declared, exported, laid
out as the ctypes mirror and numpy dtype say. No device calls (CPU-only)."""
import ctypes as C
import os
import re
import subprocess

import go_raytracer_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_abi.h")
FUNCS = ["rt_query_radiance_async", "rt_query_camera_rays_async"]
FIELDS = ["color", "object", "rays"]


def test_header_declares_both_functions_and_the_record():
    src = open(HEADER).read()
    names = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(rt_\w+)\s*\(", src, re.M))
    for n in FUNCS + ["rt_query_radiance_lanes"]:
        assert n in names
    assert re.search(r"typedef struct rt_radiance\s*\{", src) and "#define RT_RADIANCE_MAX_DEPTH 32" in src
    assert "#define RT_ABI_VERSION 6" in src  # additive: the version stays


def test_library_exports_both_functions():
    lib = rt.load_library()
    for n in FUNCS + ["rt_query_radiance_lanes"]:
        assert hasattr(lib, n), n


def test_radiance_layout_matches_header(tmp_path):
    prog = tmp_path / "rlayout.c"
    lines = ['printf("%zu %d\\n", sizeof(rt_radiance), RT_RADIANCE_MAX_DEPTH);']
    lines += ['printf("%%zu\\n", offsetof(rt_radiance, %s));' % f for f in FIELDS]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0;\n}\n'
                    % (HEADER, "\n".join(lines)))
    exe = tmp_path / "rlayout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    a = rt.abi
    assert got[:2] == [32, 32] and a.RT_RADIANCE_MAX_DEPTH == 32
    assert got[0] == C.sizeof(a.rt_radiance) == a.RADIANCE_DTYPE.itemsize
    assert got[2:] == [getattr(a.rt_radiance, f).offset for f in FIELDS]
    assert got[2:] == [a.RADIANCE_DTYPE.fields[f][1] for f in FIELDS]
    assert list(a.RADIANCE_DTYPE.names) == FIELDS and [n for n, _ in a.rt_radiance._fields_] == FIELDS


def test_null_context_is_invalid_without_a_device():
    lib = rt.load_library()
    buf = (C.c_char * 256)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    assert lib.rt_query_radiance_async(None, 1, p, 0, p, None) == rt.abi.RT_E_INVALID
    assert b"NULL context" in lib.rt_last_error() and b"rt_query_radiance_async" in lib.rt_last_error()
    assert lib.rt_query_camera_rays_async(None, 0, 1, p, None) == rt.abi.RT_E_INVALID
    assert b"NULL context" in lib.rt_last_error() and b"rt_query_camera_rays_async" in lib.rt_last_error()
    assert lib.rt_query_radiance_lanes(None, 3) == rt.abi.RT_E_INVALID
