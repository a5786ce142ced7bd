"""The ray-query part of the C ABI (include/rt_abi.h rt_ray, rt_hit,
rt_query_closest_async, rt_query_occluded_async): declared, exported, laid out
as the ctypes mirrors and numpy dtypes say. No device calls (CPU-only)."""
import ctypes as C
import os
import re
import subprocess

import go_raytracer_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_abi.h")
FUNCS = ["rt_query_closest_async", "rt_query_occluded_async"]
RAY_FIELDS = ["origin", "dir", "tmax", "exclude", "reserved"]
HIT_FIELDS = ["t", "point_obj", "point_world", "normal_world", "object", "face", "kind", "material"]


def test_header_declares_both_functions():
    src = open(HEADER).read()
    names = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(rt_\w+)\s*\(", src, re.M))
    for n in FUNCS:
        assert n in names
    assert "#define RT_ABI_VERSION 6" in src  # additive: the version stays


def test_library_exports_both_functions():
    lib = rt.load_library()
    for n in FUNCS:
        assert hasattr(lib, n), n


def test_ray_and_hit_layout_matches_header(tmp_path):
    prog = tmp_path / "qlayout.c"
    lines = ['printf("%zu %zu\\n", sizeof(rt_ray), sizeof(rt_hit));']
    lines += ['printf("%%zu\\n", offsetof(rt_ray, %s));' % f for f in RAY_FIELDS]
    lines += ['printf("%%zu\\n", offsetof(rt_hit, %s));' % f for f in HIT_FIELDS]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0;\n}\n'
                    % (HEADER, "\n".join(lines)))
    exe = tmp_path / "qlayout"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    a = rt.abi
    mirror = [C.sizeof(a.rt_ray), C.sizeof(a.rt_hit)] + [getattr(a.rt_ray, f).offset for f in RAY_FIELDS] + \
        [getattr(a.rt_hit, f).offset for f in HIT_FIELDS]
    dtypes = [a.RAY_DTYPE.itemsize, a.HIT_DTYPE.itemsize] + [a.RAY_DTYPE.fields[f][1] for f in RAY_FIELDS] + \
        [a.HIT_DTYPE.fields[f][1] for f in HIT_FIELDS]
    assert got[:2] == [64, 96]
    assert got == mirror
    assert got == dtypes
    assert list(a.RAY_DTYPE.names) == RAY_FIELDS and list(a.HIT_DTYPE.names) == HIT_FIELDS
    assert [n for n, _ in a.rt_ray._fields_] == RAY_FIELDS and [n for n, _ in a.rt_hit._fields_] == HIT_FIELDS


def test_null_context_is_invalid_without_a_device():
    lib = rt.load_library()
    buf = (C.c_char * 256)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    for n in FUNCS:
        assert getattr(lib, n)(None, 1, p, p, None) == rt.abi.RT_E_INVALID
        assert b"NULL context" in lib.rt_last_error()
