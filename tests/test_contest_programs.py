"""The contest programs chess.gml, snowgoon.gml and large.gml on the host:
cone CSG leaves, asin / acos / real in the interpreter and the surface
compiler, register reuse, and evaluation 25 000 applies deep. (The renders
are in test_gpu_contest_programs.py.)"""
import ctypes
import json
import math
import os
import random
import struct

import pytest

import go_raytracer_amd as rt
from go_raytracer_amd import abi as A
from go_raytracer_amd import gml, gomath
from go_raytracer_amd.gml import surface_compiler as SC
from go_raytracer_amd.gml.surface_compiler import CompileError, compile_surface
import contest_common as CC
import oracle_bind
import vm_emu_ext


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _material_bits(m):
    vals = list(m.color) + [m.reflectivity, m.fuzziness, m.transparency, m.refractive_index,
                            m.kd, m.ks, m.specular_exponent]
    return [_bits(float(x)) for x in vals]


@pytest.mark.parametrize("name", CC.PROGRAMS)
def test_contest_program_converts(name):
    frames = CC.rendered(name)
    assert len(frames) == 1
    args, _ = frames[0]
    packed = rt.scene.convert(args)
    s = packed.scene
    for pc in range(0, s.program_code_words, 2):
        w0 = s.program_code[pc]
        regs = [(w0 >> 8) & 0xFF, (w0 >> 16) & 0xFF, w0 >> 24]
        if (w0 & 0xFF) == SC.OP["SEL"]:
            regs.append(s.program_code[pc + 1])
        assert max(regs) < SC.MAX_REGS, (name, pc)
    kinds = [s.csg_leaves[i].kind for i in range(s.num_csg_leaves)]
    if name == "chess":
        assert kinds.count(A.RT_CONE) == 24 and s.num_objects == 61 and s.num_programs == 25
    if name == "snowgoon":
        assert kinds.count(A.RT_CONE) == 1 and s.num_objects == 5
    if name == "large":  # 8 spheres and a directional light
        assert s.num_objects == 8 and s.num_csg_leaves == 0 and s.num_ext_lights == 1
        assert all(s.objects[i].kind == A.RT_SPHERE for i in range(8))
        assert s.ext_lights[0].kind == A.RT_LIGHT_DIRECTIONAL


def _acos_inputs():
    rng = random.Random(2000)
    xs = [rng.uniform(-1.0, 1.0) for _ in range(9000)]
    xs += [s * (0.7 + k * 2.0 ** -53) for s in (1, -1) for k in range(-300, 301)]  # the branch point
    xs += [0.0, -0.0, 1.0, -1.0, math.nan, math.inf, -math.inf, 5e-324, -5e-324, 1e-300, 0.66, 0.7]
    xs += [s * math.nextafter(1.0, d) for s in (1, -1) for d in (0.0, 2.0)]  # just inside / outside
    xs += [s * (1.0 + rng.random()) for s in (1, -1) for _ in range(100)]
    xs += [s * 2.0 ** -k for s in (1, -1) for k in range(1, 60)]
    return xs


def test_go_acos_equals_the_oracle():
    lib = oracle_bind.lib()
    xs = _acos_inputs()
    assert len(xs) >= 10000
    for x in xs:
        got, ref = gomath.go_acos(x), lib.oracle_go_acos(x)
        if ref != ref:
            assert got != got, x
        else:
            assert _bits(got) == _bits(ref), x
        # Acos(x) = Pi/2 - Asin(x) (asin.go): the two restatements agree
        a = gomath.go_asin(x)
        if ref == ref:
            assert _bits(gomath.PI_2 - a) == _bits(ref), x
        else:
            assert a != a, x
    assert _bits(gomath.go_asin(-0.0)) == _bits(-0.0) and gomath.go_asin(1.0) == gomath.PI_2
    assert gomath.go_asin(-1.0) == -gomath.PI_2 and abs(gomath.go_asin(0.5) - math.pi / 6) < 1e-15
    for x in xs[:500]:
        assert _bits(gomath.go_asin(-x)) == _bits(-gomath.go_asin(x)), x


# math.Asin as the oracle's C restatement (oracle/go_math.h go_asin, which the
# library does not export) computes it, across the 0.66 / 0.7 / tan(3 pi / 8)
# branches of asin.go and atan.go: (x, bits of the result)
_ASIN_PINS = [
    (0.1, 0x3fb9a49276037884), (0.25, 0x3fd02be9ce0b87cd), (0.5, 0x3fe0c152382d7366),
    (0.55, 0x3fe2a2ba538032f0), (0.6, 0x3fe4978fa3269ee0), (0.62, 0x3fe5665718f62b98),
    (0.66, 0x3fe710f28188f80c), (0.69, 0x3fe85e1e4a3a04f1), (0.7, 0x3fe8d00e692afd95),
    (0.7000000000000001, 0x3fe8d00e692afd96), (0.71, 0x3fe94391bfac8e4b), (0.75, 0x3feb235315c680dc),
    (0.9, 0x3ff1ea93705fa172), (0.99, 0x3ff6de3c6f33d51d), (0.999999, 0x3ff91c306b2c1389),
    (1.0, 0x3ff921fb54442d18), (-0.3, 0xbfd380159e14f6ff), (-0.7, 0xbfe8d00e692afd95),
    (-0.95, 0xbff40d41159f3409), (1e-08, 0x3e45798ee2308c3b), (3e-05, 0x3eff75104d69618f),
]


def test_go_asin_pinned_values():
    for x, bits in _ASIN_PINS:
        got = gomath.go_asin(x)
        assert _bits(got) == bits, (x, hex(_bits(got)))
        # and close to the platform's asin, so the pins are not a wrong table copied twice. Go's
        # asin forms sqrt(1 - x*x): the rounding of x*x (2^-53) is divided by sqrt(1 - x*x) near 1
        c = math.sqrt(1 - x * x)
        assert x == 1.0 or abs(got - math.asin(x)) <= 4 * math.ulp(got) + 2.0 ** -53 / c, x


def test_asin_acos_real_in_the_interpreter():
    src = "0.5 asin /a 0.5 acos /b 2.0 asin /c 7 real /d -3 real /e"
    _, st = gml.run_text(src, extensions=True)
    val = {n: st.env[st.ids.name_id[n]] for n in "abcde"}
    assert float(val["a"]) == 57.29577951308232 * gomath.go_asin(0.5)
    assert abs(float(val["a"]) - 30.0) < 1e-13 and abs(float(val["b"]) - 60.0) < 1e-13
    assert float(val["c"]) != float(val["c"])
    assert float(val["d"]) == 7.0 and float(val["e"]) == -3.0
    with pytest.raises(gml.GMLError, match="unbound identifier: asin"):
        gml.run_text("0.5 asin")


def _check_against_interpreter(state, sf, tag):
    prog = compile_surface(sf, state.stack, True)
    words = CC.encode(prog)
    assert prog.nreg <= SC.MAX_REGS
    for face, u, v in CC.grid():
        out, err = vm_emu_ext.run(words, prog.consts, face, u, v)
        try:
            m = gml.eval_surface_fn(face, u, v, state.clone(), sf)
        except gml.GMLError:
            assert err, (tag, face, u, v)
            continue
        assert not err, (tag, face, u, v)
        assert [_bits(x) for x in out] == _material_bits(m), (tag, face, u, v)
    return prog


def test_chess_surfaces_compile_to_what_the_interpreter_computes():
    args, _ = CC.rendered("chess")[0]
    state, sfs = CC.surface_programs(args)
    assert len(sfs) == 25
    ext_ops = 0
    for k, sf in enumerate(sfs):
        prog = _check_against_interpreter(state, sf, "chess %d" % k)
        ext_ops += sum(1 for ins in prog.code if ins[0] >= len(SC.OPS))
    assert ext_ops > 0  # chess uses asin / acos on run-time values


def test_real_asin_acos_surface_compiles_to_what_the_interpreter_computes():
    args, _ = CC.ext_rendered()[0]
    state, sfs = CC.surface_programs(args)
    assert len(sfs) == 1
    prog = _check_against_interpreter(state, sfs[0], "ext")
    used = {ins[0] for ins in prog.code}
    assert {SC.OP["ASIN"], SC.OP["ACOS"], SC.OP["REAL"]} <= used
    assert SC.OP["ASIN"] == A.RT_VM_EXT_ASIN == 32 and SC.OP["ACOS"] == A.RT_VM_EXT_ACOS == 33
    assert SC.OP["REAL"] == A.RT_VM_EXT_REAL == 34 and len(SC.OPS) == 32
    # NaN for |argument| > 1, on both sides (checked bit for bit above)
    out, err = vm_emu_ext.run(CC.encode(prog), prog.consts, 0, 1.5, -1.25)
    assert not err and out[0] != out[0] and out[1] != out[1]
    # constant operands fold at compile time
    rendered, _ = gml.run_text("{ /v /u /face 0.5 asin 90.0 divf 0.25 acos 90.0 divf 3 real point u 0.5 1.0 } sphere /s "
                               "0.1 0.1 0.1 point [ ] s 1 90.0 8 6 \"x.ppm\" render", extensions=True)
    a2 = rendered[0][0]
    p2 = compile_surface(a2.scene.surface, a2.state.stack, True)
    assert all(ins[0] < len(SC.OPS) for ins in p2.code)
    # ... and without the extensions the names are ordinary identifiers
    with pytest.raises(CompileError, match="unbound identifier: asin"):
        compile_surface(sfs[0], state.stack, False)


def test_other_fixture_programs_compile_to_the_recorded_words():
    """Programs that fit the register file as first numbered are emitted
    unchanged: golden/surface_words.json holds the code, constants and entry
    points recorded before register reuse existed."""
    with open(os.path.join(CC.GOLDEN, "surface_words.json")) as f:
        gold = json.load(f)
    assert sorted(gold) == sorted(["cube", "sphere", "cylinder", "golf", "dice", "house", "pipe", "fractal"])
    for name, frames in gold.items():
        got = CC.rendered(name)
        assert len(got) == len(frames), name
        for (args, _), ref in zip(got, frames):
            s = rt.scene.convert(args).scene
            assert [s.program_entry[i] for i in range(s.num_programs)] == ref["entry"], name
            assert [s.program_code[i] for i in range(s.program_code_words if s.num_programs else 0)] == ref["code"], name
            assert ["%016x" % s.program_consts[i] for i in range(s.program_const_count if s.num_programs else 0)] == \
                ref["consts"], name


def _surface_of(src):
    rendered, _ = gml.run_text(src + " sphere /s 0.1 0.1 0.1 point [ ] s 1 90.0 8 6 \"x.ppm\" render", extensions=True)
    args, _ = rendered[0]
    return args.state, args.scene.surface


def _many_values(n, tail):
    """A surface binding n run-time values u*(k+1.5)+v (each its own constant), then `tail`."""
    body = " ".join("u %d.5 mulf v addf /x%d" % (k + 1, k) for k in range(n))
    return "{ /v /u /face " + body + " " + tail + " }"


def _sum_of(n):
    return "x0 " + " ".join("x%d addf" % k for k in range(1, n))


def test_registers_are_reused_when_the_first_numbering_runs_out():
    # 40 values live at once, 40 constants and 80 intermediates: > 64 as first numbered
    state, sf = _surface_of(_many_values(40, _sum_of(40) + " /t t t t point 0.5 0.5 2.0"))
    prog = _check_against_interpreter(state, sf, "reuse")
    assert 13 + 40 <= prog.nreg <= SC.MAX_REGS
    assert len(prog.code) >= 160  # (each instruction but the outputs' defines a value)


def test_a_distant_constant_is_loaded_again():
    # 30 constants read at the start and again at the end, 40 values live in between
    n = 40
    first = "0.0 " + " ".join("u %d.25 mulf addf" % k for k in range(30)) + " /h"
    body = " ".join("u %d.5 mulf v addf /x%d" % (k + 1, k) for k in range(n))
    last = "0.0 " + " ".join("v %d.25 mulf addf" % k for k in range(30)) + " /g"
    src = "{ /v /u /face " + first + " " + body + " " + last + " " + _sum_of(n) + " h addf g addf /t t t t point 0.5 0.5 2.0 }"
    state, sf = _surface_of(src)
    prog = _check_against_interpreter(state, sf, "remat")
    loads = [ins[4] for ins in prog.code if ins[0] == SC.OP["CONST"]]
    assert len(loads) > len(set(loads))  # some constant has a second CONST


def test_more_live_values_than_registers_is_still_an_error():
    state, sf = _surface_of(_many_values(70, _sum_of(70) + " /t t t t point 0.5 0.5 2.0"))
    with pytest.raises(CompileError, match="more than 64 registers"):
        compile_surface(sf, state.stack, True)


def test_deep_recursion_keeps_the_callers_environment_on_errors():
    """`apply` / `if` bodies run on an explicit frame stack: 25 000 deep works,
    and an error inside leaves the environment of the outermost caller, as the
    nested EvalClosure calls did."""
    loop = "{ /self /n n 0 eqi { 0 } { n 1 subi self self apply 1 addi } if } /f "
    _, st = gml.run_text(loop + "25000 f f apply /r")
    assert int(st.env[st.ids.name_id["r"]]) == 25000 and not st.stack
    st2 = gml.EvalState()
    st2.parse_and_eval("1 /outer { /x { 1 0 divi } apply } /g")
    names = lambda: sorted(st2.ids.id_name[i] for i in st2.env)
    assert names() == ["g", "outer"]
    with pytest.raises(gml.GMLError, match="integer divide by zero"):
        st2.parse_and_eval("5 g apply")
    assert names() == ["g", "outer"]  # not the closure's environment with x


def test_a_specialised_kernel_with_cone_leaves_compiles():
    """The embedded kernel sources build for a key whose kind mask holds the
    cone next to CSG composites (no device needed)."""
    lib = rt.load_library()
    ms = ctypes.c_double()
    key = "1:0:1:0::63:1:2:7:0:0:0:1"  # scene in LDS, CSG, every kind, closure surfaces, 2 lights
    rc = lib.rt_debug_spec_compile(key.encode(), ctypes.byref(ms))
    assert rc == 0, (key, (lib.rt_last_error() or b"").decode(errors="replace")[-500:])
