"""The compiled surface programs of tests/vm_ops.py against the GML interpreter
(CPU): gml/surface_compiler.py's words, run by tests/vm_emu.py and
tests/vm_emu_ext.py (the restatements of the device VM), must give what
gml.eval_surface_fn (the restatement of EvalSurfaceFn) gives, and flag an
error exactly where it raises. The rest asserts what the programs and operands
reach, so that the device test on the same cases means what it says."""
import math

import pytest

from go_raytracer_amd.gml.surface_compiler import EXT_OPS, OPS
import vm_emu
import vm_emu_ext
import vm_ops as V

NAMES = OPS + EXT_OPS
INT64_MIN = -(1 << 63)


def _emitted(name):
    words, _ = V.compiled(name)
    return {NAMES[w & 0xFF] for w in words[::2]}


@pytest.mark.parametrize("name", sorted(V.PROGRAMS))
def test_compiled_program_equals_the_interpreter(name):
    words, consts = V.compiled(name)
    run = vm_emu_ext.run if V.PROGRAMS[name][1] else vm_emu.run
    want = V.expected(name)
    good = 0
    for (face, u, v), w in zip(V.cases(name), want):
        out, err = run(words, consts, face, u, v)
        assert err == (w is None), (name, face, u, v, "error flag", err)
        if w is not None:  # (a failed evaluation's registers are not part of the contract)
            assert V.same_fields(out, w), (name, face, u, v, out, w)
            good += 1
    assert good >= 50, (name, good)


def test_every_opcode_the_compiler_can_emit_is_emitted():
    seen = set()
    for name in V.PROGRAMS:
        seen |= _emitted(name)
    assert set(NAMES) - seen == set(V.NOT_EMITTED), sorted(set(NAMES) - seen)
    # one family per program: a failure names it
    assert {"ADDF", "SUBF", "MULF", "DIVF", "NEGF"} <= _emitted("float_arith")
    assert {"LTF", "EQF", "LTI", "EQI", "SEL", "AND", "NOT", "OR", "ERR", "TBL"} <= _emitted("compare_select")
    assert {"ADDI", "SUBI", "MULI", "DIVI", "MODI", "NEGI", "LTI", "EQI", "REAL", "FLOOR"} <= _emitted("int_arith")
    assert {"FLOOR", "FRAC", "CLAMPF", "SQRT"} <= _emitted("floor_frac_clamp_sqrt")
    assert {"SIN", "COS"} <= _emitted("sin_cos")
    assert {"ASIN", "ACOS"} <= _emitted("asin_acos")
    assert {"TBL", "ERR", "SEL"} <= _emitted("get") and {"TBL", "MULI", "ADDI"} <= _emitted("get_nested")
    assert not _emitted("float_arith") & set(EXT_OPS)


def test_operands_reach_the_edges():
    ops = V.OPERANDS
    fl = {x: V.floor_i(x) for x in ops if x == x}
    pairs = [(V.floor_i(u), V.floor_i(v)) for _, u, v in V.cases("int_arith")]
    # integer arithmetic
    assert (INT64_MIN, -1) in pairs, "MinInt64 / -1"
    assert any(i < 0 and j > 1 and abs(i) % j for i, j in pairs), "modi of a negative dividend with a remainder"
    assert any(j == 0 for i, j in pairs), "integer division by zero"
    errors = sum(w is None for w in V.expected("int_arith"))
    assert errors == sum(j == 0 for i, j in pairs) > 0
    assert any(abs(i + j) > (1 << 53) and (i + j) % 2 for i, j in pairs if abs(i + j) < (1 << 63)), "real of an odd integer above 2^53"
    assert any(abs(i * j) >= (1 << 63) for i, j in pairs), "muli that wraps"
    # floor: MinInt64 from overflow (both signs beyond 2^63, +-Inf) and from NaN
    assert fl[V.P2_63] == INT64_MIN and fl[9.3e18] == INT64_MIN and fl[-9.3e18] == INT64_MIN and fl[math.inf] == INT64_MIN
    assert fl[-V.P2_63] == INT64_MIN  # exact, not an overflow
    assert V.floor_i(math.nan) == INT64_MIN and any(x != x for x in ops)
    assert fl[-0.5] == -1 and fl[-2.5] == -3 and fl[1e-310] == 0 and fl[V.P2_53 - 1.0] == (1 << 53) - 1
    # float division by a zero of each sign, with dividends of each sign, zero and NaN
    zeros = [x for x in ops if x == 0]
    assert sorted(math.copysign(1.0, z) for z in zeros) == [-1.0, 1.0]
    # comparisons see NaN and both zeros; clampf sees NaN, Inf and values inside and outside
    assert any(x > 1 for x in ops) and any(x < 0 for x in ops) and any(0 < x < 1 for x in ops)
    assert 1e-310 in ops and 0.7 in ops and V.BEYOND_TRIG in ops and V.BEYOND_TRIG not in V.TRIG_OPERANDS
    # sin / cos: every octant, on both sides of zero
    from gomath_inputs import octant
    from go_raytracer_amd.gml.evaluator import DEG_TO_RAD
    trig = [x for x in V.TRIG_OPERANDS if math.isfinite(x)]
    assert {octant(DEG_TO_RAD * x) for x in trig if x > 0} == set(range(8))
    assert {octant(DEG_TO_RAD * x) for x in trig if x < 0} == set(range(8))
    assert len(V.TRIG_OPERANDS) >= 50 and len(ops) >= 60
    # get: an error on each side of the array, and both ends without one
    idx = [(V.floor_i(u), w) for (_, u, v), w in zip(V.cases("get"), V.expected("get"))]
    assert any(i == -1 and w is None for i, w in idx) and any(i >= 3 and w is None for i, w in idx)
    assert any(i == 0 and w is not None for i, w in idx) and any(i == 2 and w is not None for i, w in idx)
    assert all((w is None) == (not 0 <= i <= 2) for i, w in idx)
    sums = [(V.floor_i(u + v), V.floor_i(u), V.floor_i(v), w)
            for (_, u, v), w in zip(V.cases("get_nested"), V.expected("get_nested")) if u + v == u + v]
    assert any(s == 3 and 0 <= i <= 2 and 0 <= j <= 2 and w is None for s, i, j, w in sums), "index == length"
    assert any(w is not None for s, i, j, w in sums)
