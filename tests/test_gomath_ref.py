"""The Go-math restatements against each other and against mpmath (CPU).

Four hand-copied restatements of Go's math package carry the parity promise:
oracle/go_math.h, csrc/rt_device.h, the host copy in csrc/rt_kernel.hip and
go_raytracer_amd/gomath.py. tests/test_gpu_gomath.py holds the device to the
oracle; here the Python copy is held to the oracle bit for bit, and the oracle
to 200-bit mpmath, which is what catches a coefficient copied wrongly into all
four. Inputs: tests/gomath_inputs.py.
"""
import math

import pytest

import gomath_inputs as GI
import oracle_bind
from go_raytracer_amd import gomath
from go_raytracer_amd.gml import evaluator


@pytest.fixture(scope="module")
def lib():
    return oracle_bind.lib()


@pytest.fixture(scope="module")
def trig():
    return GI.trig()


@pytest.fixture(scope="module")
def asin():
    return GI.asin()


@pytest.fixture(scope="module")
def atan2():
    return GI.atan2()


def _flat(fams):
    return [(name, x) for name, xs in fams.items() for x in xs]


def test_families_are_all_there(trig, asin, atan2):
    for fams in (trig, asin, atan2, GI.f2i()):
        assert all(len(xs) > 0 for xs in fams.values()), {k: len(v) for k, v in fams.items()}
    assert len(trig["degrees"]) == 2881 and len(atan2["special_table"]) == 49
    below = [x for _, x in _flat(trig) if math.isfinite(x) and abs(x) < GI.P2_29]
    seen = {GI.octant(x) for x in below}
    assert seen == set(range(8)), seen
    big = [x for x in below if abs(x) > 1e8]  # the three-part reduction with a large y
    assert len(big) >= 100
    ax = [abs(x) for x in asin["around_satan_0.66"]]
    assert any(a / math.sqrt(1 - a * a) <= 0.66 for a in ax) and any(a / math.sqrt(1 - a * a) > 0.66 for a in ax)
    assert any(abs(x) > 0.7 for x in asin["around_0.7"]) and any(abs(x) <= 0.7 for x in asin["around_0.7"])
    q = [abs(y / x) for y, x in atan2["quotient_thresholds"]]
    assert any(v <= 0.66 for v in q) and any(0.66 < v < 1 for v in q)
    assert any(1 < v <= GI.TAN3PIO8 for v in q) and any(v > GI.TAN3PIO8 for v in q)
    q = [abs(y / x) for y, x in atan2["quotient_underflow_overflow"]]
    assert 0.0 in q and math.inf in q


def test_python_sin_cos_equal_the_oracle(lib, trig):
    """gomath.go_sin / go_cos == oracle go_sin / go_cos, bit for bit, below
    2^29; at and above it the Python copy raises (Payne-Hanek is restated
    nowhere) for every finite argument."""
    raised = 0
    for fam, x in _flat(trig):
        if math.isfinite(x) and abs(x) >= GI.P2_29:
            for fn in (gomath.go_sin, gomath.go_cos):
                with pytest.raises(ValueError):
                    fn(x)
                raised += 1
            continue
        assert GI.same(gomath.go_sin(x), lib.oracle_go_sin(x)), ("sin", fam, x.hex())
        assert GI.same(gomath.go_cos(x), lib.oracle_go_cos(x)), ("cos", fam, x.hex())
    assert raised == 12


def test_python_asin_acos_equal_the_oracle(lib, asin):
    for fam, x in _flat(asin):
        assert GI.same(gomath.go_asin(x), lib.oracle_go_asin(x)), ("asin", fam, x.hex())
        assert GI.same(gomath.go_acos(x), lib.oracle_go_acos(x)), ("acos", fam, x.hex())
    assert GI.bits(lib.oracle_go_acos(-0.0)) == GI.bits(gomath.PI_2)
    assert GI.bits(lib.oracle_go_asin(-0.0)) == GI.bits(-0.0)


def test_python_float_to_int_equals_the_oracle(lib):
    """The interpreter's go_f2i (floor / frac) against the oracle's CVTTSD2SQ."""
    mins = 0
    for fam, x in _flat(GI.f2i()):
        want = lib.oracle_go_f2i(x)
        assert evaluator.go_f2i(x) == want, (fam, x.hex())
        mins += want == -(1 << 63)
    assert mins > 100
    assert lib.oracle_go_f2i(-GI.P2_63) == -(1 << 63) and lib.oracle_go_f2i(GI.ulps(GI.P2_63, -1)) == (1 << 63) - 1024
    assert lib.oracle_go_f2i(-1.5) == -1 and lib.oracle_go_f2i(-0.5) == 0


# Bounds: the next power of two above the oracle's largest error on the fixed
# lists of tests/gomath_inputs.py, measured with the figures in the docstring
# below (a margin below 2x for the difference to other samples). A digit
# wrong at the 12th place of a coefficient moves a result by about 1e-13.
SIN_BOUND = 2.0 ** -52
COS_BOUND = 2.0 ** -52
ASIN_BOUND = 2.0 ** -51
ACOS_BOUND = 2.0 ** -50
ATAN2_BOUND_ULP = 2.0


def test_oracle_equals_mpmath_within_its_own_error(lib, trig, asin, atan2):
    """The oracle against mpmath at 200 bits, on the fixed lists.

    Largest absolute error of sin, cos over |x| < 2^29 and of asin, acos over
    [-1, 1]; largest error of atan2 in units of the result's last place, over
    the finite pairs. Measured on the lists of tests/gomath_inputs.py
    (x86-64, gcc -O3 -ffp-contract=off):
        sin   1.478e-16  (bound 2^-52 = 2.220e-16)
        cos   1.502e-16  (bound 2^-52 = 2.220e-16)
        asin  4.420e-16  (bound 2^-51 = 4.441e-16)
        acos  6.491e-16  (bound 2^-50 = 8.882e-16)
        atan2 1.159 ulp  (bound 2 ulp)
    No relative bound for sin and cos: next to their zeros the reference
    algorithm itself is 12-15 ulp off (the three-part Pi/4 has 2^-100 or so of
    error, times y).
    """
    import mpmath
    mp = mpmath.mp.clone()
    mp.prec = 200
    reference_quirk = 0
    worst = {"sin": 0.0, "cos": 0.0, "asin": 0.0, "acos": 0.0, "atan2": 0.0}

    def err(got, exact):
        return float(abs(mp.mpf(got) - exact))

    for _, x in _flat(trig):
        if not math.isfinite(x) or abs(x) >= GI.P2_29:
            continue
        worst["sin"] = max(worst["sin"], err(lib.oracle_go_sin(x), mp.sin(mp.mpf(x))))
        worst["cos"] = max(worst["cos"], err(lib.oracle_go_cos(x), mp.cos(mp.mpf(x))))
    for _, x in _flat(asin):
        if not abs(x) <= 1:
            assert math.isnan(lib.oracle_go_asin(x)) and math.isnan(lib.oracle_go_acos(x)), x
            continue
        worst["asin"] = max(worst["asin"], err(lib.oracle_go_asin(x), mp.asin(mp.mpf(x))))
        worst["acos"] = max(worst["acos"], err(lib.oracle_go_acos(x), mp.acos(mp.mpf(x))))
    for _, (y, x) in _flat(atan2):
        if not (math.isfinite(y) and math.isfinite(x)) or y == 0 or x == 0:
            continue  # the special cases (mpmath has no signed zero): test_atan2_special_table_is_gos
        got = lib.oracle_go_atan2(y, x)
        if x < 0 and y != 0 and y / x == 0:
            # atan2.go itself: Atan(y/x) of a quotient that underflowed to +-0 has lost y's sign,
            # and q <= 0 takes q + Pi: +Pi whatever y's sign (the mathematical answer is -Pi for y < 0)
            assert GI.bits(got) == GI.bits(math.pi), (y, x, got)
            reference_quirk += 1
            continue
        worst["atan2"] = max(worst["atan2"], err(got, mp.atan2(mp.mpf(y), mp.mpf(x))) / math.ulp(got))
    print("oracle vs mpmath:", worst)
    assert reference_quirk > 0
    assert worst["sin"] <= SIN_BOUND, worst
    assert worst["cos"] <= COS_BOUND, worst
    assert worst["asin"] <= ASIN_BOUND, worst
    assert worst["acos"] <= ACOS_BOUND, worst
    assert worst["atan2"] <= ATAN2_BOUND_ULP, worst


def test_atan2_special_table_is_gos(lib, atan2):
    """atan2.go's special cases, written out: the 7 x 7 table over
    {NaN, -Inf, -1, -0, +0, 1, +Inf}."""
    pi = math.pi
    for y, x in atan2["special_table"]:
        got = lib.oracle_go_atan2(y, x)
        if y != y or x != x:
            assert got != got
            continue
        want = math.atan2(y, x)  # C99 Annex F lists the same table as atan2.go
        assert abs(got - want) <= 1e-15 and math.copysign(1.0, got) == math.copysign(1.0, want), (y, x, got, want)
        if y == 0:
            assert abs(got) in (0.0, pi)
        if math.isinf(y) and math.isinf(x):
            assert abs(got) in (pi / 4, 3 * pi / 4)
