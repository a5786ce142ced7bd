"""Input families for the Go-math checks -- test infrastructure.

The same families tests/hip/gomath_check.hip generates for the device (not the
same bits): arguments chosen for the branches of Go's sin.go, asin.go, atan.go
and atan2.go and of the amd64 float -> int conversion. A fixed seed: every
list is the same on every run, so a bound measured on it stays meaningful.
"""
import math
import random
import struct

INF, NAN = math.inf, math.nan
P2_29 = float(1 << 29)
P2_63 = float(1 << 63)
DEG_TO_RAD = 0.017453292519943295
TAN3PIO8 = 2.41421356237309504880
DENORMALS = (4.9e-324, 1e-310, 2.2250738585072009e-308)
ULP_OFFSETS = (0, 1, -1, 2, -2, 16, -16)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b & ((1 << 64) - 1)))[0]


def ulps(x, k):
    """x >= 0 moved by k units in the last place (through zero into the negatives)."""
    b = bits(x) + k
    return from_bits(b) if b >= 0 else -from_bits(-b)


def same(a, b):
    """Identical bits; any NaN equals any NaN."""
    return (a != a and b != b) or bits(a) == bits(b)


def _both(xs):
    return [s * x for x in xs for s in (1.0, -1.0)]


def trig(n=3000, seed=11):
    """{family: [x]} for sin / cos. Everything outside "threshold" is below 2^29."""
    rng = random.Random(seed)
    kmax = int(P2_29 * 1.2732395447351628)
    kpi4 = []
    for k in list(range(65)) + [kmax - i for i in range(16)]:
        c = k * (math.pi / 4)
        kpi4 += [ulps(c, o) for o in ULP_OFFSETS] + [c + 1e-9, c - 1e-9]
    return {
        "uniform": [rng.uniform(-8 * math.pi, 8 * math.pi) for _ in range(n)],
        "k_pi_4": _both(kpi4),
        "log_uniform": [rng.choice((1.0, -1.0)) * math.ldexp(rng.uniform(0.5, 1.0), rng.randrange(-1073, 30))
                        for _ in range(n)],
        "degrees": [(h * 0.5) * DEG_TO_RAD for h in range(-1440, 1441)],
        "specials": _both([0.0, INF, 2.2250738585072014e-308] + list(DENORMALS)) + [NAN],
        "threshold": _both([P2_29, ulps(P2_29, -1), P2_29 + 1.0, 1e300]),
    }


def octant(x):
    """The eighth of the circle sin.go's reduction first finds for a finite x."""
    return int(abs(x) * 1.2732395447351628) & 7


def asin(n=3000, seed=12):
    """{family: [x]} for asin / acos."""
    rng = random.Random(seed)
    ax = 0.66 / math.sqrt(1.0 + 0.66 * 0.66)  # ax / sqrt(1 - ax^2) crosses satan's 0.66 here
    return {
        "uniform": [rng.uniform(-1.0, 1.0) for _ in range(n)],
        "around_0.7": _both([ulps(0.7, k) for k in range(-16, 17)]),
        "around_satan_0.66": _both([ulps(ax, k) for k in range(-16, 17)]),
        "ends": _both([1.0, ulps(1.0, -1), ulps(1.0, -2), ulps(1.0, 1), 2.0, 0.0]),
        "specials": _both(list(DENORMALS) + [INF]) + [NAN],
    }


def atan2(n=3000, seed=13):
    """{family: [(y, x)]}."""
    rng = random.Random(seed)
    sgn = lambda: rng.choice((1.0, -1.0))
    mag = lambda lo, hi: math.ldexp(rng.uniform(0.5, 1.0), rng.randrange(lo, hi + 1))
    thresholds = []
    for i in range(n // 2):
        x = 1.0 + rng.random()
        q = TAN3PIO8 if i & 1 else 0.66
        thresholds.append((sgn() * ulps(x * q, rng.randrange(-4, 5)), sgn() * x))
    flows = []
    for _ in range(64):
        s, l = mag(-1000, -600), mag(600, 1000)
        flows += [(sgn() * s, sgn() * l), (sgn() * l, sgn() * s)]
    table = (NAN, -INF, -1.0, -0.0, 0.0, 1.0, INF)
    return {
        "log_uniform": [(sgn() * mag(-300, 300), sgn() * mag(-300, 300)) for _ in range(n)],
        "quotient_thresholds": thresholds,
        "quotient_underflow_overflow": flows,
        "special_table": [(y, x) for y in table for x in table],
    }


def f2i(n=3000, seed=14):
    """{family: [x]} for the float64 -> int64 / uint32 conversions."""
    rng = random.Random(seed)
    colour = []
    for k in range(257):
        for c0 in (k / 256.0, (k * 256) / 65535.0):
            colour += [ulps(c0, o) * 65535.0 for o in ULP_OFFSETS]
    return {
        "around_2^63": _both([P2_63, ulps(P2_63, -1), ulps(P2_63, -2), ulps(P2_63, 1), 9.3e18, 1e300]),
        "around_2^32_2^53": _both([4294967295.0, 4294967296.0, 4294967297.0, 4294967295.5, 9007199254740991.0,
                                   9007199254740992.0, 9007199254740994.0, 2147483648.0, 2147483647.5]),
        "specials": _both([0.0, 0.5, 1.5, 0.9999999999999999, 4.9e-324, INF]) + [NAN],
        "colour_channels": colour,
        "random_bits": [from_bits(rng.getrandbits(64)) for _ in range(n)],
    }
