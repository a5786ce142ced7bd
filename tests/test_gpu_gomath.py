"""Device Go-math restatements vs the oracle's, bit for bit (needs an MI355X).

tests/hip/gomath_check runs rt_device.h go_sin / go_cos / go_asin / go_acos /
go_atan2 / go_f2i / go_f64_to_u32 in one kernel over fixed-seed input
families (DESIGN "Go math on the device") and compares on the host with
oracle/go_math.h. tests/test_gomath_ref.py holds the oracle itself to mpmath.
"""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

FUNCTIONS = ("sin", "cos", "asin", "acos", "atan2", "f2i", "f64_to_u32")
FAMILIES = {
    "trig": ("uniform", "k_pi_4", "log_uniform", "degrees", "specials", "threshold"),
    "asin": ("uniform", "around_0.7", "around_satan_0.66", "ends", "specials"),
    "atan2": ("log_uniform", "quotient_thresholds", "quotient_underflow_overflow", "special_table"),
    "f2i": ("around_2^63", "around_2^32_2^53", "specials", "colour_channels", "random_bits"),
}


def test_device_trig_and_conversions_equal_oracle_restatement():
    """About 2^20 cases per function: identical bits (any NaN equals any NaN,
    signed zeros must match), NaN for every finite |x| >= 2^29 of sin / cos,
    acos(-0) == Pi/2; every input family, all eight octants of the sin / cos
    reduction, both sides of asin's 0.7, every branch of satan and both
    degenerate quotients of atan2 are reached."""
    exe = os.path.join(os.path.dirname(__file__), "hip", "gomath_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    n = 1 << 20
    r = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert stats["mismatches"] == {f: 0 for f in FUNCTIONS}, (stats, r.stderr)
    for what, cases in stats["cases"].items():
        assert cases >= n, stats
    for what, names in FAMILIES.items():
        assert tuple(stats["families"][what]) == names, stats["families"]
        assert all(stats["families"][what][k] > 0 for k in names), stats["families"]
    assert stats["families"]["atan2"]["special_table"] == 49
    assert stats["families"]["trig"]["degrees"] == 2881
    assert len(stats["octants"]) == 8 and all(c > 0 for c in stats["octants"]), stats
    assert stats["beyond_2^29"] >= 6 and stats["beyond_2^29_not_nan"] == 0, stats
    assert stats["acos_neg_zero_is_half_pi"] == 1, stats
    for key in ("asin_above_0.7", "asin_below_0.7", "asin_satan_low", "asin_satan_mid", "atan2_q_low", "atan2_q_mid",
                "atan2_q_high", "atan2_q_zero", "atan2_q_inf", "f2i_min_int64"):
        assert stats[key] > 0, (key, stats)
