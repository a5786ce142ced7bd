"""The references of the variance work (tests/variance_ref.py) against
independent statements of what they compute. CPU-only: nothing here touches
the library's device side.

Negative estimates: on the c3 frames tests/test_gpu_variance.py renders (the
zero camera at 13 x 23 with 4 samples; the thin lens at 24 x 16) no S among 3,
5, 6, 7 produces a negative e_c -- every equal-sample pixel of those frames
gives exactly 0.0 (test_no_negative_estimate_on_the_c3_frames pins this) -- so
the thin-lens case there uses S = 7, odd and no power of two, and the clamp is
shown on synthetic pixels instead (test_equal_samples_give_zero).
"""
import numpy as np
import pytest

import go_raytracer_amd as rt
import adaptive_ref as AR
import denoise_ref as DR
import variance_ref as VR

INF = float("inf")


def records(colors):
    """[rows, W, S, 3] colours as radiance records [rows, W, S]."""
    colors = np.asarray(colors, dtype=np.float64)
    rad = np.zeros(colors.shape[:3], dtype=rt.abi.RADIANCE_DTYPE)
    rad["color"] = colors
    return rad


@pytest.mark.parametrize("S", [2, 4, 7, 16])
def test_resolve_var_is_the_sample_variance_over_n(S):
    rng = np.random.RandomState(S)
    col = rng.uniform(0.0, 1.5, (5, 7, S, 3))
    got = VR.resolve_var(records(col))
    want = col.var(axis=2, ddof=1) / S
    big = want > 1e-12
    assert big.sum() > 90
    assert np.all(np.abs(got[big] - want[big]) <= 1e-9 * want[big])


def test_resolve_var_at_per_pixel_counts():
    rng = np.random.RandomState(5)
    col = rng.uniform(0.0, 1.5, (4, 6, 16, 3))
    counts = rng.choice([2, 4, 8, 16], size=(4, 6)).astype(np.int32)
    assert len(np.unique(counts)) == 4
    got = VR.resolve_var(records(col), counts)
    for y in range(4):
        for x in range(6):
            n = counts[y, x]
            want = col[y, x, :n].var(axis=0, ddof=1) / n
            assert np.all(np.abs(got[y, x] - want) <= 1e-9 * want)
            assert np.array_equal(got[y, x], VR.resolve_var(records(col[y:y + 1, x:x + 1, :n]))[0, 0])


def test_equal_samples_give_zero():
    """n equal samples c: Q and Sum * m both round n * c * c, so e_c is 0 or a
    rounding residue. Where n = 2, or every sum and product is exact (dyadic
    c), it is exactly 0; a negative residue is clamped to exactly 0. The rule does
    leave a positive residue at some (n, c), (3, 0.3) for one: each of Sum, m,
    Sum * m and Q is off by at most n roundings of n * c * c, so
    |e_c| <= 8 * 2^-53 * c * c, twenty orders below any sampled variance."""
    neg = pos = 0
    for n in (2, 3, 4, 5, 6, 7, 8):
        for c in (0.0, 0.1, 0.25, 0.3, 0.6, 0.7, 1.0):
            var, est = VR.pixel_var([(c, c, c)] * n)
            assert all(abs(e) <= 8.0 * 2.0 ** -53 * c * c for e in est)
            assert var == [0.0 if e < 0.0 else e for e in est]
            if n == 2 or c in (0.0, 0.25, 1.0):
                assert est == [0.0, 0.0, 0.0]
            neg += est[0] < 0.0
            pos += est[0] > 0.0
    assert neg >= 3 and pos >= 1  # (5, 0.3), (6, 0.7), (7, 0.6) clamp; (3, 0.3) does not
    assert VR.pixel_var([(0.3, 0.6, 0.7)] * 5) == ([0.0, 0.0, 0.0], [-5.551115123125783e-18, -2.2204460492503132e-17,
                                                                     -2.2204460492503132e-17])
    nan = VR.pixel_var([(float("nan"), 0.5, 0.5), (0.25, 0.5, 0.5)])[0]
    assert nan[0] != nan[0] and nan[1:] == [0.0, 0.0]  # a NaN stays NaN


def test_no_negative_estimate_on_the_c3_frames():
    cams = [rt.RenderContext.camera(samples=4, size=(13, 23))]
    cams += [rt.RenderContext.camera(model="thinlens", samples=S, size=(24, 16), aperture=0.35, focus=4.5,
                                     chunk_pixels=100) for S in (3, 5, 6, 7)]
    for cam in cams:
        rad = AR.radiance("c3", cam)
        est = VR.resolve_var(rad, estimates=True)
        var = VR.resolve_var(rad)
        assert (var == 0.0).any() and (var > 0.0).any()
        assert not (est < 0.0).any()  # (see the module docstring)
        assert np.array_equal(est, var)


def flat(H, W, value):
    return np.full((H, W, 3), value, dtype=np.float64)


def test_constant_variance_with_every_term_off():
    H, W = 9, 11
    color = np.random.RandomState(1).uniform(0.0, 1.0, (H, W, 3))
    var = flat(H, W, 0.125 / 4.0)
    var[..., 2] = 0.0625  # S_0 = (1/32 + 1/32) + 1/16 = 1/8
    out, s1 = VR.atrous_var(color, var, iterations=1)
    s0 = 0.125
    assert s1[4, 5] == s0 * 4900.0 / 65536.0  # interior: sum of h^2 is (70/256)^2, exact in binary
    assert s1[2, 2] == s1[4, 5] and s1[0, 0] > s1[4, 5]  # fewer taps at the border: less averaging
    assert np.array_equal(out, DR.atrous(color, iterations=1))  # the colour is the plain filter's with all terms off


def test_zero_variance_with_distinct_colours_is_the_identity():
    H, W = 8, 10
    # distinct colours on a dyadic grid: w * c and (w * c) / w are exact for the centre tap
    color = (np.arange(H * W * 3, dtype=np.float64).reshape(H, W, 3) + 1.0) / 1024.0
    out, sk = VR.atrous_var(color, flat(H, W, 0.0), iterations=5, sigma_color=4.0)
    assert np.array_equal(out, color)
    assert (sk == 0.0).all()


def test_nan_and_inf_variance_pixels():
    H, W = 9, 9
    rng = np.random.RandomState(2)
    color = 0.5 + rng.normal(0.0, 0.02, (H, W, 3))
    var = flat(H, W, 4e-4)
    var[2, 2] = np.nan
    var[6, 6, 1] = INF
    out, s1 = VR.atrous_var(color, var, iterations=1, sigma_color=4.0)
    # a NaN g shuts every tap: the 3 x 3 around the NaN passes through, colour and variance
    for y in range(1, 4):
        for x in range(1, 4):
            assert np.array_equal(out[y, x], color[y, x])
            assert s1[y, x] == (var[y, x, 0] + var[y, x, 1]) + var[y, x, 2] or (y, x) == (2, 2)
    assert s1[2, 2] != s1[2, 2]
    # ... and a pixel further off that taps the NaN pixel carries it in its variance only
    assert s1[2, 4] != s1[2, 4] and np.isfinite(out[2, 4]).all() and not np.array_equal(out[2, 4], color[2, 4])
    # +inf opens the colour term fully: the pixel is the plain filter's with every term off
    plain = DR.atrous(color, iterations=1)
    for y in range(5, 8):
        for x in range(5, 8):
            assert np.array_equal(out[y, x], plain[y, x])
            assert s1[y, x] == INF
    assert np.isfinite(out).all()
    # with the colour term off no g is formed and the variance still propagates
    out0, s0 = VR.atrous_var(color, var, iterations=1)
    assert np.array_equal(out0, plain) and 0.0 < s0[0, 8] < 3.0 * 4e-4
    assert s0[2, 2] != s0[2, 2] and s0[6, 6] == INF


def test_guided_filter_beats_the_raw_mean_on_a_heteroscedastic_frame():
    """VR.hetero_frame(64, 48): a smooth ramp, 4 samples per pixel, per-sample
    noise of sigma 0.25 in the middle third of the rows and 0.01 elsewhere;
    5 iterations at 4 standard deviations, no guides."""
    clean, mean, var = VR.hetero_frame(64, 48)
    out, sk = VR.atrous_var(mean, var, iterations=5, sigma_color=4.0)
    raw = float(((mean - clean) ** 2).mean())
    got = float(((out - clean) ** 2).mean())
    print("raw MSE %.3e, variance-guided MSE %.3e" % (raw, got))
    assert got < raw
    assert (sk >= 0.0).all() and sk.mean() < ((var[..., 0] + var[..., 1]) + var[..., 2]).mean()
