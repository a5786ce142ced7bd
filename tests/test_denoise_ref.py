"""tests/denoise_ref.py, the a-trous filter's reference, on its own (CPU-only):
the properties of the header's rule that make it an edge-avoiding filter."""
import numpy as np
import pytest

import denoise_ref as DR

W, H = 37, 29
ALL = dict(sigma_color=0.6, sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.25)


@pytest.fixture(scope="module")
def frame():
    return DR.test_frame(W, H)


def test_the_guided_filter_removes_noise(frame):
    """Gaussian noise, sigma 0.15, on piecewise-constant surfaces, the three
    guide terms on. One interior B3 pass alone divides the variance by
    1 / (sum h^2)^2 = 13.4; the bound of 20 therefore needs the later, wider
    iterations to work too, and the guides to keep the three regions apart
    (mixing them costs about 0.1 per channel at every edge pixel)."""
    clean, noisy, normal, depth, albedo = frame
    out = DR.atrous(noisy, normal, depth, albedo, 5, sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.25)
    before = float(((noisy - clean) ** 2).mean())
    after = float(((out - clean) ** 2).mean())
    assert np.isfinite(out).all()
    assert 1.5e-2 < before < 3e-2 and after < before / 20.0, (before, after)
    # the colour term keeps detail instead: it still helps, less
    mid = float(((DR.atrous(noisy, normal, depth, albedo, 5, **ALL) - clean) ** 2).mean())
    assert after < mid < before, (before, mid, after)


@pytest.mark.parametrize("term", ["sigma_normal", "sigma_depth", "sigma_albedo"])
def test_guides_stop_colour_crossing_a_discontinuity(frame, term):
    """With the colour term off, the outputs left of the wall / floor edge (and
    below the background) are bit-identical when the colours right of it are
    replaced: no tap crosses a guide discontinuity of the one term that is on."""
    _, noisy, normal, depth, albedo = frame
    top = max(1, H // 5)
    left = np.zeros((H, W), dtype=bool)
    left[top:, :W // 2] = True
    other = noisy.copy()
    other[~left] = other[~left] * -3.0 + 7.0
    # the one term that is on separates the regions: its weight is 0 across the edge
    sig = {term: {"sigma_normal": 0.5, "sigma_depth": 1.0, "sigma_albedo": 0.25}[term]}
    a = DR.atrous(noisy, normal, depth, albedo, 3, **sig)
    b = DR.atrous(other, normal, depth, albedo, 3, **sig)
    assert a[left].tobytes() == b[left].tobytes()
    assert a[~left].tobytes() != b[~left].tobytes()
    # without any guide the replaced colours do reach the left side
    c = DR.atrous(noisy, iterations=3)
    d = DR.atrous(other, iterations=3)
    assert c[left].tobytes() != d[left].tobytes()


def test_a_nan_pixel_stays_nan_and_spreads_nowhere_with_the_colour_term_on(frame):
    _, noisy, normal, depth, albedo = frame
    bad = noisy.copy()
    bad[11, 17] = np.nan
    for kw in (dict(sigma_color=0.6), ALL):
        out = DR.atrous(bad, normal, depth, albedo, 4, **kw)
        nan = np.isnan(out)
        assert nan[11, 17].all()
        nan[11, 17] = False
        assert not nan.any()
    # (with the colour term off the NaN does spread: the term is what stops it)
    assert np.isnan(DR.atrous(bad, iterations=2)).sum() > 3


def test_eight_iterations_on_a_small_frame_are_finite(frame):
    _, noisy, normal, depth, albedo = frame
    out = DR.atrous(noisy, normal, depth, albedo, 8, **ALL)  # the last step, 128, exceeds the frame
    assert out.shape == (H, W, 3) and np.isfinite(out).all()


def test_all_terms_off_is_the_b3_filter_renormalised_at_the_borders():
    rng = np.random.RandomState(5)
    img = rng.rand(9, 11, 3)
    out = DR.atrous(img, iterations=1)
    h = np.array(DR.TAPS)
    k = np.outer(h, h)
    for y in range(9):
        for x in range(11):
            acc, ws = np.zeros(3), 0.0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if 0 <= y + dy < 9 and 0 <= x + dx < 11:
                        acc += k[dy + 2, dx + 2] * img[y + dy, x + dx]
                        ws += k[dy + 2, dx + 2]
            assert np.allclose(out[y, x], acc / ws, rtol=1e-14, atol=0.0)
    # an interior pixel's weights add up to exactly 1; a constant frame is a fixed point everywhere
    flat = np.full((9, 11, 3), 0.625)
    assert (DR.atrous(flat, iterations=3) == 0.625).all()
    # off means off: 0 and +inf sigmas give the same bits, negative and NaN are invalid
    assert DR.atrous(img, iterations=1, sigma_color=float("inf"), sigma_depth=0.0).tobytes() == out.tobytes()
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            DR.atrous(img, iterations=1, sigma_normal=bad)
