"""tests/adaptive_ref.py against camera_ref and recorded histograms (CPU-only):
at min_samples = S it is the fixed render's resolve, at an infinite tolerance
every pixel stops at min_samples, and on the GPU tests' own 13 x 23 frames it
spreads the pixels over the pass levels as recorded. This pins the reference
the adaptive-render tests compare the device with."""
import math

import numpy as np
import pytest

import go_raytracer_amd as rt
import adaptive_ref as AR
import camera_ref as CR

W, H = 13, 23
HISTOGRAMS = AR.HISTOGRAMS


def cam13(S):
    return rt.RenderContext.camera(samples=S, size=(W, H))


def test_schedule():
    assert AR.schedule(16, 2) == [2, 4, 8, 16]
    assert AR.schedule(20, 3) == [3, 6, 12, 20]
    assert AR.schedule(1024, 2) == [2 << k for k in range(10)]
    assert AR.schedule(64) == [4, 8, 16, 32, 64] and AR.schedule(3) == [3] and AR.schedule(2) == [2]
    assert AR.schedule(12, 12) == [12]


def test_min_samples_at_the_cap_is_the_fixed_resolve():
    rad = AR.radiance("c3", cam13(16))
    assert rad.shape == (H, W, 16)
    img, mean, count = AR.resolve(rad, 0.005, 16)
    wimg, wmean = CR.resolve(rad)
    assert np.array_equal(img, wimg) and np.array_equal(mean, wmean) and (count == 16).all()
    assert len(np.unique(wimg.reshape(-1, 4), axis=0)) >= 20
    # a pixel that runs to the cap under a finite tolerance is the fixed render's pixel too
    img, mean, count = AR.resolve(rad, 0.005, 2)
    cap = count == 16
    assert cap.sum() >= 3 and np.array_equal(img[cap], wimg[cap]) and np.array_equal(mean[cap], wmean[cap])
    assert not np.array_equal(mean[~cap], wmean[~cap])


def test_infinite_tolerance_stops_every_pixel_at_min_samples():
    rad = AR.radiance("c3", cam13(16))
    for n0 in (2, 5):
        img, mean, count = AR.resolve(rad, math.inf, n0)
        assert (count == n0).all()
        wimg, wmean = CR.resolve(rad[:, :, :n0])
        assert np.array_equal(mean, wmean) and np.array_equal(img, wimg)
    assert (AR.resolve(rad, math.inf)[2] == 4).all()  # min_samples 0: min(4, S)


def test_nan_never_converges_and_a_negative_variance_does():
    assert not AR.converged([math.nan, 0.0, 0.0], [math.nan, 0.0, 0.0], 2, math.inf)
    assert AR.converged([1.0, 1.0, 1.0], [0.4, 0.5, 0.5], 2, 0.0)  # v = 0.4 - 0.5 < 0 passes, v = 0 passes
    assert not AR.converged([1.0, 1.0, 1.0], [0.5, 0.5, 0.6], 2, 0.0)


@pytest.mark.parametrize("case", list(HISTOGRAMS), ids=lambda c: "%s-%d-%d" % c[:3])
def test_recorded_histograms(case):
    name, S, n0, tol = case
    _, _, count = AR.resolve(AR.radiance(name, cam13(S)), tol, n0)
    assert AR.histogram(count) == HISTOGRAMS[case]
