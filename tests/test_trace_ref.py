"""tests/trace_ref.py against the oracle itself (CPU-only): averaging and
quantising trace() over camera_rays() reproduces oracle_render_rows byte for
byte, and the rays it traces are the oracle's primary + secondary rays. This
pins the reference the radiance-query tests compare the device with."""
import numpy as np
import pytest

import oracle_bind
import trace_ref as T


@pytest.mark.parametrize("name", ["c2", "c3", "c3cone", "canned", "c4csg", "closure"])
def test_trace_over_camera_rays_reproduces_the_oracle_render(name):
    p = T.packed(name)
    if name == "closure":
        assert p.scene.num_programs >= 1
    ref, st = oracle_bind.render_rows(p)
    img, rays, rad = T.render(p)
    assert np.array_equal(img, ref), "%d of %d pixels differ" % ((img != ref).any(axis=2).sum(), ref.shape[0] * ref.shape[1])
    assert rays == int(st.primary_rays) + int(st.secondary_rays)
    assert st.surface_errors == 0
    assert bool((rad["rays"] > 1).any()) == (st.secondary_rays > 0)
    if name in ("c3", "c3cone", "canned", "c4csg"):
        assert st.secondary_rays > 0
    assert (rad["object"] < 0).any() and (rad["object"] >= 0).any()


def test_camera_rays_of_a_band_equal_the_full_frame_rows():
    p = T.packed("c2")
    full = T.camera_rays(p, 0, 16)
    assert full.shape == (16, 24, 4)
    assert T.camera_rays(p, 5, 11).tobytes() == full[5:11].tobytes()
    assert (full["tmax"] == np.inf).all() and (full["exclude"] == -1).all() and (full["reserved"] == 0).all()
