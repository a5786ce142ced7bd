"""tests/aov_ref.py, the feature buffers' reference, on its own (CPU-only): the
cases the device tests rely on exist in it, a pixel no sample hits reads as the
header says, and at one sample the buffers are query_ref's closest record of
the one ray. Frames are 13 x 23 at 7 samples: (scene, camera model) pairs are
shared with tests/test_gpu_aov.py through aov_ref.reference."""
import numpy as np
import pytest

import go_raytracer_amd as rt
import aov_ref as AR
import camera_ref as CR
import query_ref
import trace_ref as T

abi = rt.abi
W, H, S = 13, 23, 7
SCENES = ["c3", "c4", "c4csg", "closure"]
MODELS = {  # tests/test_gpu_camera.py MODELS
    "pinhole": dict(model="pinhole"),
    "ortho": dict(model="ortho", extent=6.5),
    "equirect": dict(model="equirect"),
    "thinlens": dict(model="thinlens", aperture=0.35, focus=4.5),
}


def camera(model, samples=S):
    return rt.RenderContext.camera(samples=samples, size=(W, H), **MODELS[model])


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("name", SCENES)
def test_every_pair_has_empty_partial_and_full_pixels(name, model):
    ref = AR.reference(name, T.packed(name), camera(model))
    cov = ref["coverage"]
    assert (cov == 0.0).any() and (cov == 1.0).any()
    partial = (cov > 0.0) & (cov < 1.0)
    assert partial.sum() >= 2, partial.sum()
    if name == "closure":
        assert ref["closure"] >= 17, ref["closure"]
    # a pixel no sample hits: depth +inf, zero normal and albedo, ids (-1, 0, 0, 0)
    empty = cov == 0.0
    assert np.isposinf(ref["depth"][empty]).all()
    assert (ref["normal"][empty] == 0.0).all() and (ref["albedo"][empty] == 0.0).all()
    ids = ref["ids"][empty]
    assert (ids["object"] == -1).all() and (ids["face"] == 0).all() and (ids["kind"] == 0).all() \
        and (ids["material"] == 0).all()
    # ... and elsewhere: finite depth, coverage a multiple of 1 / S formed as h * inv
    assert np.isfinite(ref["depth"][~empty]).all()
    inv = 1.0 / float(S)
    assert set(np.unique(cov)) <= {float(h) * inv for h in range(S + 1)}


@pytest.mark.parametrize("name", ["c3", "c4csg"])
def test_one_sample_equals_the_closest_record_of_the_one_ray(name):
    p = T.packed(name)
    cam = camera("pinhole", samples=1)
    ref = AR.buffers(p, cam)
    rays = CR.rays(p, cam).reshape(-1)
    hits = query_ref.Table(p, rays["origin"], rays["dir"]).closest().reshape(H, W)
    hit = hits["object"] >= 0
    assert hit.any() and (~hit).any()
    assert np.array_equal(ref["coverage"], hit.astype(np.float64))
    assert np.array_equal(ref["depth"][hit], hits["t"][hit]) and np.isposinf(ref["depth"][~hit]).all()
    for k in abi.AOV_IDS_DTYPE.names:
        assert np.array_equal(ref["ids"][k], hits[k]), k  # (a miss record is -1, 0, 0, 0 as well)
    sc = p.scene
    for y in range(H):
        for x in range(W):
            if not hit[y, x]:
                continue
            n = T.v_norm(tuple(float(v) for v in hits[y, x]["normal_world"]))
            assert AR.same(ref["normal"][y, x], np.array(n))
            m = int(hits[y, x]["material"])
            assert m >= 0
            assert tuple(ref["albedo"][y, x]) == tuple(sc.materials[m].color[:])
