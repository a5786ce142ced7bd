"""The query, radiance, render, camera and aov kernels where the FP64 tests
themselves err and where the BVH builder meets extreme layouts, against the
oracle (needs an MI355X): the families of tests/cull_limits.py -- ray origins
1e2 .. 1e12 units out, transforms of condition 1 .. 1e16, geometric arms,
coincident centroids, an enclosing sphere, the 11 / 12 / 13 object boundary,
and a frame whose ground is met 1e6 .. 3e7 units out.

Bar: every field of every record equals the oracle's under edge_rays.same()
(==, or both NaN: no tolerance anywhere), every occlusion byte equals the
oracle predicate, every frame equals the oracle's bytes and counters. What the
families contain is asserted from the oracle's side in
tests/test_cull_limits_ref.py. Rays go to the device in batches of at most
cull_limits.BATCH.
"""
import math

import numpy as np
import pytest

import go_raytracer_amd as rt
import aov_ref as AR
import camera_ref as CR
import cull_limits as CL
import edge_rays as E
import oracle_bind
import query_ref as Q
import trace_ref as T
from test_gpu_aov import assert_buffers_equal
from test_gpu_edge_rays import ACCEL, assert_miss_is_zero, mid_bound
from test_gpu_query import gpu_closest, gpu_occluded
from test_gpu_trace import gpu_radiance

abi = rt.abi
pytestmark = pytest.mark.gpu
INF = float("inf")
FAR_FORMS = ("linear", "bvh", "csg")
FORMS = ("linear", "bvh")
_want = {}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def spec_ctx():
    c = rt.RenderContext(0, specialize=True)
    yield c
    c.close()


def batched(fn, c, fam, tmax=None):
    """fn (gpu_closest, gpu_occluded) over `fam` in batches of CL.BATCH."""
    o, d, tm, ex = fam
    tm = tm if tmax is None else np.broadcast_to(np.asarray(tmax, dtype=np.float64), (len(o),))
    return np.concatenate([fn(c, o[a:a + CL.BATCH], d[a:a + CL.BATCH], tm[a:a + CL.BATCH], ex[a:a + CL.BATCH])
                           for a in range(0, len(o), CL.BATCH)])


def closest_of(key, Tb, fam):
    """The oracle's records of `fam`: shared, never modified."""
    if key not in _want:
        _want[key] = Tb.closest(fam[2], fam[3])
    return _want[key]


def check_queries(c, key, Tb, fam, bounds):
    """Closest records field by field and occlusion bytes at every bound against the oracle table."""
    got = batched(gpu_closest, c, fam)
    E.assert_same(got, closest_of(key, Tb, fam), str(key))
    assert_miss_is_zero(got)
    for label, b in bounds:
        occ = batched(gpu_occluded, c, fam, b)
        assert set(occ.tolist()) <= {0, 1}
        bad = np.flatnonzero(occ.astype(bool) != Tb.occluded(b, fam[3]))
        assert len(bad) == 0, "%s, occluded at %s: %d of %d differ, first ray %d" % (key, label, len(bad), len(occ), bad[0])


def set_scene(c, p, bvh, csg=False):
    c.set_scene(p)
    assert bool(c.scene_info() & abi.RT_INFO_BVH) == bvh and bool(c.scene_info() & abi.RT_INFO_CSG) == csg
    return p


def check_accel(p, fam, bound, want, what):
    """The four accel settings return identical bytes for `fam`, and those are the oracle's."""
    c = rt.RenderContext(0)
    try:
        res = []
        for flags in ACCEL:
            c.set_accel(flags)
            c.set_scene(p)
            if not flags & abi.RT_ACCEL_BVH:
                assert not c.scene_info() & abi.RT_INFO_BVH
            res.append((batched(gpu_closest, c, fam).tobytes(), batched(gpu_occluded, c, fam, bound).tobytes()))
        E.assert_same(np.frombuffer(res[0][0], dtype=abi.HIT_DTYPE), want, what + ", accel 0")
        for flags, r in zip(ACCEL[1:], res[1:]):
            E.assert_same(np.frombuffer(r[0], dtype=abi.HIT_DTYPE), want, "%s, accel %d" % (what, flags))
            assert r[0] == res[0][0] and r[1] == res[0][1], "%s: accel %d differs from accel 0" % (what, flags)
    finally:
        c.close()


def check_radiance(c, p, fam, what, depths=(1, 3)):
    o, d, tm, ex = fam
    for depth in depths:
        want = T.trace_many(p, o, d, depth, tm, ex)
        got = np.concatenate([gpu_radiance(c, o[a:a + CL.BATCH], d[a:a + CL.BATCH], depth, tm[a:a + CL.BATCH],
                                           ex[a:a + CL.BATCH]) for a in range(0, len(o), CL.BATCH)])
        E.assert_same(got, want, "%s depth %d" % (what, depth))


def check_render(c, p, what):
    ref, ost = oracle_bind.render_rows(p)
    c.set_scene(p)
    c.read_stats(reset=True)
    img = c.render()
    st = c.read_stats(reset=True)
    assert np.array_equal(img, ref), "%s: %d pixels differ" % (what, (img != ref).any(axis=2).sum())
    assert st.as_dict() == ost.as_dict(), what


# ---- far --------------------------------------------------------------------------
def far_table(form, D):
    return CL.table(("far", form, D), CL.far_scene(form), CL.far_rays(form, D))


@pytest.mark.parametrize("D", CL.FAR_D)
@pytest.mark.parametrize("form", FAR_FORMS)
def test_far_origins_equal_the_oracle(ctx, form, D):
    p = set_scene(ctx, CL.far_scene(form), form != "linear", form == "csg")
    fam, Tb = CL.far_rays(form, D), far_table(form, D)
    check_queries(ctx, ("far", form, D), Tb, fam, (("tmax inf", INF), ("just past the scene", CL.far_tmax(fam)),
                                                   ("a mid bound", mid_bound(Tb, fam))))


def far_mixed(form):
    """Every rung's rays in one stream, interleaved: near and far lanes share each wave."""
    fams = [CL.far_rays(form, D) for D in CL.FAR_D]
    want = np.concatenate([closest_of(("far", form, D), far_table(form, D), f) for D, f in zip(CL.FAR_D, fams)])
    fam, perm = E.interleave(fams, 23)
    past = np.concatenate([CL.far_tmax(f) for f in fams])[perm]
    return fam, want[perm], past


@pytest.mark.parametrize("form", FAR_FORMS)
def test_far_accel_settings_give_identical_bytes(form):
    fam, want, past = far_mixed(form)
    assert len(fam[0]) % CL.BATCH == 0 and len(fam[0]) >= 7 * CL.BATCH
    check_accel(CL.far_scene(form), fam, past, want, "far " + form)


@pytest.mark.parametrize("form", FAR_FORMS)
def test_far_radiance_equals_the_reference(ctx, form):
    p = set_scene(ctx, CL.far_scene(form), form != "linear", form == "csg")
    fam = E.concat([tuple(v[:CL.BATCH] for v in CL.far_rays(form, D)) for D in CL.FAR_D])
    check_radiance(ctx, p, fam, "far " + form)


def far_camera():
    """16 x 12, 2 samples, 1e7 units from the bvh form's middle (0, 0, 8), the view 26 units wide there."""
    u = np.array([0.3, 0.45, -0.84])
    eye = np.array([0.0, 0.0, 8.0]) + 1e7 * u / np.linalg.norm(u)
    fov = 2.0 * math.degrees(math.atan(2.0 / 2.6e-6))
    return rt.RenderContext.camera(samples=2, size=(16, 12), fov=fov, eye=tuple(eye), look_at=(0.0, 0.0, 8.0),
                                   up=(0.0, 1.0, 0.0))


def test_far_camera_equals_the_reference(ctx):
    p = set_scene(ctx, CL.far_scene("bvh"), True)
    cam = far_camera()
    rays = CR.rays(p, cam)
    assert rays.shape == (12, 16, 2)
    flat = rays.reshape(-1)
    assert (np.linalg.norm(flat["origin"] - np.array([0.0, 0.0, 8.0]), axis=1) > 0.99e7).all()
    rad = T.trace_many(p, flat["origin"], flat["dir"], 0).reshape(rays.shape)
    assert (rad["object"] >= 0).sum() >= 40 and len(set(rad["object"].reshape(-1).tolist())) >= 5  # the scene fills the frame
    img, mean = CR.resolve(rad)
    got, gmean = ctx.render_camera(cam, mean=True)
    same = (gmean == mean) | (np.isnan(gmean) & np.isnan(mean))
    assert same.all(), "%d means differ" % (~same).any(axis=2).sum()
    assert np.array_equal(got, img)
    assert_buffers_equal(ctx.render_camera_aov(cam), AR.buffers(p, cam), "far camera")


# ---- needle -----------------------------------------------------------------------
@pytest.mark.parametrize("k", CL.NEEDLE_K)
@pytest.mark.parametrize("form", FORMS)
def test_needles_equal_the_oracle(ctx, form, k):
    p = CL.needle_scene(form, k)
    ctx.set_scene(p)
    fam = CL.needle_rays(form, k)[0]
    Tb = CL.table(("needle", form, k), p, fam)
    mid = mid_bound(Tb, fam)
    check_queries(ctx, ("needle", form, k), Tb, fam, (("tmax inf", INF), ("a mid bound", mid)))


@pytest.mark.parametrize("k", [0, 5, 6, 7, 8, 12, 16])
@pytest.mark.parametrize("form", FORMS)
def test_needle_accel_settings_and_frames(ctx, spec_ctx, form, k):
    p = CL.needle_scene(form, k)
    fam = CL.needle_rays(form, k)[0]
    Tb = CL.table(("needle", form, k), p, fam)
    (o, d, tm, ex), perm = E.interleave([tuple(v[a:a + CL.BATCH // 2] for v in fam)
                                         for a in range(0, len(fam[0]), CL.BATCH // 2)], 3)
    check_accel(p, (o, d, tm, ex), mid_bound(Tb, fam)[perm], closest_of(("needle", form, k), Tb, fam)[perm],
                "needle %s %d" % (form, k))
    check_render(ctx, p, "needle %s %d" % (form, k))
    if k in (0, 8, 16):
        check_render(spec_ctx, p, "needle %s %d, specialised" % (form, k))


# needles as CSG leaves: the host's composite bound, leaf groups and their spheres with a never-culled leaf
@pytest.mark.parametrize("k", CL.NEEDLE_CSG_K)
def test_needle_leaves_equal_the_oracle(ctx, k):
    p = set_scene(ctx, CL.needle_scene("csg", k), True, True)
    fam = CL.needle_rays("csg", k)[0]
    Tb = CL.table(("needle", "csg", k), p, fam)
    mid = mid_bound(Tb, fam)
    check_queries(ctx, ("needle", "csg", k), Tb, fam, (("tmax inf", INF), ("a mid bound", mid)))
    check_accel(p, fam, mid, closest_of(("needle", "csg", k), Tb, fam), "needle csg %d" % k)
    check_radiance(ctx, p, tuple(v[:128] for v in fam), "needle csg %d" % k, depths=(3,))


# ---- layout -----------------------------------------------------------------------
@pytest.mark.parametrize("name", CL.LAYOUTS)
def test_layouts_equal_the_oracle(ctx, spec_ctx, name):
    p = set_scene(ctx, CL.layout_scene(name), CL.LAYOUT_BVH[name])
    fam = CL.layout_rays(name)
    Tb = CL.table(("layout", name), p, fam)
    mid = mid_bound(Tb, fam)
    check_queries(ctx, ("layout", name), Tb, fam, (("own tmax", fam[2]), ("a mid bound", mid)))
    (o, d, tm, ex), perm = E.interleave([tuple(v[a:a + CL.BATCH // 2] for v in fam) for a in (0, CL.BATCH // 2)], 9)
    check_accel(p, (o, d, tm, ex), mid[perm], closest_of(("layout", name), Tb, fam)[perm], "layout " + name)
    check_radiance(ctx, p, fam, "layout " + name)
    check_render(ctx, p, "layout " + name)
    check_render(spec_ctx, p, "layout %s, specialised" % name)


# ---- horizon ----------------------------------------------------------------------
def test_horizon_frame_and_its_shadow_rays(ctx, spec_ctx):
    p = set_scene(ctx, CL.horizon_scene(), True)
    fam, _ = CL.horizon_shadow_rays()
    Tb = CL.table(("horizon-shadow",), p, fam)
    check_queries(ctx, ("horizon-shadow",), Tb, fam, (("the light", fam[2]), ("tmax inf", INF)))
    check_accel(p, fam, fam[2], closest_of(("horizon-shadow",), Tb, fam), "horizon shadow rays")
    check_render(ctx, p, "horizon")
    check_render(spec_ctx, p, "horizon, specialised")
