"""Batched ray queries (rt_query_closest_async / rt_query_occluded_async) on the
device against the oracle loop of tests/query_ref.py (needs an MI355X).

Bar: every field of every hit record equals the oracle's value (==, no
tolerance: the render path is byte-exact through these same values), every
occlusion byte equals the oracle predicate. Each test first asserts, from the
oracle's side alone, that its inputs still cover what it is about (ties,
misses, distinct winners, shadowed and lit rays, rays that depend on
`exclude`).
"""
import ctypes as C

import numpy as np
import pytest

import go_raytracer_amd as rt
import oracle_bind
import query_ref as Q

abi = rt.abi
pytestmark = pytest.mark.gpu

N = 1024
ALL_SCENES = ["mixed11", "mixed12", "c3cone", "c4csg"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


def ray_records(origins, dirs, tmax=None, exclude=None):
    n = len(origins)
    rec = np.zeros(n, dtype=abi.RAY_DTYPE)
    rec["origin"] = origins
    rec["dir"] = dirs
    rec["tmax"] = np.inf if tmax is None else tmax
    rec["exclude"] = -1 if exclude is None else exclude
    return rec


def upload(rec):
    import torch
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")


def gpu_closest(ctx, origins, dirs, tmax=None, exclude=None, stream=None):
    import torch
    rays = upload(ray_records(origins, dirs, tmax, exclude))
    hits = torch.empty(len(origins) * abi.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    ctx.query_closest_async(rays, hits, stream)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(abi.HIT_DTYPE)


def gpu_occluded(ctx, origins, dirs, tmax=None, exclude=None, stream=None):
    import torch
    rays = upload(ray_records(origins, dirs, tmax, exclude))
    out = torch.empty(len(origins), dtype=torch.uint8, device="cuda:0")
    ctx.query_occluded_async(rays, out, stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_hits_equal(got, want, what):
    bad = Q.fields_equal(got, want)
    if bad:
        k = bad[0]
        rows = np.argwhere(np.asarray(got[k] != want[k]).reshape(len(got), -1).any(axis=1)).ravel()
        r = int(rows[0])
        raise AssertionError("%s: fields %s differ in %d records; first ray %d: gpu %s oracle %s"
                             % (what, bad, len(rows), r, got[r], want[r]))


def assert_surface_fields(p, hits):
    """kind and material of every hit against the packed scene's arrays."""
    for h in hits[hits["object"] >= 0]:
        o = p.scene.objects[int(h["object"])]
        face = int(h["face"])
        if o.kind == abi.RT_CSG:
            o = p.scene.csg_leaves[o.csg_first + (face >> 4)]
            face &= 7
        assert h["kind"] == o.kind and h["material"] == o.material[face], h


# 1. closest hits equal the oracle in every field
@pytest.mark.parametrize("name", ALL_SCENES)
def test_closest_hits_equal_the_oracle(ctx, name):
    T = Q.table(name)
    want = T.closest()
    win = want["object"]
    assert (win < 0).sum() >= 50
    if name.startswith("mixed"):
        assert T.tied_winners().sum() >= 20
        assert len(set(win[win >= 0])) >= (30 if name == "mixed12" else 8)
        assert set(want["face"][win >= 0]) == {0, 1, 2, 3, 4, 5}
    if name == "c4csg":  # composite hits: leaf numbers and flipped normals in the face code
        comp = want["face"][win >= 0]
        assert (comp >> 4).max() > 0 and ((comp >> 3) & 1).any()
    p = ctx.set_scene(Q.packed(name))
    bvh = bool(ctx.scene_info() & abi.RT_INFO_BVH)
    assert bvh == (name == "mixed12")
    got = gpu_closest(ctx, T.origins, T.dirs)
    assert_hits_equal(got, want, name)
    assert_surface_fields(p, got)
    miss = got[got["object"] < 0]
    assert not miss.view(np.uint8).reshape(len(miss), -1)[:, :80].any()  # a miss: zero in every other field


# 2. far origins (far_shift of the BVH culls)
def test_far_origins_equal_the_oracle(ctx):
    o, d = Q.rays(N, 5)
    o, d = o[:128], d[:128]
    dist = np.logspace(3, 5, 128)
    o = o - d * (dist / np.linalg.norm(d, axis=1))[:, None]
    T = Q.Table(Q.packed("mixed12"), o, d)
    want = T.closest()
    assert (want["object"] >= 0).sum() >= 50
    ctx.set_scene(Q.packed("mixed12"))
    assert ctx.scene_info() & abi.RT_INFO_BVH
    assert_hits_equal(gpu_closest(ctx, o, d), want, "far origins")
    # from that far every ray first meets one of the two planes; with that one
    # left out the winners are spread over the BVH's objects
    ex = want["object"].astype(np.int32)
    behind = T.closest(exclude=ex)
    assert len(set(behind["object"])) >= 10
    assert_hits_equal(gpu_closest(ctx, o, d, exclude=ex), behind, "far origins, first plane excluded")
    tm = behind["t"] * np.where(np.arange(128) % 2 == 0, 0.999, 1.001)  # just short of / just past the hit
    occ = T.occluded(tmax=tm, exclude=ex)
    assert occ.sum() >= 20 and (~occ).sum() >= 20
    assert np.array_equal(gpu_occluded(ctx, o, d, tmax=tm, exclude=ex).astype(bool), occ)


# 3. all four accel settings return identical records
@pytest.mark.parametrize("name", ["mixed12", "c4csg"])
def test_accel_settings_give_identical_bytes(name):
    T = Q.table(name)
    c = rt.RenderContext(0)
    try:
        res = []
        for flags in (0, abi.RT_ACCEL_CULL, abi.RT_ACCEL_BVH, abi.RT_ACCEL_BVH | abi.RT_ACCEL_CULL):
            c.set_accel(flags)
            c.set_scene(Q.packed(name))
            bvh = bool(c.scene_info() & abi.RT_INFO_BVH)
            assert bvh == (name == "mixed12" and bool(flags & abi.RT_ACCEL_BVH))
            res.append((gpu_closest(c, T.origins, T.dirs).tobytes(), gpu_occluded(c, T.origins, T.dirs, tmax=1.0).tobytes()))
        for r in res[1:]:
            assert r[0] == res[0][0] and r[1] == res[0][1]
        assert_hits_equal(np.frombuffer(res[0][0], dtype=abi.HIT_DTYPE), T.closest(), name)
    finally:
        c.close()


# 4. tmax and exclude in closest mode
@pytest.mark.parametrize("name", ["mixed11", "mixed12", "c4csg"])
def test_closest_with_exclude_and_tmax(ctx, name):
    T = Q.table(name)
    first = T.closest()
    hit = first["object"] >= 0
    assert hit.sum() >= 500
    ctx.set_scene(Q.packed(name))
    ex = first["object"].astype(np.int32)  # (-1 for a miss: none)
    want = T.closest(exclude=ex)
    assert (want["object"][hit] != first["object"][hit]).all()
    assert (want["object"][hit] >= 0).sum() >= 100  # something lies behind the winner
    assert_hits_equal(gpu_closest(ctx, T.origins, T.dirs, exclude=ex), want, name + " exclude")
    tm = np.where(hit, first["t"], np.inf)
    want = T.closest(tmax=tm)
    got = gpu_closest(ctx, T.origins, T.dirs, tmax=tm)
    # the winner and its exact duplicates are gone: nothing lies before the closest hit
    assert (want["object"] == -1).all()
    assert_hits_equal(got, want, name + " tmax")
    # (and the bound is strict: one ulp further the winner is back)
    tm = np.where(hit, np.nextafter(first["t"], np.inf), np.inf)
    assert_hits_equal(gpu_closest(ctx, T.origins, T.dirs, tmax=tm), first, name + " tmax + 1 ulp")


# 5. occluded mode equals the oracle predicate
@pytest.mark.parametrize("name", ALL_SCENES)
def test_occluded_equals_the_oracle_predicate(ctx, name):
    T = Q.table(name)
    want = T.occluded(tmax=1.0)
    assert want.sum() >= 20 and (~want).sum() >= 20
    so, sd, sex = Q.shadow_rays(name)
    TS = Q.table(name, "shadow")
    shadowed, plain = TS.occluded(1.0, sex), TS.occluded(1.0, None)
    assert shadowed.sum() >= 20 and (~shadowed).sum() >= 20
    assert (shadowed != plain).sum() >= 5
    ctx.set_scene(Q.packed(name))
    assert np.array_equal(gpu_occluded(ctx, T.origins, T.dirs, tmax=1.0).astype(bool), want)
    got = gpu_occluded(ctx, so, sd, tmax=1.0, exclude=sex)
    assert set(got.tolist()) <= {0, 1}
    assert np.array_equal(got.astype(bool), shadowed)
    assert np.array_equal(gpu_occluded(ctx, so, sd, tmax=1.0).astype(bool), plain)


# 6. batch edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_batch_sizes_and_untouched_tail(ctx, n):
    import torch
    T = Q.table("c3cone")
    ctx.set_scene(Q.packed("c3cone"))
    rays = upload(ray_records(T.origins, T.dirs, tmax=5.0))
    hb = abi.HIT_DTYPE.itemsize
    full_h = torch.empty(N * hb, dtype=torch.uint8, device="cuda:0")
    full_o = torch.empty(N, dtype=torch.uint8, device="cuda:0")
    ctx.query_closest_async(rays, full_h)
    ctx.query_occluded_async(rays, full_o)
    hits = torch.full((N * hb,), 0xA5, dtype=torch.uint8, device="cuda:0")
    occ = torch.full((N,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ctx.query_closest_async(rays[:n * 64], hits[:n * hb])
    ctx.query_occluded_async(rays[:n * 64], occ[:n])
    torch.cuda.synchronize()
    full_h, full_o, hits, occ = (t.cpu().numpy() for t in (full_h, full_o, hits, occ))
    assert_hits_equal(full_h.view(abi.HIT_DTYPE), T.closest(tmax=5.0), "c3cone tmax 5")
    assert np.array_equal(hits[:n * hb], full_h[:n * hb]) and (hits[n * hb:] == 0xA5).all()
    assert np.array_equal(occ[:n], full_o[:n]) and (occ[n:] == 0xA5).all()


# 7. no side effects on renders and their counters
def test_queries_leave_renders_and_counters_alone():
    import torch
    p = rt.scene.convert(rt.configs.c3cone(64, 48))
    ref, ost = oracle_bind.render_rows(p)
    o, d = Q.rays(N, 5)
    c = rt.RenderContext(0)
    try:
        c.set_scene(p)
        c.read_stats(reset=True)
        img1 = c.render()
        st1 = c.read_stats(reset=True)
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            rays = upload(ray_records(o, d))
        side.synchronize()
        hits = torch.empty(N * abi.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        occ = torch.empty(N, dtype=torch.uint8, device="cuda:0")
        for _ in range(3):
            c.query_closest_async(rays, hits, side)
            c.query_occluded_async(rays, occ, side)
        side.synchronize()
        img2 = c.render()
        st2 = c.read_stats(reset=True)
    finally:
        c.close()
    assert np.array_equal(img1, ref) and np.array_equal(img2, ref)
    assert st1.as_dict() == ost.as_dict() and st2.as_dict() == ost.as_dict()
    assert_hits_equal(hits.cpu().numpy().view(abi.HIT_DTYPE), Q.table("c3cone").closest(), "side stream")


# 8. errors leave the context usable; an empty scene answers all misses
def test_errors_and_empty_scene():
    import torch
    lib = rt.load_library()
    T = Q.table("c3cone")
    rays = upload(ray_records(T.origins, T.dirs))
    hits = torch.empty(N * abi.HIT_DTYPE.itemsize + 16, dtype=torch.uint8, device="cuda:0")
    occ = torch.empty(N, dtype=torch.uint8, device="cuda:0")
    rp, hp, op = rays.data_ptr(), hits.data_ptr(), occ.data_ptr()
    assert rp % 16 == 0 and hp % 16 == 0
    c = rt.RenderContext(0)

    def both(n, r, h, o):
        for rc in (lib.rt_query_closest_async(c.handle, n, C.c_void_p(r), C.c_void_p(h), None),
                   lib.rt_query_occluded_async(c.handle, n, C.c_void_p(r), C.c_void_p(o), None)):
            assert rc == abi.RT_E_INVALID
            assert lib.rt_last_error()

    try:
        both(N, rp, hp, op)  # no scene
        c.set_scene(Q.packed("c3cone"))
        both(-1, rp, hp, op)
        both(N - 1, rp + 8, hp, op)  # a ray pointer off by 8 bytes
        assert lib.rt_query_closest_async(c.handle, N - 1, C.c_void_p(rp), C.c_void_p(hp + 8), None) == abi.RT_E_INVALID
        both(N, rp, None, None)  # NULL outputs
        both(N, None, hp, op)
        assert lib.rt_query_closest_async(c.handle, 0, None, None, None) == abi.RT_OK
        c.query_closest_async(rays, hits[:N * abi.HIT_DTYPE.itemsize])
        torch.cuda.synchronize()
        got = hits[:N * abi.HIT_DTYPE.itemsize].cpu().numpy().view(abi.HIT_DTYPE)
        assert_hits_equal(got, T.closest(), "after the errors")
        empty = rt.scene.RenderArgs(ambient=(0.1, 0.1, 0.1), lights=[], scene=rt.scene.Union(()), depth=3,
                                    fov=90.0, width=16, height=16)
        c.set_scene(empty)
        got = gpu_closest(c, T.origins, T.dirs)
        assert (got["object"] == -1).all() and not got.view(np.uint8).reshape(N, -1)[:, :80].any()
        assert not gpu_occluded(c, T.origins, T.dirs).any()
    finally:
        c.close()


# 9. the synchronous helpers equal the async path
def test_synchronous_helpers(ctx):
    T = Q.table("mixed11")
    ctx.set_scene(Q.packed("mixed11"))
    so, sd, sex = Q.shadow_rays("mixed11")
    got = ctx.closest_hits(T.origins, T.dirs)
    assert got.dtype == abi.HIT_DTYPE and got.shape == (N,)
    assert got.tobytes() == gpu_closest(ctx, T.origins, T.dirs).tobytes()
    tm = np.linspace(0.5, 3.0, N)
    assert ctx.closest_hits(T.origins, T.dirs, tmax=tm, exclude=3).tobytes() == \
        gpu_closest(ctx, T.origins, T.dirs, tmax=tm, exclude=3).tobytes()
    occ = ctx.occluded(so, sd, tmax=1.0, exclude=sex)
    assert occ.dtype == np.bool_ and occ.shape == (len(so),)
    assert np.array_equal(occ, gpu_occluded(ctx, so, sd, tmax=1.0, exclude=sex).astype(bool))
    assert np.array_equal(ctx.occluded(T.origins, T.dirs), Q.table("mixed11").occluded())
    with pytest.raises(ValueError):
        ctx.closest_hits(T.origins[:, :2], T.dirs)


# 10. unit-length directions: a wave whose rays are all normalised takes the
# composite search with its FP32 leaf culls (csg_hit); rays() alone, whose
# directions are not unit length, never does
@pytest.mark.parametrize("name", ["c4csg", "mixed12"])
def test_unit_directions_equal_the_oracle(ctx, name):
    o, d = Q.rays(N, 5)
    d = d / np.linalg.norm(d, axis=1)[:, None]
    d[1::128] *= 3.0  # eight waves hold one longer direction each: those take the other search
    T = Q.Table(Q.packed(name), o, d)
    want = T.closest()
    occ = T.occluded(tmax=4.0)
    assert (want["object"] >= 0).sum() >= 500 and (want["object"] < 0).sum() >= 50
    assert occ.sum() >= 20 and (~occ).sum() >= 20
    if name == "c4csg":
        comp = want["face"][want["object"] >= 0]
        assert ((comp >> 4) > 0).sum() >= 20  # hits on the subtracted spheres' surfaces
    ctx.set_scene(Q.packed(name))
    assert_hits_equal(gpu_closest(ctx, o, d), want, name + " unit directions")
    assert np.array_equal(gpu_occluded(ctx, o, d, tmax=4.0).astype(bool), occ)


# 11. the any-hit bound is strict exactly at the closest hit: with tmax = t of
# the oracle's winner nothing occludes, one ulp further the winner does. Unit
# directions take the composite search with its leaf culls and its cut at the
# bound, longer ones the search without either (the head of rt_query.hip).
@pytest.mark.parametrize("length", [1.0, 3.0])
@pytest.mark.parametrize("name", ["mixed11", "mixed12", "c4csg"])
def test_occluded_bound_is_strict_at_the_closest_hit(ctx, name, length):
    T0 = Q.table(name)
    o, d = T0.origins[:256], T0.dirs[:256]
    d = d / np.linalg.norm(d, axis=1)[:, None] * length
    T = Q.Table(Q.packed(name), o, d)
    first = T.closest()
    hit = first["object"] >= 0
    assert hit.sum() >= 50
    at = np.where(hit, first["t"], np.inf)
    past = np.where(hit, np.nextafter(first["t"], np.inf), np.inf)
    want_at, want_past = T.occluded(tmax=at), T.occluded(tmax=past)
    assert not want_at.any() and np.array_equal(want_past, hit)
    ctx.set_scene(Q.packed(name))
    assert bool(ctx.scene_info() & abi.RT_INFO_BVH) == (name == "mixed12")
    assert np.array_equal(gpu_occluded(ctx, o, d, tmax=at).astype(bool), want_at)
    assert np.array_equal(gpu_occluded(ctx, o, d, tmax=past).astype(bool), want_past)
