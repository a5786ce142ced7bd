"""Radiance queries and camera-ray export (rt_query_radiance_async,
rt_query_camera_rays_async) on the device against tests/trace_ref.py and the
oracle's renders (needs an MI355X).

Bar: every colour component (==, no tolerance), object and ray count of every
record equals the reference's; frames rebuilt from the camera's rays equal
oracle_render_rows byte for byte. Each test first asserts, from the
reference's side alone, that its inputs still cover what it is about.
"""
import ctypes as C

import numpy as np
import pytest

import go_raytracer_amd as rt
import oracle_bind
import trace_ref as T

abi = rt.abi
pytestmark = pytest.mark.gpu

RB = abi.RADIANCE_DTYPE.itemsize
FRAME_SCENES = ["c2", "c3", "c3cone", "canned", "c4csg", "closure", "c4"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


def ray_records(origins, dirs, tmax=None, exclude=None):
    rec = np.zeros(len(origins), dtype=abi.RAY_DTYPE)
    rec["origin"] = origins
    rec["dir"] = dirs
    rec["tmax"] = np.inf if tmax is None else tmax
    rec["exclude"] = -1 if exclude is None else exclude
    return rec


def upload(rec):
    import torch
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")


def gpu_radiance(ctx, origins, dirs, depth=0, tmax=None, exclude=None, stream=None):
    import torch
    rays = upload(ray_records(origins, dirs, tmax, exclude))
    out = torch.empty(len(origins) * RB, dtype=torch.uint8, device="cuda:0")
    ctx.query_radiance_async(rays, out, depth, stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(abi.RADIANCE_DTYPE)


def assert_radiance_equal(got, want, what):
    assert len(got) == len(want), what
    if len(want) == 0:
        return
    bad = np.zeros(len(want), dtype=bool)
    for k in abi.RADIANCE_DTYPE.names:
        bad |= np.asarray(got[k] != want[k]).reshape(len(want), -1).any(axis=1)
    if bad.any():
        r = int(np.argwhere(bad).ravel()[0])
        raise AssertionError("%s: %d of %d records differ; first ray %d: gpu %s reference %s"
                             % (what, bad.sum(), len(want), r, got[r], want[r]))


# 1. camera identity: the camera's rays, traced and averaged, are the oracle's frame
@pytest.mark.parametrize("name", FRAME_SCENES)
def test_camera_rays_traced_reproduce_the_oracle_frame(ctx, name):
    import torch
    p = T.packed(name)
    ref, st = oracle_bind.render_rows(p)
    ctx.set_scene(p)
    if name == "c4":
        assert ctx.scene_info() & abi.RT_INFO_BVH and p.scene.depth == 8
    if name == "closure":
        assert p.scene.num_programs >= 1
    H, W = p.height, p.width
    rays = torch.empty(H * W * 4 * abi.RAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(H * W * 4 * RB, dtype=torch.uint8, device="cuda:0")
    ctx.camera_rays_async(0, H, rays)
    ctx.query_radiance_async(rays, out)
    img = ctx.image_from_radiance(out, 4)
    torch.cuda.synchronize()
    assert img.shape == (H, W, 4) and img.dtype == torch.uint8
    img = img.cpu().numpy()
    rad = out.cpu().numpy().view(abi.RADIANCE_DTYPE)
    assert np.array_equal(img, ref), "%s: %d pixels differ" % (name, (img != ref).any(axis=2).sum())
    assert int(rad["rays"].sum()) == int(st.primary_rays) + int(st.secondary_rays)


# 2. the camera's rays themselves, whole frame and a band that starts mid-strip
def test_camera_rays_equal_the_reference(ctx):
    p = rt.scene.convert(rt.configs.c2(31, 45))
    ctx.set_scene(p)
    full = ctx.camera_rays()
    want = T.camera_rays(p, 0, 45)
    assert full.dtype == abi.RAY_DTYPE and full.shape == (45, 31, 4)
    assert full.tobytes() == want.tobytes()
    band = ctx.camera_rays(17, 43)  # starts mid-strip, crosses the boundaries at rows 20 and 40
    assert band.shape == (26, 31, 4)
    assert band.tobytes() == want[17:43].tobytes()
    assert band.tobytes() == T.camera_rays(p, 17, 43).tobytes()


# 3. arbitrary rays (non-unit directions, half the origins inside the scene box)
@pytest.mark.parametrize("name,n,depth", [("glass21", 1024, 1), ("glass21", 1024, 2), ("glass21", 1024, 5),
                                          ("glass22", 256, 4), ("c4csg", 1024, 0), ("closure", 1024, 0)])
def test_arbitrary_rays_equal_the_reference(ctx, name, n, depth):
    want = T.reference(name, n, depth)
    if name.startswith("glass"):
        if depth == 1:
            assert (want["rays"] == 1).all()
        if depth >= 4:  # the deepest depth of the scene's cases
            assert (want["rays"] > 1).mean() >= 0.15
            assert (want["rays"] >= 4).mean() >= 0.02
        assert (want["object"] < 0).sum() >= 1
        assert len(np.unique(want["color"], axis=0)) >= n // 4
    else:
        assert (want["object"] < 0).sum() >= 1 and (want["object"] >= 0).sum() >= 1
    ctx.set_scene(T.packed(name))
    assert bool(ctx.scene_info() & abi.RT_INFO_BVH) == (name == "glass22")
    o, d = T.ray_set(n)
    assert_radiance_equal(gpu_radiance(ctx, o, d, depth), want, "%s depth %d" % (name, depth))


# 4. tmax and exclude act on the ray's own hit only
def test_tmax_and_exclude_bound_the_first_hit_only(ctx):
    name, n, depth = "glass21", 1024, 5
    p = T.packed(name)
    sc = T.scene_of(p)
    o, d = T.ray_set(n)
    first = T.reference(name, n, depth)
    hit = first["object"] >= 0
    assert hit.sum() >= 500
    t = np.full(n, np.inf)
    for r in np.argwhere(hit).ravel():
        h = T.closest_hit(sc, tuple(o[r]), tuple(d[r]))
        assert h[0] == first["object"][r]
        t[r] = h[1]
    ex = first["object"].astype(np.int32)  # (-1 for a miss: none)
    ctx.set_scene(p)
    want = T.reference(name, n, depth, exclude=ex, key="exclude")
    assert (want["object"][hit] != first["object"][hit]).all() and (want["object"][hit] >= 0).sum() >= 100
    # secondary rays still see the excluded object: some trees meet it again
    assert (want["rays"] > 1).sum() >= 50
    assert_radiance_equal(gpu_radiance(ctx, o, d, depth, exclude=ex), want, "exclude")
    tm = np.where(hit, t * 0.5, np.inf)
    want = T.reference(name, n, depth, tmax=tm, key="tmax")
    assert (want["object"] == -1).all() and (want["rays"] == 1).all()  # nothing lies before half the first hit
    assert_radiance_equal(gpu_radiance(ctx, o, d, depth, tmax=tm), want, "tmax")
    # both: what lies behind the winner within twice its distance
    tm2 = np.where(hit, t * 2.0, np.inf)
    want = T.reference(name, n, depth, tmax=tm2, exclude=ex, key="both")
    assert (want["object"][hit] >= 0).sum() >= 20 and (want["object"][hit] < 0).sum() >= 20
    assert_radiance_equal(gpu_radiance(ctx, o, d, depth, tmax=tm2, exclude=ex), want, "tmax and exclude")


# 5. all four accel settings return identical records
@pytest.mark.parametrize("name,n,depth", [("glass22", 256, 4), ("c4csg", 1024, 0)])
def test_accel_settings_give_identical_bytes(name, n, depth):
    o, d = T.ray_set(n)
    c = rt.RenderContext(0)
    try:
        res = []
        for flags in (0, abi.RT_ACCEL_CULL, abi.RT_ACCEL_BVH, abi.RT_ACCEL_BVH | abi.RT_ACCEL_CULL):
            c.set_accel(flags)
            c.set_scene(T.packed(name))
            bvh = bool(c.scene_info() & abi.RT_INFO_BVH)
            assert bvh == (name == "glass22" and bool(flags & abi.RT_ACCEL_BVH))
            res.append(gpu_radiance(c, o, d, depth).tobytes())
        for r in res[1:]:
            assert r == res[0]
        assert_radiance_equal(np.frombuffer(res[0], dtype=abi.RADIANCE_DTYPE), T.reference(name, n, depth), name)
    finally:
        c.close()


# 6. batch edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_batch_sizes_and_untouched_tail(ctx, n):
    import torch
    N = 1024
    want = T.reference("glass21", N, 5)
    ctx.set_scene(T.packed("glass21"))
    o, d = T.ray_set(N)
    rays = upload(ray_records(o, d))
    out = torch.full((N * RB,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ctx.query_radiance_async(rays[:n * 64], out[:n * RB], 5)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert_radiance_equal(out[:n * RB].view(abi.RADIANCE_DTYPE), want[:n], "first %d rays" % n)
    assert (out[n * RB:] == 0xA5).all()


def test_batch_larger_than_the_persistent_grid(ctx):
    """Every lane takes several rays from the ticket counter: 256 distinct rays
    tiled in a shuffled order to twice the grid's lane count."""
    import torch
    want = T.reference("c2", 256, 0)
    assert (want["object"] < 0).sum() >= 10 and len(set(want["object"])) >= 3
    ctx.set_scene(T.packed("c2"))
    lanes = ctx.radiance_lanes()
    assert lanes >= 256 and lanes % 256 == 0
    assert lanes == ctx.radiance_lanes(T.packed("c2").scene.depth)
    total = 2 * lanes + 37
    src = np.random.default_rng(7).integers(0, 256, total)
    o, d = T.ray_set(256)
    rays = upload(ray_records(o, d)[src])
    out = torch.empty(total * RB, dtype=torch.uint8, device="cuda:0")
    ctx.query_radiance_async(rays, out)
    torch.cuda.synchronize()
    assert_radiance_equal(out.cpu().numpy().view(abi.RADIANCE_DTYPE), want[src], "tiled batch of %d" % total)


# 7. the workspace grows with the depth (and deep calls run on fewer lanes)
def test_workspace_growth_keeps_answers():
    o, d = T.ray_set(256)
    p = T.packed("glass21")
    deep = abi.RT_RADIANCE_MAX_DEPTH
    fresh = {}
    for depth in (2, deep):
        c = rt.RenderContext(0)
        try:
            c.set_scene(p)
            fresh[depth] = gpu_radiance(c, o, d, depth)
            if depth == deep:
                assert c.radiance_lanes(deep) < c.radiance_lanes(2)  # the workspace bound shrinks the grid
        finally:
            c.close()
    assert_radiance_equal(fresh[2], T.reference("glass21", 256, 2), "depth 2")
    assert (fresh[deep]["rays"] > 3).any()  # more than depth 2 can trace (1 + 2 children)
    c = rt.RenderContext(0)
    try:
        c.set_scene(p)
        for depth in (2, deep, 2):
            assert_radiance_equal(gpu_radiance(c, o, d, depth), fresh[depth], "depth %d on one context" % depth)
    finally:
        c.close()


# 8. no side effects on renders, their counters, specialisation and tile order
def test_radiance_queries_leave_renders_and_counters_alone():
    import torch
    p = rt.scene.convert(rt.configs.c3cone(64, 48))
    ref, ost = oracle_bind.render_rows(p)
    o, d = T.ray_set(256)
    c = rt.RenderContext(0)
    try:
        c.set_scene(p)
        c.read_stats(reset=True)
        state0 = (c.specialized()[0], c.tile_order_info()[0], c.scene_info())
        side = torch.cuda.Stream(device=0)
        img = [torch.empty((48, 64, 4), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        with torch.cuda.stream(side):
            rays = upload(ray_records(o, d))
            out = torch.empty(256 * RB, dtype=torch.uint8, device="cuda:0")
            cam = torch.empty(48 * 64 * 4 * 64, dtype=torch.uint8, device="cuda:0")
        side.synchronize()
        c.render_rows_async(0, 48, img[0], side)
        c.query_radiance_async(rays, out, 0, side)
        c.camera_rays_async(0, 48, cam, side)
        c.render_rows_async(0, 48, img[1], side)
        side.synchronize()
        st = c.read_stats(reset=True)
        assert (c.specialized()[0], c.tile_order_info()[0], c.scene_info()) == state0
        plain = c.render()
        st1 = c.read_stats(reset=True)
    finally:
        c.close()
    assert np.array_equal(img[0].cpu().numpy(), ref) and np.array_equal(img[1].cpu().numpy(), ref)
    assert np.array_equal(plain, ref) and st1.as_dict() == ost.as_dict()
    two = {k: (2 * v if not isinstance(v, list) else [2 * x for x in v]) for k, v in ost.as_dict().items()}
    assert st.as_dict() == two  # two renders' counters, nothing from the queries
    assert_radiance_equal(out.cpu().numpy().view(abi.RADIANCE_DTYPE),
                          T.trace_many(p, o, d, 0), "between two renders")


# 9. errors name the function and leave the context usable
def test_errors_leave_the_context_usable():
    import torch
    lib = rt.load_library()
    N = 256
    o, d = T.ray_set(N)
    rays = upload(ray_records(o, d))
    out = torch.empty(N * RB + 16, dtype=torch.uint8, device="cuda:0")
    cam = torch.empty(16 * 24 * 4 * 64 + 16, dtype=torch.uint8, device="cuda:0")
    rp, op, cp = rays.data_ptr(), out.data_ptr(), cam.data_ptr()
    assert rp % 16 == 0 and op % 16 == 0 and cp % 16 == 0
    c = rt.RenderContext(0)

    def rad_invalid(n, r, depth, o_):
        assert lib.rt_query_radiance_async(c.handle, n, C.c_void_p(r), depth, C.c_void_p(o_), None) == abi.RT_E_INVALID
        assert b"rt_query_radiance_async" in lib.rt_last_error()

    def cam_invalid(y0, y1, ptr):
        assert lib.rt_query_camera_rays_async(c.handle, y0, y1, C.c_void_p(ptr), None) == abi.RT_E_INVALID
        assert b"rt_query_camera_rays_async" in lib.rt_last_error()

    try:
        rad_invalid(N, rp, 0, op)  # no scene
        cam_invalid(0, 16, cp)
        c.set_scene(T.packed("c2"))  # 24 x 16
        rad_invalid(-1, rp, 0, op)
        rad_invalid(N, rp, -1, op)
        rad_invalid(N, rp, abi.RT_RADIANCE_MAX_DEPTH + 1, op)
        rad_invalid(N, None, 0, op)
        rad_invalid(N, rp, 0, None)
        rad_invalid(N - 1, rp + 8, 0, op)  # a ray pointer off by 8 bytes
        rad_invalid(N - 1, rp, 0, op + 8)
        for y0, y1 in ((0, 0), (5, 5), (7, 3), (-1, 4), (0, 17), (16, 17)):
            cam_invalid(y0, y1, cp)
        cam_invalid(0, 16, None)
        cam_invalid(0, 16, cp + 8)
        assert lib.rt_query_radiance_async(c.handle, 0, None, 0, None, None) == abi.RT_OK
        assert lib.rt_query_radiance_lanes(c.handle, -1) == abi.RT_E_INVALID
        assert lib.rt_query_radiance_lanes(c.handle, abi.RT_RADIANCE_MAX_DEPTH + 1) == abi.RT_E_INVALID
        assert_radiance_equal(gpu_radiance(c, o, d), T.reference("c2", N, 0), "after the errors")
        assert c.camera_rays().tobytes() == T.camera_rays(T.packed("c2"), 0, 16).tobytes()
    finally:
        c.close()


# 10. the synchronous helpers equal the async path
def test_synchronous_helpers(ctx):
    ctx.set_scene(T.packed("glass21"))
    o, d = T.ray_set(256)
    got = ctx.radiance(o, d)
    assert got.dtype == abi.RADIANCE_DTYPE and got.shape == (256,)
    assert got.tobytes() == gpu_radiance(ctx, o, d, 0).tobytes()
    assert_radiance_equal(got, T.reference("glass21", 256, 5), "scene depth")
    tm = np.linspace(0.5, 3.0, 256)
    assert ctx.radiance(o, d, depth=2, tmax=tm, exclude=3).tobytes() == \
        gpu_radiance(ctx, o, d, 2, tmax=tm, exclude=3).tobytes()
    with pytest.raises(ValueError):
        ctx.radiance(o[:, :2], d)
    import torch
    H, W = 16, 16
    buf = torch.empty(6 * W * 4 * 64, dtype=torch.uint8, device="cuda:0")
    ctx.camera_rays_async(3, 9, buf)
    torch.cuda.synchronize()
    rows = ctx.camera_rays(3, 9)
    assert rows.shape == (6, W, 4) and rows.tobytes() == buf.cpu().numpy().tobytes()
    assert ctx.camera_rays().shape == (H, W, 4)
    # image_from_radiance: the reference's sum order and quantisation
    flat = rows.reshape(-1)
    out = torch.empty(len(flat) * RB, dtype=torch.uint8, device="cuda:0")
    ctx.query_radiance_async(buf, out)
    img = ctx.image_from_radiance(out, 4)
    torch.cuda.synchronize()
    rad = out.cpu().numpy().view(abi.RADIANCE_DTYPE).reshape(6, W, 4)
    assert np.array_equal(img.cpu().numpy(), T.image(rad))
    assert np.array_equal(img.cpu().numpy(), oracle_bind.render_rows(T.packed("glass21"), 3, 9)[0])
