"""Camera renders (rt_camera_rays_async, rt_render_camera_async,
rt_render_camera_chunks) on the device against tests/camera_ref.py, the
render kernel and the radiance queries (needs an MI355X).

Bar: bytes. The zero camera's frame equals render()'s; every field of every
ray equals camera_ref's (==, no tolerance); the fused render's mean and bytes
equal the materialised route (camera_rays_ex -> query_radiance_async -> an
ordered sum in Python floats). The frame is 13 x 23 unless stated: it crosses
the 20-row strip boundary and 299 pixels are no multiple of 64. Each test
first asserts, from the reference's side alone, what it is about.
"""
import ctypes as C

import numpy as np
import pytest

import go_raytracer_amd as rt
import camera_ref as CR
import oracle_bind
import trace_ref as T

abi = rt.abi
pytestmark = pytest.mark.gpu

RB = abi.RADIANCE_DTYPE.itemsize
W, H = 13, 23
OBLIQUE = dict(eye=(2.5, 1.75, -3.0), look_at=(0.25, -0.25, 6.0), up=(0.3, 1.0, -0.2))
MODELS = {
    "pinhole": dict(model="pinhole"),
    "ortho": dict(model="ortho", extent=6.5),
    "equirect": dict(model="equirect"),
    "thinlens": dict(model="thinlens", aperture=0.35, focus=4.5),
}
_packed = {}


def packed13(name):
    """c3 at 13 x 23, or a trace_ref scene (its own size: cameras then override it)."""
    if name not in _packed:
        _packed[name] = rt.scene.convert(rt.configs.c3(W, H)) if name == "c3@13x23" else T.packed(name)
    return _packed[name]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


def camera(**kw):
    return rt.RenderContext.camera(**kw)


def assert_rays_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == abi.RAY_DTYPE, what
    for k in abi.RAY_DTYPE.names:
        bad = np.asarray(got[k] != want[k])
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("%s: field %s differs in %d places; first at %s: gpu %s reference %s"
                                 % (what, k, bad.sum(), at, got[k][at[:3]], want[k][at[:3]]))
    assert got.tobytes() == want.tobytes(), what


def materialised(ctx, cam, y0=0, y1=None):
    """The parent route: the camera's rays written out, traced by the radiance
    query, summed in order, scaled and quantised in Python floats."""
    import torch
    rays = ctx.camera_rays_ex(cam, y0, y1)
    dev = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    out = torch.empty(rays.size * RB, dtype=torch.uint8, device="cuda:0")
    ctx.query_radiance_async(dev, out, int(cam.depth))
    torch.cuda.synchronize()
    rad = out.cpu().numpy().view(abi.RADIANCE_DTYPE).reshape(rays.shape)
    return CR.resolve(rad) + (rad,)


# 1. identity: the zero camera is Render()
@pytest.mark.parametrize("name", ["c2", "c3", "canned", "c4", "c4csg", "closure"])
def test_zero_camera_equals_render(ctx, name):
    p = T.packed(name)
    ctx.set_scene(p)
    assert (p.width, p.height) == ((16, 12) if name in ("c4", "c4csg") else (24, 16))
    if name == "c4":
        assert ctx.scene_info() & abi.RT_INFO_BVH and p.scene.depth == 8
    if name == "c4csg":
        assert ctx.scene_info() & abi.RT_INFO_CSG
    if name == "closure":
        assert p.scene.num_programs >= 1
    want = ctx.render()
    got = ctx.render_camera()
    assert got.shape == want.shape == (p.height, p.width, 4) and got.dtype == np.uint8
    assert np.array_equal(got, want), "%s: %d pixels differ" % (name, (got != want).any(axis=2).sum())
    assert np.array_equal(ctx.render_camera(abi.rt_camera()), want)
    assert np.array_equal(want, oracle_bind.render_rows(p)[0])


def test_zero_camera_band_equals_the_frames_rows(ctx):
    p = rt.scene.convert(rt.configs.c3(31, 45))
    ctx.set_scene(p)
    full = ctx.render()
    band = ctx.render_camera(None, 17, 43)  # starts mid-strip, crosses rows 20 and 40
    assert band.shape == (26, 31, 4)
    assert np.array_equal(band, full[17:43])
    assert np.array_equal(ctx.render_camera(), full)


# 2. the rays, field by field
RAY_CASES = {
    "pinhole-s1": (dict(samples=1), None),
    "pinhole-s2": (dict(samples=2), None),
    "pinhole-s3": (dict(samples=3), None),
    "pinhole-s4": (dict(samples=4), None),
    "pinhole-s9": (dict(samples=9), None),
    "pinhole-s16": (dict(samples=16), None),
    "ortho": (dict(samples=3, **MODELS["ortho"]), None),
    "equirect": (dict(samples=3, **MODELS["equirect"]), None),
    "thinlens": (dict(samples=3, **MODELS["thinlens"]), None),
    "posed-pinhole": (dict(samples=3, **OBLIQUE), None),
    "posed-thinlens": (dict(samples=3, **MODELS["thinlens"], **OBLIQUE), None),
    "size-17x21": (dict(samples=3, size=(17, 21)), None),
    "fov": (dict(samples=3, fov=38.5), None),
    "s1024-2x22": (dict(samples=1024, size=(2, 22)), None),
    "band": (dict(samples=3), (17, 23)),
}


@pytest.mark.parametrize("case", list(RAY_CASES))
def test_camera_rays_equal_the_reference(ctx, case):
    kw, band = RAY_CASES[case]
    name = "c3" if case == "size-17x21" else "c3@13x23"
    p = packed13(name)
    assert (p.width, p.height) == ((24, 16) if case == "size-17x21" else (W, H))
    cam = camera(**kw)
    y0, y1 = band or (0, None)
    want = CR.rays(p, cam, y0, y1)
    fw, fh, S, D = CR.frame(p, cam)
    assert (fw, fh) == kw.get("size", (W, H)) and S == kw["samples"]
    assert want.shape == ((y1 or fh) - y0, fw, S)
    assert y0 < 20 < (y1 or fh)  # rows on both sides of the strip boundary
    assert (want["tmax"] == np.inf).all() and (want["exclude"] == -1).all() and (want["reserved"] == 0).all()
    plain = CR.rays(p, camera(samples=S), y0, y1) if fw == W and fh == H else None
    if "thinlens" in case:
        assert D == 4
        o = want["origin"].reshape(-1, 3)
        eye = np.array(kw.get("eye", (0.0, 0.0, -1.0)))
        assert (o != eye).any(axis=1).all() and len(np.unique(o, axis=0)) == len(o)
    if case == "equirect":
        d = want["dir"].reshape(-1, 3)
        for k in range(3):
            assert (d[:, k] > 0.1).any() and (d[:, k] < -0.1).any()
        assert (want["origin"] == (0.0, 0.0, -1.0)).all()
    if case == "ortho":
        assert (want["dir"] == (0.0, 0.0, 1.0)).all() and len(np.unique(want["origin"].reshape(-1, 3), axis=0)) > 100
    if case.startswith("posed") or case == "fov":
        assert (want["dir"] != plain["dir"]).any(axis=-1).all()
    if case == "s1024-2x22":
        assert len(np.unique(want["origin"][21, 1, :, 0])) == 1024  # the last row's draws, the largest jump
    if case == "pinhole-s4":  # the zero camera: the older export's records
        assert want.tobytes() == T.camera_rays(p, 0, H).tobytes()
    ctx.set_scene(p)
    got = ctx.camera_rays_ex(cam, y0, y1)
    assert_rays_equal(got, want, case)


def test_zero_camera_rays_equal_the_older_export(ctx):
    ctx.set_scene(packed13("c3@13x23"))
    assert ctx.camera_rays_ex().tobytes() == ctx.camera_rays().tobytes()
    assert ctx.camera_rays_ex(None, 17, 23).tobytes() == ctx.camera_rays(17, 23).tobytes()


# 3. fused against materialised
@pytest.mark.parametrize("name", ["glass21", "c4csg", "closure", "glass22"])
@pytest.mark.parametrize("model", list(MODELS))
def test_fused_render_equals_the_materialised_route(ctx, model, name):
    p = packed13(name)
    ctx.set_scene(p)
    if name == "glass21":
        assert p.scene.num_objects == 10 and p.scene.depth == 5
    assert bool(ctx.scene_info() & abi.RT_INFO_BVH) == (name == "glass22")
    assert bool(ctx.scene_info() & abi.RT_INFO_CSG) == (name == "c4csg")
    assert (p.scene.num_programs >= 1) == (name == "closure")
    cam = camera(samples=3, size=(W, H), **MODELS[model])
    img, mean, rad = materialised(ctx, cam)
    # (the checked cube has three colours on a black background)
    assert rad.shape == (H, W, 3)
    assert len(np.unique(rad["color"].reshape(-1, 3), axis=0)) >= (2 if name == "closure" else 20)
    if model != "equirect" or name != "closure":
        assert (rad["object"] >= 0).any()
    if name.startswith("glass") and model != "equirect":
        assert (rad["rays"] > 1).any()
    got, gmean = ctx.render_camera(cam, mean=True)
    assert gmean.shape == (H, W, 3) and gmean.dtype == np.float64
    assert np.array_equal(gmean, mean), "%d means differ" % (gmean != mean).any(axis=2).sum()
    assert np.array_equal(got, img)
    assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("depth", [1, 2])
def test_depth_override(ctx, depth):
    p = packed13("glass21")
    ctx.set_scene(p)
    cam = camera(samples=3, size=(W, H), depth=depth)
    img, mean, rad = materialised(ctx, cam)
    scene_depth = materialised(ctx, camera(samples=3, size=(W, H)))[2]
    # depth 1 traces the camera's ray alone, depth 2 at most its two children; the scene's depth goes deeper
    assert rad["rays"].max() == 1 if depth == 1 else 1 < rad["rays"].max() <= 3
    assert scene_depth["rays"].max() > rad["rays"].max()
    got, gmean = ctx.render_camera(cam, mean=True)
    assert np.array_equal(gmean, mean) and np.array_equal(got, img)


# 4. chunking
def test_chunk_sizes_give_identical_frames(ctx):
    p = packed13("glass21")
    ctx.set_scene(p)
    assert W % 7 != 0 and (W * H) % 7 != 0  # a chunk boundary falls inside a row; the last chunk is short
    res = {}
    for cp in (7, 64, 0):
        cam = camera(samples=5, size=(W, H), chunk_pixels=cp, **OBLIQUE)
        n = ctx.render_camera_chunks(cam)
        assert n == (1 if cp == 0 else -(-W * H // cp))
        assert n >= 3 if cp == 7 else True
        res[cp] = ctx.render_camera(cam, mean=True)
        assert ctx.render_camera_chunks(cam, 17, 23) == (1 if cp == 0 else -(-W * 6 // cp))
    for cp in (7, 64):
        assert np.array_equal(res[cp][0], res[0][0]) and np.array_equal(res[cp][1], res[0][1])
    img, mean, _ = materialised(ctx, camera(samples=5, size=(W, H), **OBLIQUE))
    assert np.array_equal(res[0][0], img) and np.array_equal(res[0][1], mean)
    # a sample count that does not divide the buffer: 2097152 // 1000 pixels per chunk
    assert ctx.render_camera_chunks(camera(samples=1000, size=(2098, 2))) == 3


# 5. accel independence and the outputs
def test_accel_settings_give_identical_bytes():
    cam = camera(samples=3, size=(W, H), **MODELS["thinlens"])
    c = rt.RenderContext(0)
    try:
        res = []
        for flags in (0, abi.RT_ACCEL_CULL, abi.RT_ACCEL_BVH, abi.RT_ACCEL_BVH | abi.RT_ACCEL_CULL):
            c.set_accel(flags)
            c.set_scene(T.packed("glass22"))
            assert bool(c.scene_info() & abi.RT_INFO_BVH) == bool(flags & abi.RT_ACCEL_BVH)
            img, mean = c.render_camera(cam, mean=True)
            res.append(img.tobytes() + mean.tobytes())
        for r in res[1:]:
            assert r == res[0]
    finally:
        c.close()


def test_outputs_agree_and_leave_the_rest_of_a_buffer_alone(ctx):
    import torch
    ctx.set_scene(packed13("glass21"))
    cam = camera(samples=3, size=(W, H), **OBLIQUE)
    img, mean = ctx.render_camera(cam, mean=True)
    assert len(np.unique(img.reshape(-1, 4), axis=0)) >= 20
    rgba = torch.full((H, W, 4), 0xA5, dtype=torch.uint8, device="cuda:0")
    m = torch.full((H, W, 3), -7.0, dtype=torch.float64, device="cuda:0")
    ctx.render_camera_async(cam, 17, 22, rgba=rgba[17:22])
    ctx.render_camera_async(cam, 3, 9, mean=m[3:9])
    torch.cuda.synchronize()
    rgba, m = rgba.cpu().numpy(), m.cpu().numpy()
    assert np.array_equal(rgba[17:22], img[17:22]) and (rgba[:17] == 0xA5).all() and (rgba[22:] == 0xA5).all()
    assert np.array_equal(m[3:9], mean[3:9]) and (m[:3] == -7.0).all() and (m[9:] == -7.0).all()


# 6. no side effects on renders, their counters, specialisation, tile order and radiance queries
def test_camera_renders_leave_the_context_alone():
    import torch
    p = rt.scene.convert(rt.configs.c3cone(64, 48))
    ref, ost = oracle_bind.render_rows(p)
    o, d = T.ray_set(256)
    rec = np.zeros(256, dtype=abi.RAY_DTYPE)
    rec["origin"], rec["dir"], rec["tmax"], rec["exclude"] = o, d, np.inf, -1
    cam = camera(samples=5, size=(W, H), **MODELS["thinlens"], **OBLIQUE)
    c = rt.RenderContext(0)
    try:
        c.set_scene(p)
        c.read_stats(reset=True)
        state0 = (c.specialized()[0], c.tile_order_info()[0], c.scene_info())
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            img = [torch.empty((48, 64, 4), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
            rays = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
            out = [torch.empty(256 * RB, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
            rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
            zero = torch.empty((48, 64, 4), dtype=torch.uint8, device="cuda:0")
            crays = torch.empty(H * W * 5 * 64, dtype=torch.uint8, device="cuda:0")
        side.synchronize()
        c.render_rows_async(0, 48, img[0], side)
        c.query_radiance_async(rays, out[0], 0, side)
        c.render_camera_async(cam, 0, H, rgba=rgba, stream=side)
        c.render_camera_async(None, 0, 48, rgba=zero, stream=side)
        c.camera_rays_ex_async(cam, 0, H, crays, side)
        c.query_radiance_async(rays, out[1], 0, side)
        c.render_rows_async(0, 48, img[1], side)
        side.synchronize()
        st = c.read_stats(reset=True)
        assert (c.specialized()[0], c.tile_order_info()[0], c.scene_info()) == state0
        plain = c.render()
        st1 = c.read_stats(reset=True)
    finally:
        c.close()
    assert np.array_equal(img[0].cpu().numpy(), ref) and np.array_equal(img[1].cpu().numpy(), ref)
    assert np.array_equal(zero.cpu().numpy(), ref)
    assert np.array_equal(plain, ref) and st1.as_dict() == ost.as_dict()
    two = {k: (2 * v if not isinstance(v, list) else [2 * x for x in v]) for k, v in ost.as_dict().items()}
    assert st.as_dict() == two  # two renders' counters, nothing from the camera renders
    assert out[0].cpu().numpy().tobytes() == out[1].cpu().numpy().tobytes()
    assert len(np.unique(rgba.cpu().numpy().reshape(-1, 4), axis=0)) >= 10


# 7. errors name the function and leave the context usable
def test_errors_leave_the_context_usable():
    import torch
    lib = rt.load_library()
    c = rt.RenderContext(0)
    buf = torch.empty(24 * 16 * 4 * 64 + 64, dtype=torch.uint8, device="cuda:0")
    bp = buf.data_ptr()
    assert bp % 16 == 0

    def invalid(cam, y0=0, y1=16, rays=bp, rgba=bp, mean=bp, text=None):
        ref = None if cam is None else C.byref(cam)
        checks = [("rt_camera_rays_async", lib.rt_camera_rays_async(c.handle, ref, y0, y1, C.c_void_p(rays), None))]
        msg = [lib.rt_last_error()]
        checks.append(("rt_render_camera_async",
                       lib.rt_render_camera_async(c.handle, ref, y0, y1, C.c_void_p(rgba), C.c_void_p(mean), None)))
        msg.append(lib.rt_last_error())
        for (who, rc), m in zip(checks, msg):
            assert rc == abi.RT_E_INVALID, (who, rc)
            assert who.encode() in m and (text is None or text in m), m

    def invalid_plan(cam, y0=0, y1=16, text=None):
        invalid(cam, y0, y1, text=text)
        assert lib.rt_render_camera_chunks(c.handle, C.byref(cam), y0, y1) == abi.RT_E_INVALID
        assert b"rt_render_camera_chunks" in lib.rt_last_error()

    try:
        invalid(None, text=b"no scene")
        assert lib.rt_render_camera_chunks(c.handle, None, 0, 16) == abi.RT_E_INVALID
        c.set_scene(T.packed("c2"))  # 24 x 16
        want = c.render()
        invalid_plan(camera(model=4), text=b"model")
        invalid_plan(camera(model=-1), text=b"model")
        bad = camera()
        bad.flags = 2
        invalid_plan(bad, text=b"flag")
        invalid_plan(camera(samples=-1), text=b"samples")
        invalid_plan(camera(samples=abi.RT_CAMERA_MAX_SAMPLES + 1), text=b"samples")
        for size in ((1, 16), (24, 1), (0, 16), (24, 0), (-3, -3), (65536, 65536)):
            invalid_plan(camera(size=size), 0, 1)
        invalid_plan(camera(depth=-1), text=b"depth")
        invalid_plan(camera(depth=abi.RT_RADIANCE_MAX_DEPTH + 1), text=b"depth")
        invalid_plan(camera(chunk_pixels=-1), text=b"chunk_pixels")
        for y0, y1 in ((0, 0), (5, 5), (7, 3), (-1, 4), (0, 17), (16, 17)):
            invalid_plan(camera(), y0, y1, text=b"rows")
        invalid_plan(camera(size=(30, 10)), 0, 11, text=b"rows")  # the camera's height, not the scene's
        for extent in (0.0, -2.0, float("nan"), float("inf")):
            invalid_plan(camera(model="ortho", extent=extent), text=b"extent")
        for focus in (0.0, -1.0, float("nan")):
            invalid_plan(camera(model="thinlens", aperture=0.1, focus=focus), text=b"focus")
        for aperture in (-0.1, float("nan"), float("inf")):
            invalid_plan(camera(model="thinlens", aperture=aperture, focus=3.0), text=b"aperture")
        invalid_plan(camera(eye=(1.0, 2.0, 3.0), look_at=(1.0, 2.0, 3.0)), text=b"look_at")
        invalid_plan(camera(eye=(0.0, 0.0, -1.0), look_at=(0.0, 0.0, 0.0), up=(0.0, 0.0, 2.0)), text=b"up")
        invalid_plan(camera(eye=(0.0, 0.0, -1.0), look_at=(0.0, 4.0, -1.0), up=(0.0, -1.0, 0.0)), text=b"up")
        invalid_plan(camera(eye=(0.0, float("nan"), -1.0)))
        # buffers
        z = camera()
        for ref in (None, C.byref(z)):
            assert lib.rt_camera_rays_async(c.handle, ref, 0, 16, None, None) == abi.RT_E_INVALID
            assert lib.rt_camera_rays_async(c.handle, ref, 0, 16, C.c_void_p(bp + 8), None) == abi.RT_E_INVALID
            assert b"rt_camera_rays_async" in lib.rt_last_error() and b"aligned" in lib.rt_last_error()
            assert lib.rt_render_camera_async(c.handle, ref, 0, 16, None, None, None) == abi.RT_E_INVALID
            assert b"both NULL" in lib.rt_last_error()
            assert lib.rt_render_camera_async(c.handle, ref, 0, 16, C.c_void_p(bp), C.c_void_p(bp + 4), None) \
                == abi.RT_E_INVALID
            assert b"rt_render_camera_async" in lib.rt_last_error() and b"aligned" in lib.rt_last_error()
        # what is out of range only for the models that read it is accepted elsewhere
        assert c.render_camera_chunks(camera(extent=-1.0, focus=-1.0, aperture=-1.0)) == 1
        assert c.render_camera_chunks(camera(model="ortho", extent=2.0, fov=-5.0, focus=-1.0)) == 1
        # the context still renders, and the zero camera still is Render()
        assert np.array_equal(c.render_camera(), want)
        assert c.camera_rays_ex().tobytes() == CR.rays(T.packed("c2")).tobytes()
        assert np.array_equal(c.render(), want)
    finally:
        c.close()


# 8. the CLI routes `render` through a camera render when a camera flag is given
def test_cli_camera_flags_route_the_programs_render(ctx, tmp_path):
    import os
    from go_raytracer_amd import cli, gml
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gml", "checked-cube.gml")
    ap = cli.build_parser()
    for d in ("plain", "four", "ortho"):
        (tmp_path / d).mkdir()
    plain = cli.render_program(path, str(tmp_path / "plain"), camera=cli.camera_from_args(ap.parse_args([path])))
    four = cli.render_program(path, str(tmp_path / "four"),
                              camera=cli.camera_from_args(ap.parse_args(["--samples", "4", path])))
    cam = cli.camera_from_args(ap.parse_args(["--camera", "ortho", "--extent", "5", "--samples", "2", "--size",
                                              "13x23", path]))
    ortho = cli.render_program(path, str(tmp_path / "ortho"), camera=cam)
    assert len(plain) == len(four) == len(ortho) == 1
    a, b, c = (rt.imageio.read_image(p[0]) for p in (plain, four, ortho))
    assert np.array_equal(a, b)  # the zero camera at 4 samples is the program's own render
    ctx.set_scene(gml.run_file(path)[0][0][0])
    assert c.shape[:2] == (23, 13) and np.array_equal(c[..., :3], ctx.render_camera(cam)[..., :3])
