"""Feature buffers of a camera render (rt_render_camera_aov_async) on the
device against tests/aov_ref.py, the closest-hit query and the render kernel
(needs an MI355X).

Bar: every field of every buffer equals the reference's (==, or both NaN: the
edge-ray tests' contract; ids as integers). The frame is 13 x 23 unless stated:
it crosses the 20-row strip boundary and 299 pixels are no multiple of 64.
Each test first asserts, from the reference's side alone, what it is about.
"""
import ctypes as C
import os

import numpy as np
import pytest

import go_raytracer_amd as rt
import aov_ref as AR
import oracle_bind
import trace_ref as T

abi = rt.abi
pytestmark = pytest.mark.gpu

W, H = 13, 23
OBLIQUE = dict(eye=(2.5, 1.75, -3.0), look_at=(0.25, -0.25, 6.0), up=(0.3, 1.0, -0.2))
MODELS = {  # tests/test_gpu_camera.py MODELS
    "pinhole": dict(model="pinhole"),
    "ortho": dict(model="ortho", extent=6.5),
    "equirect": dict(model="equirect"),
    "thinlens": dict(model="thinlens", aperture=0.35, focus=4.5),
}
SCENES = ["c3", "c4", "c4csg", "closure"]
GML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gml")
_gml = {}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


def camera(**kw):
    return rt.RenderContext.camera(**kw)


def assert_buffers_equal(got, want, what, names=AR.NAMES):
    for k in names:
        g, w = got[k], want[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if k == "ids":
            for f in abi.AOV_IDS_DTYPE.names:
                bad = g[f] != w[f]
                assert not bad.any(), "%s: ids.%s differs in %d pixels; first at %s: gpu %s reference %s" % (
                    what, f, bad.sum(), np.argwhere(bad)[0], g[f][bad][0], w[f][bad][0])
            continue
        bad = ~((g == w) | ((g != g) & (w != w)))
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("%s: %s differs in %d places; first at %s: gpu %r reference %r"
                                 % (what, k, bad.sum(), at, g[at], w[at]))


def gml_packed(name):
    """The first render of a fixture program, converted (one per process)."""
    if name not in _gml:
        from go_raytracer_amd import gml
        rendered, _ = gml.run_file(os.path.join(GML, name + ".gml"))
        _gml[name] = rt.scene.convert(rendered[0][0])
    return _gml[name]


# 1. every scene kind x camera model x sample count equals the reference
@pytest.mark.parametrize("S", [1, 4, 7])
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("name", SCENES)
def test_buffers_equal_the_reference(ctx, name, model, S):
    p = T.packed(name)
    cam = camera(samples=S, size=(W, H), **MODELS[model])
    ref = AR.reference(name, p, cam)
    cov = ref["coverage"]
    assert (cov == 0.0).any() and (cov > 0.0).any()
    if S == 7:  # (tests/test_aov_ref.py: every pair has empty, partial and full pixels at 7 samples)
        assert (cov == 1.0).any() and ((cov > 0.0) & (cov < 1.0)).any()
    if name == "closure":
        assert ref["closure"] > 0
    if name == "c4csg":  # sample 0 of some pixel hits a composite: ids then names the leaf's kind
        top = ref["ids"]["object"]
        assert any(p.scene.objects[int(i)].kind == abi.RT_CSG for i in top[top >= 0])
        assert (ref["ids"]["kind"] != abi.RT_CSG).all()
    ctx.set_scene(p)
    assert_buffers_equal(ctx.render_camera_aov(cam), ref, "%s %s S=%d" % (name, model, S))


# 2. a posed camera
@pytest.mark.parametrize("model", ["pinhole", "thinlens"])
def test_posed_oblique_camera(ctx, model):
    p = T.packed("c3")
    cam = camera(samples=4, size=(W, H), **MODELS[model], **OBLIQUE)
    ref = AR.reference("c3", p, cam)
    plain = AR.reference("c3", p, camera(samples=4, size=(W, H), **MODELS[model]))
    assert not np.array_equal(ref["depth"], plain["depth"])  # the pose matters
    assert (ref["coverage"] > 0.0).sum() >= 20
    ctx.set_scene(p)
    assert_buffers_equal(ctx.render_camera_aov(cam), ref, "posed " + model)


# 3. closure surfaces with u, v formulas of their own: a sphere, a cylinder's side
@pytest.mark.parametrize("name,kind", [("sphere", abi.RT_SPHERE), ("cylinder", abi.RT_CYLINDER)])
def test_closure_surfaces_on_a_sphere_and_a_cylinders_side(ctx, name, kind):
    p = gml_packed(name)
    assert p.scene.num_programs > 0
    cam = camera(samples=3, size=(26, 19))
    ref = AR.reference("gml-" + name, p, cam)
    ids = ref["ids"]
    on = (ids["kind"] == kind) & (ids["material"] < 0) & (ids["face"] == 0)
    assert on.sum() >= 10, on.sum()
    assert len(np.unique(ref["albedo"][on], axis=0)) >= 2  # the program's colour varies over the surface
    ctx.set_scene(p)
    assert_buffers_equal(ctx.render_camera_aov(cam), ref, name + ".gml")


# 4. bands
def test_a_band_equals_the_frames_rows(ctx):
    p = T.packed("c4csg")
    cam = camera(samples=4, size=(31, 45), **MODELS["thinlens"])
    ref = AR.reference("c4csg", p, cam, 17, 43)
    assert (ref["coverage"] == 0.0).any() and (ref["coverage"] == 1.0).any()
    ctx.set_scene(p)
    frame = ctx.render_camera_aov(cam)
    band = ctx.render_camera_aov(cam, 17, 43)
    assert band["depth"].shape == (26, 31)
    assert_buffers_equal(band, {k: frame[k][17:43] for k in AR.NAMES}, "band vs frame")
    assert_buffers_equal(band, ref, "band vs reference")


def test_a_one_row_band_of_13_pixels(ctx):
    p = T.packed("c3")
    cam = camera(samples=7, size=(W, H), **MODELS["pinhole"])
    ref = AR.reference("c3", p, cam)
    y = int(np.argmax(((ref["coverage"] > 0.0) & (ref["coverage"] < 1.0)).sum(axis=1)))
    assert ((ref["coverage"][y] > 0.0) & (ref["coverage"][y] < 1.0)).any()
    ctx.set_scene(p)
    band = ctx.render_camera_aov(cam, y, y + 1)
    assert band["ids"].shape == (1, W)
    assert_buffers_equal(band, {k: ref[k][y:y + 1] for k in AR.NAMES}, "row %d" % y)


# 5. the outputs are independent of each other and leave the rest of a buffer alone
def test_each_output_alone_gives_the_bytes_it_gives_with_all_five(ctx):
    import torch
    p = T.packed("closure")
    cam = camera(samples=4, size=(W, H), **MODELS["thinlens"])
    ref = AR.reference("closure", p, cam)
    assert ref["closure"] > 0
    ctx.set_scene(p)
    every = ctx.render_camera_aov(cam)
    assert_buffers_equal(every, ref, "all five")
    for k in AR.NAMES:
        one = ctx.render_camera_aov(cam, which=(k,))
        assert list(one) == [k] and one[k].tobytes() == every[k].tobytes(), k
    d = torch.full((H, W), -7.0, dtype=torch.float64, device="cuda:0")
    ctx.render_camera_aov_async(cam, 3, 9, depth=d[3:9])
    torch.cuda.synchronize()
    d = d.cpu().numpy()
    assert d[3:9].tobytes() == every["depth"][3:9].tobytes() and (d[:3] == -7.0).all() and (d[9:] == -7.0).all()


# 6. accel independence
@pytest.mark.parametrize("name", ["glass22", "c4csg"])
def test_accel_settings_give_identical_bytes(name):
    p = T.packed(name)
    cam = camera(samples=3, size=(W, H), **MODELS["thinlens"])
    ref = AR.reference(name, p, cam)
    assert (ref["coverage"] > 0.0).sum() >= 20
    c = rt.RenderContext(0)
    try:
        res = []
        for flags in (0, abi.RT_ACCEL_CULL, abi.RT_ACCEL_BVH, abi.RT_ACCEL_BVH | abi.RT_ACCEL_CULL):
            c.set_accel(flags)
            c.set_scene(p)
            if name == "glass22":
                assert bool(c.scene_info() & abi.RT_INFO_BVH) == bool(flags & abi.RT_ACCEL_BVH)
            got = c.render_camera_aov(cam)
            res.append(b"".join(got[k].tobytes() for k in AR.NAMES))
        assert_buffers_equal(got, ref, name)
        for r in res[1:]:
            assert r == res[0]
    finally:
        c.close()


# 7. the materialised route: the camera's rays written out, the closest-hit query, ordered sums in Python
@pytest.mark.parametrize("name", ["c3", "c4csg"])
def test_buffers_equal_the_materialised_route(ctx, name):
    import torch
    p = T.packed(name)
    S = 5
    cam = camera(samples=S, size=(W, H), **MODELS["thinlens"], **OBLIQUE)
    ctx.set_scene(p)
    rays = ctx.camera_rays_ex(cam)
    dev = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    out = torch.empty(rays.size * abi.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    ctx.query_closest_async(dev, out)
    torch.cuda.synchronize()
    hits = out.cpu().numpy().view(abi.HIT_DTYPE).reshape(rays.shape)
    hit = hits["object"] >= 0
    assert hit.any() and (~hit).any() and (hits["material"][hit] >= 0).all()
    want = {"depth": np.zeros((H, W)), "normal": np.zeros((H, W, 3)), "albedo": np.zeros((H, W, 3)),
            "coverage": np.zeros((H, W)), "ids": np.zeros((H, W), dtype=abi.AOV_IDS_DTYPE)}
    inv = 1.0 / float(S)
    mats = p.scene.materials
    for y in range(H):
        for x in range(W):
            zt, N, A, h = 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0
            for s in range(S):
                r = hits[y, x, s]
                if r["object"] < 0:
                    continue
                zt = zt + float(r["t"])
                N = T.v_add(N, T.v_norm(tuple(float(v) for v in r["normal_world"])))
                A = T.v_add(A, tuple(mats[int(r["material"])].color[:]))
                h += 1
            want["coverage"][y, x] = float(h) * inv
            want["normal"][y, x] = T.v_scale(N, inv)
            want["albedo"][y, x] = T.v_scale(A, inv)
            want["depth"][y, x] = zt / float(h) if h > 0 else T.INF
            r0 = hits[y, x, 0]
            want["ids"][y, x] = (r0["object"], r0["face"], r0["kind"], r0["material"])
    part = (want["coverage"] > 0.0) & (want["coverage"] < 1.0)
    assert part.any()
    assert_buffers_equal(ctx.render_camera_aov(cam), want, name + " vs the materialised route")


# 8. errors name the function and leave the context usable
def test_errors_leave_the_context_usable():
    import torch
    lib = rt.load_library()
    c = rt.RenderContext(0)
    buf = torch.empty(24 * 16 * 16 + 64, dtype=torch.uint8, device="cuda:0")
    bp = buf.data_ptr()
    assert bp % 16 == 0

    def call(cam, out, y0=0, y1=16):
        return lib.rt_render_camera_aov_async(c.handle, None if cam is None else C.byref(cam), y0, y1,
                                              None if out is None else C.byref(out), None)

    def invalid(cam, out, y0=0, y1=16, text=None):
        assert call(cam, out, y0, y1) == abi.RT_E_INVALID
        m = lib.rt_last_error()
        assert b"rt_render_camera_aov_async" in m and (text is None or text in m), m

    def outs(**kw):
        o = abi.rt_aov_out()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    try:
        good = outs(depth=bp)
        invalid(None, good, text=b"no scene")
        p = T.packed("c2")  # 24 x 16
        c.set_scene(p)
        want = c.render()
        st0 = c.read_stats(reset=True)
        # what camera renders reject
        invalid(camera(model=4), good, text=b"model")
        invalid(camera(samples=-1), good, text=b"samples")
        invalid(camera(samples=abi.RT_CAMERA_MAX_SAMPLES + 1), good, text=b"samples")
        invalid(camera(size=(1, 16)), good, 0, 1)
        invalid(camera(depth=-1), good, text=b"depth")
        invalid(camera(depth=abi.RT_RADIANCE_MAX_DEPTH + 1), good, text=b"depth")
        invalid(camera(chunk_pixels=-1), good, text=b"chunk_pixels")
        for y0, y1 in ((0, 0), (7, 3), (-1, 4), (0, 17)):
            invalid(camera(), good, y0, y1, text=b"rows")
        invalid(camera(model="ortho", extent=0.0), good, text=b"extent")
        invalid(camera(model="thinlens", aperture=0.1, focus=0.0), good, text=b"focus")
        invalid(camera(eye=(1.0, 2.0, 3.0), look_at=(1.0, 2.0, 3.0)), good, text=b"look_at")
        # the outputs
        invalid(camera(), None, text=b"NULL rt_aov_out")
        invalid(None, outs(), text=b"NULL")
        for k in ("depth", "normal", "albedo", "coverage"):
            invalid(camera(), outs(**{k: bp + 4}), text=b"aligned")
        invalid(camera(), outs(ids=bp + 8), text=b"16-byte aligned")
        invalid(camera(), outs(depth=bp, ids=bp + 4), text=b"aligned")
        # the context still works: a valid call equals the reference, renders and counters are untouched
        cam = camera(samples=3)
        ref = AR.reference("c2", p, cam)
        assert (ref["coverage"] > 0.0).any() and (ref["coverage"] == 0.0).any()
        assert_buffers_equal(c.render_camera_aov(cam), ref, "after the errors")
        assert np.array_equal(c.render(), want)
        assert c.read_stats(reset=True).as_dict() == st0.as_dict()
    finally:
        c.close()


# 9. no side effects on renders and their counters
def test_feature_buffers_leave_the_context_alone():
    p = rt.scene.convert(rt.configs.c3cone(64, 48))
    ref, ost = oracle_bind.render_rows(p)
    cam = camera(samples=5, size=(W, H), **MODELS["thinlens"], **OBLIQUE)
    c = rt.RenderContext(0)
    try:
        c.set_scene(p)
        c.read_stats(reset=True)
        state0 = (c.specialized()[0], c.tile_order_info()[0], c.scene_info())
        before = c.render()
        got = c.render_camera_aov(cam)
        st = c.read_stats(reset=True)
        assert (c.specialized()[0], c.tile_order_info()[0], c.scene_info()) == state0
        after = c.render()
        st1 = c.read_stats(reset=True)
    finally:
        c.close()
    assert (got["coverage"] > 0.0).any()
    assert np.array_equal(before, ref) and np.array_equal(after, ref)
    assert st.as_dict() == ost.as_dict() and st1.as_dict() == ost.as_dict()  # one render's counters each, nothing more


# 10. the CLI writes the buffers, their views and the denoised frame
def test_cli_writes_feature_buffers_and_the_denoised_frame(ctx, tmp_path):
    from go_raytracer_amd import cli, gml
    path = os.path.join(GML, "checked-cube.gml")
    a = cli.build_parser().parse_args(["--samples", "3", "--size", "13x23", "--aov", "depth,albedo,ids", "--denoise",
                                       "--denoise-iterations", "2", path])
    cam, dn = cli.camera_from_args(a), cli.denoise_from_args(a)
    written = cli.render_program(path, str(tmp_path), camera=cam, aov=cli.aov_from_args(a), denoise=dn)
    img = written[0]
    stem, ext = os.path.splitext(img)
    assert written[1:] == [img + ".depth.npy", img + ".depth.png", img + ".albedo.npy", img + ".albedo.png",
                           img + ".ids.npy", stem + ".denoised" + ext]
    ctx.set_scene(gml.run_file(path)[0][0][0])
    want = ctx.render_camera_aov(cam)
    assert (want["ids"]["material"] < 0).any()  # closure surfaces
    for k in ("depth", "albedo", "ids"):
        assert np.load(img + "." + k + ".npy").tobytes() == want[k].tobytes(), k
    assert np.array_equal(rt.imageio.read_image(img + ".depth.png")[..., :3], cli.aov_view("depth", want["depth"]))
    rgba, mean = ctx.render_camera(cam, mean=True)
    assert np.array_equal(rt.imageio.read_image(img)[..., :3], rgba[..., :3])
    _, den = ctx.denoise(mean, want["normal"], want["depth"], want["albedo"], dn, rgba=True)
    assert np.array_equal(rt.imageio.read_image(stem + ".denoised" + ext)[..., :3], den[..., :3])
