"""Adaptive camera renders (rt_render_camera_adaptive_async,
rt_render_camera_adaptive_plan) on the device against tests/adaptive_ref.py
(needs an MI355X).

Bar: bytes. rgba, mean and the sample counts equal adaptive_ref over the
per-sample radiance of the fixed render at the cap (camera_ref.rays traced by
trace_ref on the CPU), compared with `==`. The frame is 13 x 23 unless stated:
it crosses the 20-row strip boundary and 299 pixels are no multiple of 64.
Each test first asserts, from the reference's side alone, that its inputs
spread the pixels over the pass levels: at least three distinct final counts
with at least 3 pixels each, min_samples and the cap among them.
"""
import ctypes as C
import math

import numpy as np
import pytest

import go_raytracer_amd as rt
import adaptive_ref as AR
import camera_ref as CR
import trace_ref as T

abi = rt.abi
pytestmark = pytest.mark.gpu

RB = abi.RADIANCE_DTYPE.itemsize
W, H = 13, 23
OBLIQUE = dict(eye=(2.5, 1.75, -3.0), look_at=(0.25, -0.25, 6.0), up=(0.3, 1.0, -0.2))


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


def camera(**kw):
    kw.setdefault("size", (W, H))
    return rt.RenderContext.camera(**kw)


def adaptive(tol, n0=0):
    return rt.RenderContext.adaptive(tol, n0)


def spread(count, n0, S, levels=3):
    """The histogram precondition, from reference counts alone."""
    h = AR.histogram(count)
    big = {n for n, k in h.items() if k >= 3}
    assert n0 in big and S in big and len(big) >= levels, h
    return h


def assert_equal(got, want, what):
    img, mean, count = got
    wimg, wmean, wcount = want
    assert count.dtype == np.int32 and count.shape == wcount.shape, what
    assert np.array_equal(count, wcount), "%s: %d counts differ: gpu %s reference %s" % (
        what, (count != wcount).sum(), AR.histogram(count), AR.histogram(wcount))
    assert mean.dtype == np.float64 and np.array_equal(mean, wmean), "%s: %d means differ" % (
        what, (mean != wmean).any(axis=2).sum())
    assert img.dtype == np.uint8 and np.array_equal(img, wimg), what
    assert (img[..., 3] == 255).all()


# 1. exactness on the recorded frames
@pytest.mark.parametrize("case", list(AR.HISTOGRAMS), ids=lambda c: "%s-%d-%d" % c[:3])
def test_adaptive_render_equals_the_reference(ctx, case):
    name, S, n0, tol = case
    cam = camera(samples=S)
    want = AR.resolve(AR.radiance(name, cam), tol, n0)
    assert spread(want[2], n0, S, 2 if name == "closure" else 3) == AR.HISTOGRAMS[case]
    p = T.packed(name)
    ctx.set_scene(p)
    assert bool(ctx.scene_info() & abi.RT_INFO_BVH) == (name == "glass22")
    assert bool(ctx.scene_info() & abi.RT_INFO_CSG) == (name == "c4csg")
    assert (p.scene.num_programs >= 1) == (name == "closure")
    if name == "glass21":
        assert p.scene.depth == 5
    got = ctx.render_camera_adaptive(cam, adaptive(tol, n0), mean=True, samples=True)
    assert_equal(got, want, "%s %d/%d/%g" % case)
    assert ctx.render_camera_adaptive_plan(cam, adaptive(tol, n0)) == (1, 4)


# 2. identity with the fixed render, and the infinite tolerance
@pytest.mark.parametrize("name", ["c3", "c4csg", "glass22", "closure"])
def test_min_samples_at_the_cap_is_the_fixed_render(ctx, name):
    ctx.set_scene(T.packed(name))
    cam = camera(samples=6, **OBLIQUE)
    wimg, wmean = ctx.render_camera(cam, mean=True)
    assert len(np.unique(wimg.reshape(-1, 4), axis=0)) >= (3 if name == "closure" else 20)
    for tol in (0.0, 0.005, math.inf):
        img, mean, count = ctx.render_camera_adaptive(cam, adaptive(tol, 6), mean=True, samples=True)
        assert (count == 6).all() and np.array_equal(mean, wmean) and np.array_equal(img, wimg)
    assert ctx.render_camera_adaptive_plan(cam, adaptive(0.005, 6)) == (1, 1)


def test_infinite_tolerance_stops_at_min_samples(ctx):
    cam = camera(samples=16)
    rad = AR.radiance("c3", cam)
    assert len(AR.histogram(AR.resolve(rad, 0.005, 2)[2])) == 4  # a finite tolerance does spread these pixels
    ctx.set_scene(T.packed("c3"))
    for n0 in (2, 5, 0):
        want = AR.resolve(rad, math.inf, n0)
        assert (want[2] == (n0 or 4)).all()
        assert_equal(ctx.render_camera_adaptive(cam, adaptive(math.inf, n0), mean=True, samples=True), want, "inf %d" % n0)


# 3. chunks and the plan
def test_chunk_sizes_give_identical_outputs(ctx):
    assert W % 7 != 0 and (W * H) % 7 != 0  # a chunk boundary falls inside a row; the last chunk is short
    want = AR.resolve(AR.radiance("c3", camera(samples=16)), 0.005, 2)
    spread(want[2], 2, 16)
    ctx.set_scene(T.packed("c3"))
    ad = adaptive(0.005, 2)
    for cp in (7, 64, 0):
        cam = camera(samples=16, chunk_pixels=cp)
        assert ctx.render_camera_adaptive_plan(cam, ad) == (1 if cp == 0 else -(-W * H // cp), 4)
        assert ctx.render_camera_adaptive_plan(cam, ad, 17, 23) == (1 if cp == 0 else -(-W * 6 // cp), 4)
        assert_equal(ctx.render_camera_adaptive(cam, ad, mean=True, samples=True), want, "chunk_pixels %d" % cp)
    assert ctx.render_camera_adaptive_plan(camera(samples=20), adaptive(0.005, 3)) == (1, 4)
    assert ctx.render_camera_adaptive_plan(camera(samples=1024, size=(2, 22)), adaptive(0.005, 2)) == (1, 10)
    assert ctx.render_camera_adaptive_plan(camera(samples=64), adaptive(0.005)) == (1, 5)  # 4, 8, 16, 32, 64
    # the chunk follows the largest batch: 2097152 / 32 pixels at 4 -> 64, and never more than 524288
    assert ctx.render_camera_adaptive_plan(camera(samples=64, size=(1920, 1080)), adaptive(0.005)) == (32, 5)
    assert ctx.render_camera_adaptive_plan(camera(samples=2, size=(1920, 1080)), adaptive(0.005)) == (4, 1)


# 4. bands
def test_bands_equal_the_frames_rows(ctx):
    ctx.set_scene(T.packed("c3"))
    cam = camera(samples=8, size=(31, 45))
    ad = adaptive(0.005, 2)
    want = AR.resolve(AR.radiance("c3", cam), 0.005, 2)
    spread(want[2], 2, 8)
    spread(want[2][17:23], 2, 8)
    full = ctx.render_camera_adaptive(cam, ad, mean=True, samples=True)
    assert_equal(full, want, "full frame")
    for y0, y1 in ((17, 23), (17, 43)):  # start mid-strip; the second crosses rows 20 and 40
        band = ctx.render_camera_adaptive(cam, ad, y0, y1, mean=True, samples=True)
        assert band[0].shape == (y1 - y0, 31, 4)
        assert_equal(band, tuple(a[y0:y1] for a in full), "band %d..%d" % (y0, y1))


# 5. the other camera models
MODEL_CASES = {
    "thinlens": dict(model="thinlens", aperture=0.35, focus=4.5),
    "equirect": dict(model="equirect"),
    "ortho": dict(model="ortho", extent=3.0),
    "oblique": dict(OBLIQUE),
    "thinlens-oblique": dict(model="thinlens", aperture=0.35, focus=4.5, **OBLIQUE),
}


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_other_camera_models_equal_the_reference(ctx, case):
    cam = camera(samples=12, **MODEL_CASES[case])
    assert CR.frame(T.packed("c3"), cam)[3] == (4 if "thinlens" in case else 2)
    want = AR.resolve(AR.radiance("c3", cam), 0.005, 3)
    spread(want[2], 3, 12)
    ctx.set_scene(T.packed("c3"))
    assert_equal(ctx.render_camera_adaptive(cam, adaptive(0.005, 3), mean=True, samples=True), want, case)


# 6. the longest schedule and the largest draw offsets
def test_cap_1024_from_2_samples(ctx):
    cam = camera(samples=1024, size=(2, 22))
    assert AR.schedule(1024, 2) == [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]
    want = AR.resolve(AR.radiance("c3", cam), 0.002, 2)
    h = spread(want[2], 2, 1024)
    assert len(h) >= 6 and (want[2][:20] == 1024).any() and (want[2][:20] == 2).any()
    ctx.set_scene(T.packed("c3"))
    assert ctx.render_camera_adaptive_plan(cam, adaptive(0.002, 2)) == (1, 10)
    assert_equal(ctx.render_camera_adaptive(cam, adaptive(0.002, 2), mean=True, samples=True), want, "s1024")


# 7. accel independence
def test_accel_settings_give_identical_bytes():
    case = ("glass22", 20, 3, 0.02)
    cam = camera(samples=20)
    want = AR.resolve(AR.radiance("glass22", cam), 0.02, 3)
    assert spread(want[2], 3, 20) == AR.HISTOGRAMS[case]
    c = rt.RenderContext(0)
    try:
        for flags in (0, abi.RT_ACCEL_CULL, abi.RT_ACCEL_BVH, abi.RT_ACCEL_BVH | abi.RT_ACCEL_CULL):
            c.set_accel(flags)
            c.set_scene(T.packed("glass22"))
            assert bool(c.scene_info() & abi.RT_INFO_BVH) == bool(flags & abi.RT_ACCEL_BVH)
            assert_equal(c.render_camera_adaptive(cam, adaptive(0.02, 3), mean=True, samples=True), want, "accel %d" % flags)
    finally:
        c.close()


# 8. output selection
def test_any_subset_of_the_outputs_and_the_rest_of_a_buffer(ctx):
    import torch
    cam = camera(samples=16)
    ad = adaptive(0.005, 2)
    want = AR.resolve(AR.radiance("c3", cam), 0.005, 2)
    spread(want[2], 2, 16)
    spread(want[2][3:9], 2, 16, 2)
    ctx.set_scene(T.packed("c3"))
    for pick in range(1, 8):
        rgba = torch.full((H, W, 4), 0xA5, dtype=torch.uint8, device="cuda:0") if pick & 1 else None
        mean = torch.full((H, W, 3), -7.0, dtype=torch.float64, device="cuda:0") if pick & 2 else None
        cnt = torch.full((H, W), -9, dtype=torch.int32, device="cuda:0") if pick & 4 else None
        ctx.render_camera_adaptive_async(cam, ad, 3, 9, None if rgba is None else rgba[3:9],
                                         None if mean is None else mean[3:9], None if cnt is None else cnt[3:9])
        torch.cuda.synchronize()
        for t, w, fill in ((rgba, want[0], 0xA5), (mean, want[1], -7.0), (cnt, want[2], -9)):
            if t is not None:
                a = t.cpu().numpy()
                assert np.array_equal(a[3:9], w[3:9]), pick
                assert (a[:3] == fill).all() and (a[9:] == fill).all(), pick
    assert np.array_equal(ctx.render_camera_adaptive(cam, ad), want[0])
    img, cnt = ctx.render_camera_adaptive(cam, ad, samples=True)
    assert np.array_equal(img, want[0]) and np.array_equal(cnt, want[2])
    img, mean = ctx.render_camera_adaptive(cam, ad, mean=True)
    assert np.array_equal(img, want[0]) and np.array_equal(mean, want[1])


# 9. no side effects on renders, their counters, specialisation, tile order, radiance queries and fixed camera renders
def test_adaptive_renders_leave_the_context_alone():
    import torch
    import oracle_bind
    p = rt.scene.convert(rt.configs.c3cone(64, 48))
    ref, ost = oracle_bind.render_rows(p)
    o, d = T.ray_set(256)
    rec = np.zeros(256, dtype=abi.RAY_DTYPE)
    rec["origin"], rec["dir"], rec["tmax"], rec["exclude"] = o, d, np.inf, -1
    cam = camera(samples=16, model="thinlens", aperture=0.35, focus=4.5, **OBLIQUE)
    crays = CR.rays(p, cam).reshape(-1)
    want = AR.resolve(T.trace_many(p, crays["origin"], crays["dir"], 0).reshape(H, W, 16), 0.005, 2)
    spread(want[2], 2, 16)
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
            fixed = [torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
            rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
            cnt = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
        side.synchronize()
        c.render_rows_async(0, 48, img[0], side)
        c.query_radiance_async(rays, out[0], 0, side)
        c.render_camera_async(cam, 0, H, rgba=fixed[0], stream=side)
        c.render_camera_adaptive_async(cam, adaptive(0.005, 2), 0, H, rgba=rgba, samples=cnt, stream=side)
        c.render_camera_async(cam, 0, H, rgba=fixed[1], stream=side)
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
    assert np.array_equal(plain, ref) and st1.as_dict() == ost.as_dict()
    two = {k: (2 * v if not isinstance(v, list) else [2 * x for x in v]) for k, v in ost.as_dict().items()}
    assert st.as_dict() == two  # two renders' counters, nothing from the camera renders
    assert out[0].cpu().numpy().tobytes() == out[1].cpu().numpy().tobytes()
    assert np.array_equal(fixed[0].cpu().numpy(), fixed[1].cpu().numpy())
    assert len(np.unique(fixed[0].cpu().numpy().reshape(-1, 4), axis=0)) >= 10
    assert np.array_equal(cnt.cpu().numpy(), want[2]) and np.array_equal(rgba.cpu().numpy(), want[0])
    capped = want[2] == 16
    assert np.array_equal(want[0][capped], fixed[0].cpu().numpy()[capped])


# 10. errors name the function and leave the context usable
def test_errors_leave_the_context_usable():
    import torch
    lib = rt.load_library()
    c = rt.RenderContext(0)
    buf = torch.empty(24 * 16 * 32 + 64, dtype=torch.uint8, device="cuda:0")
    bp = buf.data_ptr()
    assert bp % 16 == 0
    good = adaptive(0.005, 2)

    def invalid(cam, ad=good, y0=0, y1=16, rgba=bp, mean=bp, cnt=bp, text=None, plan=True):
        cref = None if cam is None else C.byref(cam)
        aref = None if ad is None else C.byref(ad)
        rc = lib.rt_render_camera_adaptive_async(c.handle, cref, aref, y0, y1, C.c_void_p(rgba), C.c_void_p(mean),
                                                 C.c_void_p(cnt), None)
        m = lib.rt_last_error()
        assert rc == abi.RT_E_INVALID and b"rt_render_camera_adaptive_async" in m and (text is None or text in m), (rc, m)
        if plan:
            n = C.c_int(-7)
            assert lib.rt_render_camera_adaptive_plan(c.handle, cref, aref, y0, y1, C.byref(n), C.byref(n)) \
                == abi.RT_E_INVALID
            m = lib.rt_last_error()
            assert b"rt_render_camera_adaptive_plan" in m and (text is None or text in m) and n.value == -7, m

    def cam16(**kw):
        kw.setdefault("samples", 16)
        return rt.RenderContext.camera(**kw)

    def bad(**kw):
        ad = adaptive(0.005, 2)
        for k, v in kw.items():
            setattr(ad, k, v)
        return ad

    try:
        invalid(cam16(), text=b"no scene")
        c.set_scene(T.packed("c2"))  # 24 x 16
        want = c.render()
        fixed = c.render_camera(cam16())
        # everything rt_render_camera_async rejects
        invalid(cam16(model=4), text=b"model")
        flg = cam16()
        flg.flags = 2
        invalid(flg, text=b"flag")
        invalid(cam16(samples=-1), text=b"samples")
        invalid(cam16(samples=abi.RT_CAMERA_MAX_SAMPLES + 1), text=b"samples")
        for size in ((1, 16), (24, 1), (0, 16), (65536, 65536)):
            invalid(cam16(size=size), y0=0, y1=1)
        invalid(cam16(depth=-1), text=b"depth")
        invalid(cam16(depth=abi.RT_RADIANCE_MAX_DEPTH + 1), text=b"depth")
        invalid(cam16(chunk_pixels=-1), text=b"chunk_pixels")
        for y0, y1 in ((0, 0), (7, 3), (-1, 4), (0, 17)):
            invalid(cam16(), y0=y0, y1=y1, text=b"rows")
        invalid(cam16(model="ortho", extent=0.0), text=b"extent")
        invalid(cam16(model="thinlens", aperture=0.1, focus=0.0), text=b"focus")
        invalid(cam16(model="thinlens", aperture=-0.1, focus=3.0), text=b"aperture")
        invalid(cam16(eye=(1.0, 2.0, 3.0), look_at=(1.0, 2.0, 3.0)), text=b"look_at")
        invalid(cam16(eye=(0.0, 0.0, -1.0), look_at=(0.0, 0.0, 0.0), up=(0.0, 0.0, 2.0)), text=b"up")
        # the record
        invalid(cam16(), None, text=b"NULL rt_adaptive")
        invalid(cam16(), bad(reserved=1), text=b"reserved")
        for n0 in (1, -2, 17, 1 << 30):
            invalid(cam16(), bad(min_samples=n0), text=b"min_samples")
        invalid(cam16(samples=3), bad(min_samples=4), text=b"min_samples")
        for tol in (-0.001, -math.inf, math.nan):
            invalid(cam16(), bad(tolerance=tol), text=b"tolerance")
        for n0 in (0, 1, 2):
            invalid(cam16(samples=1), bad(min_samples=n0), text=b"at least 2")
        # the outputs
        invalid(cam16(), rgba=None, mean=None, cnt=None, text=b"all NULL", plan=False)
        invalid(cam16(), rgba=bp + 2, text=b"aligned", plan=False)
        invalid(cam16(), mean=bp + 4, text=b"aligned", plan=False)
        invalid(cam16(), cnt=bp + 2, text=b"aligned", plan=False)
        # what is in range: the zero camera (4 samples) with the default first pass, tolerance 0 and +inf
        assert c.render_camera_adaptive_plan(None, adaptive(0.0)) == (1, 1)
        assert c.render_camera_adaptive_plan(cam16(samples=2), adaptive(math.inf)) == (1, 1)
        assert c.render_camera_adaptive_plan(cam16(samples=3), adaptive(0.0)) == (1, 1)
        assert c.render_camera_adaptive_plan(cam16(samples=3), adaptive(0.0, 2)) == (1, 2)
        # the context still renders: the fixed and the adaptive camera render, and Render()
        assert np.array_equal(c.render_camera(cam16()), fixed)
        img, cnt = c.render_camera_adaptive(cam16(), adaptive(0.0, 16), samples=True)
        assert np.array_equal(img, fixed) and (cnt == 16).all()
        assert np.array_equal(c.render_camera_adaptive(None, adaptive(0.0)), want)  # 4 of 4 samples: Render()
        assert np.array_equal(c.render(), want)
    finally:
        c.close()


# 11. the CLI
def test_cli_adaptive_flags_route_the_programs_render(ctx, tmp_path):
    import os
    from go_raytracer_amd import cli, gml
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gml", "checked-cube.gml")
    ap = cli.build_parser()
    smap = str(tmp_path / "counts.png")
    a = ap.parse_args(["--adaptive", "0.005", "--min-samples", "2", "--samples", "16", "--size", "13x23",
                       "--samples-map", smap, path])
    cam, ad = cli.camera_from_args(a), cli.adaptive_from_args(a)
    (tmp_path / "out").mkdir()
    written = cli.render_program(path, str(tmp_path / "out"), camera=cam, adaptive=ad, samples_map=a.samples_map)
    assert len(written) == 1
    ctx.set_scene(gml.run_file(path)[0][0][0])
    img, cnt = ctx.render_camera_adaptive(cam, ad, samples=True)
    assert cnt.min() == 2 and cnt.max() == 16 and len(np.unique(img.reshape(-1, 4), axis=0)) >= 3
    got = rt.imageio.read_image(written[0])
    assert got.shape[:2] == (23, 13) and np.array_equal(got, img[..., :3])
    grey = rt.imageio.read_image(smap)
    assert np.array_equal(grey, cli.samples_image(cnt, 16))
    # without --adaptive the frame is the fixed camera render's, as before
    (tmp_path / "fixed").mkdir()
    fixed = cli.render_program(path, str(tmp_path / "fixed"), camera=cam)
    assert np.array_equal(rt.imageio.read_image(fixed[0]), ctx.render_camera(cam)[..., :3])
