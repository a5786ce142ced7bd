"""The variance of camera renders (rt_render_camera_var_async,
rt_render_camera_adaptive_var_async) and the variance-guided a-trous filter
(rt_denoise_atrous_var_async) on the device against tests/variance_ref.py
(needs an MI355X).

Bar: every output double equals the reference's (==, or both NaN), every byte
and count too. Each test first asserts, from the reference's side alone, what
it is about. The thin-lens case uses S = 7: no S among 3, 5, 6, 7 produces a
negative estimate on these c3 frames (tests/test_variance_ref.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

import go_raytracer_amd as rt
import adaptive_ref as AR
import denoise_ref as DR
import trace_ref as T
import variance_ref as VR

abi = rt.abi
pytestmark = pytest.mark.gpu

GML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gml")
THIN = dict(model="thinlens", size=(24, 16), aperture=0.35, focus=4.5)
FIXED = {
    "c3-zero-13x23-S4": ("c3", dict(samples=4, size=(13, 23))),
    "c3-thinlens-24x16-S7-chunks": ("c3", dict(samples=7, chunk_pixels=100, **THIN)),
    "closure-S2": ("closure", dict(samples=2, size=(13, 23))),
}
SIG = dict(sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.25)
TERMS = {"all": tuple(SIG), "color": ("sigma_color",), "none": ()}
FRAMES = {"37x29": (37, 29, (11, 17), (20, 30)), "70x9": (70, 9, (4, 33), (6, 60))}  # W, H, the NaN, the +inf pixel
_frames = {}
_refs = {}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = ~((got == want) | ((got != got) & (want != want)))
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: differs in %d places; first at %s: gpu %r reference %r"
                             % (what, bad.sum(), at, got[at], want[at]))


# 1. fixed renders
@pytest.mark.parametrize("case", list(FIXED))
def test_fixed_render_variance_equals_the_reference(ctx, case):
    name, kw = FIXED[case]
    cam = rt.RenderContext.camera(**kw)
    rad = AR.radiance(name, cam)
    want = VR.resolve_var(rad)
    assert (want > 0.0).any() and (want == 0.0).any() and not (want < 0.0).any()
    ctx.set_scene(T.packed(name))
    if "chunk_pixels" in kw:
        assert ctx.render_camera_chunks(cam) == 4 and cam.width % 100 != 0  # chunks do not align to rows
    wimg, wmean = ctx.render_camera(cam, mean=True)
    img, mean, var = ctx.render_camera(cam, mean=True, var=True)
    assert_same(var, want, case)
    assert np.array_equal(img, wimg) and mean.tobytes() == wmean.tobytes()
    img2, var2 = ctx.render_camera(cam, var=True)
    assert np.array_equal(img2, wimg) and var2.tobytes() == var.tobytes()


def test_var_alone_and_inside_a_larger_buffer(ctx):
    import torch
    cam = rt.RenderContext.camera(**FIXED["c3-zero-13x23-S4"][1])
    want = VR.resolve_var(AR.radiance("c3", cam))
    ctx.set_scene(T.packed("c3"))
    n = 13 * 23 * 3
    big = torch.full((n + 64,), -7.0, dtype=torch.float64, device="cuda:0")
    ctx.render_camera_async(cam, 0, 23, var=big[5:5 + n].view(23, 13, 3))  # rgba and mean NULL
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert_same(got[5:5 + n].reshape(23, 13, 3), want, "d_var alone, at an offset")
    assert (got[:5] == -7.0).all() and (got[5 + n:] == -7.0).all()
    # a band: rows [7, 21) cross the 20-row strip boundary
    band = torch.full((14, 13, 3), -7.0, dtype=torch.float64, device="cuda:0")
    ctx.render_camera_async(cam, 7, 21, var=band)
    torch.cuda.synchronize()
    assert_same(band.cpu().numpy(), want[7:21], "rows 7..21")


# 2. adaptive renders
@pytest.mark.parametrize("case", [("c3", 16, 2, 0.005), ("c4csg", 16, 2, 0.005)], ids=lambda c: "%s-%d-%d" % c[:3])
def test_adaptive_render_variance_equals_the_reference(ctx, case):
    name, S, n0, tol = case
    cam = rt.RenderContext.camera(samples=S, size=(13, 23))
    rad = AR.radiance(name, cam)
    wimg, wmean, wcount = AR.resolve(rad, tol, n0)
    assert AR.histogram(wcount) == AR.HISTOGRAMS[case] and len(AR.HISTOGRAMS[case]) == 4
    want = VR.resolve_var(rad, wcount)  # at the reference's own counts
    assert (want > 0.0).any() and (want == 0.0).any()
    assert not np.array_equal(want, VR.resolve_var(rad))  # not the cap's variance
    ctx.set_scene(T.packed(name))
    ad = rt.RenderContext.adaptive(tol, n0)
    old = ctx.render_camera_adaptive(cam, ad, mean=True, samples=True)
    img, mean, count, var = ctx.render_camera_adaptive(cam, ad, mean=True, samples=True, var=True)
    assert_same(var, want, "%s %d/%d/%g" % case)
    assert np.array_equal(count, wcount) and np.array_equal(count, old[2])
    assert mean.tobytes() == old[1].tobytes() == wmean.tobytes()
    assert np.array_equal(img, old[0]) and np.array_equal(img, wimg)


# 3. the filter
def frame(key):
    """(colour, variance with a zero region, one NaN and one +inf pixel, normal, depth, albedo) of FRAMES[key],
    shared and never modified."""
    if key not in _frames:
        W, H, nan_at, inf_at = FRAMES[key]
        _, noisy, normal, depth, albedo = DR.test_frame(W, H)
        rng = np.random.RandomState(7)
        var = 0.15 * 0.15 * rng.uniform(0.5, 1.5, (H, W, 3))
        var[:, :W // 4] = 0.0
        var[nan_at] = np.nan
        var[inf_at + (1,)] = np.inf
        _frames[key] = (noisy, var, normal, depth, albedo)
    return _frames[key]


def reference(key, terms, K):
    k = (key, terms, K)
    if k not in _refs:
        color, var, normal, depth, albedo = frame(key)
        _refs[k] = VR.atrous_var(color, var, normal, depth, albedo, K, **{t: SIG[t] for t in TERMS[terms]})
    return _refs[k]


def params(terms, K):
    s = {t: SIG[t] for t in TERMS[terms]}
    return rt.RenderContext.denoise_params(K, s.get("sigma_color", 0.0), s.get("sigma_normal", 0.0),
                                           s.get("sigma_depth", 0.0), s.get("sigma_albedo", 0.0))


@pytest.mark.parametrize("K", [1, 2, 5, 8])  # K = 1 and 2 run the tile kernels only; K >= 3 the global one too
@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("key", list(FRAMES))
def test_filter_output_equals_the_reference(ctx, key, terms, K):
    import torch
    color, var, normal, depth, albedo = frame(key)
    W, H, nan_at, inf_at = FRAMES[key]
    assert (var == 0.0).sum() >= 3 * H and np.isnan(var).sum() == 3 and np.isposinf(var).sum() == 1
    assert np.isfinite(color).all()
    want, wvar = reference(key, terms, K)
    assert not np.array_equal(want[H - 1, W - 1], color[H - 1, W - 1])  # the filter did something
    assert np.isfinite(want).all() and np.isnan(wvar[nan_at]) and not np.isfinite(wvar[inf_at])  # (inf, or NaN by then)
    assert np.isfinite(wvar).sum() > W * H // 3 or (terms == "none" and K >= 5)  # the wide steps spread the NaN
    if "sigma_color" in TERMS[terms]:
        assert np.array_equal(want[nan_at], color[nan_at])  # a NaN g: the pixel passes through
        # zero variance shuts all but the centre tap: (w * c) / w per iteration, the identity to a rounding each
        assert (np.abs(want[:, 0] - color[:, 0]) <= K * 2.0 ** -52 * np.abs(color[:, 0])).all()
        assert (wvar[:, 0] == 0.0).all()
    dev = "cuda:0"
    guides = {"normal": normal, "depth": depth, "albedo": albedo}
    on = {g: torch.from_numpy(a).to(dev) for g, a in guides.items() if "sigma_" + g in TERMS[terms]}  # others: NULL
    col, v = torch.from_numpy(color).to(dev), torch.from_numpy(var).to(dev)
    out = torch.full((H, W, 3), -7.0, dtype=torch.float64, device=dev)
    tmp = torch.empty((H, W, 3), dtype=torch.float64, device=dev) if K > 1 else None  # NULL at K = 1
    vo = torch.full((H, W), -7.0, dtype=torch.float64, device=dev)
    vt = torch.empty((H, W), dtype=torch.float64, device=dev)
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    ctx.denoise_async(params(terms, K), col, out, tmp, rgba=rgba, var=v, var_out=vo, var_tmp=vt, **on)
    torch.cuda.synchronize()
    what = "%s %s K=%d" % (key, terms, K)
    assert_same(out.cpu().numpy(), want, what)
    assert_same(vo.cpu().numpy(), wvar, what + " variance")
    assert np.array_equal(rgba.cpu().numpy(), DR.quantised(want))
    assert col.cpu().numpy().tobytes() == color.tobytes() and v.cpu().numpy().tobytes() == var.tobytes()
    for g, t in on.items():
        assert t.cpu().numpy().tobytes() == guides[g].tobytes(), g


def test_filter_errors_leave_the_context_usable(ctx):
    import torch
    lib = rt.load_library()
    color, var, normal, depth, albedo = frame("37x29")
    W, H = FRAMES["37x29"][:2]
    n = W * H * 3
    dev = "cuda:0"
    col, v = torch.from_numpy(color).to(dev), torch.from_numpy(var).to(dev)
    gn, gz, ga = (torch.from_numpy(a).to(dev) for a in (normal, depth, albedo))
    big = torch.empty(3 * n + 8, dtype=torch.float64, device=dev)
    out, tmp, vo, vt = big[:n], big[n:2 * n], big[2 * n:2 * n + W * H], big[2 * n + W * H:2 * n + 2 * W * H]
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(dn, w=W, h=H, color=col, var=v, normal=gn, depth=gz, albedo=ga, out=out, tmp=tmp, vo=vo, vt=vt,
             rgba=None):
        raw = lambda t: t if isinstance(t, C.c_void_p) else P(t)  # noqa: E731
        return lib.rt_denoise_atrous_var_async(ctx.handle, None if dn is None else C.byref(dn), w, h, P(color),
                                               raw(var), P(normal), P(depth), P(albedo), P(out), P(tmp), raw(vo),
                                               raw(vt), rgba, None)

    def invalid(text, dn, **kw):
        assert call(dn, **kw) == abi.RT_E_INVALID
        m = lib.rt_last_error()
        assert b"rt_denoise_atrous_var_async" in m and text in m, m

    good = params("all", 5)
    # the plain call's errors
    invalid(b"NULL rt_denoise", None)
    bad = params("all", 5)
    bad.reserved = 1
    invalid(b"reserved", bad)
    for k in (-1, 9):
        invalid(b"iterations", params("all", k))
    bad = params("all", 5)
    bad.sigma_color = float("nan")
    invalid(b"sigma", bad)
    invalid(b"width", good, w=0)
    invalid(b"NULL", good, color=None)
    invalid(b"NULL", good, out=None)
    invalid(b"d_tmp", good, tmp=None)
    invalid(b"guide", good, depth=None)
    invalid(b"overlap", good, tmp=out)
    invalid(b"aligned", good, rgba=C.c_void_p(big.data_ptr() + 2))
    # ... plus its own
    for name in ("var", "vo", "vt"):
        invalid(b"NULL d_var", good, **{name: None})
    invalid(b"8-byte aligned", good, var=C.c_void_p(v.data_ptr() + 4))
    invalid(b"8-byte aligned", good, vo=C.c_void_p(vo.data_ptr() + 4))
    invalid(b"8-byte aligned", good, vt=C.c_void_p(vt.data_ptr() + 4))
    invalid(b"overlap", good, var=col)
    invalid(b"overlap", good, vo=vt)
    invalid(b"overlap", good, vt=big[2 * n + W * H - 1:2 * n + 2 * W * H - 1])  # one double into d_var_out
    invalid(b"overlap", good, vo=big[n - 1:n - 1 + W * H])                      # the last double of d_out
    invalid(b"overlap", good, vt=v[H - 1, W - 1])                               # the last pixel of d_var
    invalid(b"overlap", params("all", 1), tmp=None, vo=col[0, 0])
    # d_tmp may be NULL at K = 1, +inf is off, and the context still filters
    off = rt.RenderContext.denoise_params(1, 2.0, float("inf"), 0.0, 0.25)
    assert call(off, normal=None, depth=None, tmp=None) == abi.RT_OK
    torch.cuda.synchronize()
    want, wvar = VR.atrous_var(color, var, None, None, albedo, 1, sigma_color=2.0, sigma_albedo=0.25)
    assert_same(out.cpu().numpy().reshape(H, W, 3), want, "after the errors")
    assert_same(vo.cpu().numpy().reshape(H, W), wvar, "after the errors: variance")
    assert col.cpu().numpy().tobytes() == color.tobytes() and v.cpu().numpy().tobytes() == var.tobytes()


def test_render_errors_leave_the_context_usable(ctx):
    import torch
    lib = rt.load_library()
    ctx.set_scene(T.packed("c3"))
    dev = "cuda:0"
    buf = torch.zeros(13 * 23 * 3 + 8, dtype=torch.float64, device=dev)
    p = C.c_void_p(buf.data_ptr())
    odd = C.c_void_p(buf.data_ptr() + 4)
    cam = rt.RenderContext.camera(samples=4, size=(13, 23))
    one = rt.RenderContext.camera(samples=1, size=(13, 23))
    ad = rt.RenderContext.adaptive(0.005, 2)

    def fixed(c, rgba, mean, var):
        return lib.rt_render_camera_var_async(ctx.handle, C.byref(c), 0, 23, rgba, mean, var, None)

    def adaptive(c, rgba, mean, samples, var):
        return lib.rt_render_camera_adaptive_var_async(ctx.handle, C.byref(c), C.byref(ad), 0, 23, rgba, mean, samples,
                                                       var, None)

    def said(text, who):
        m = lib.rt_last_error()
        assert who in m and text in m, m

    assert fixed(cam, None, None, None) == abi.RT_E_INVALID
    said(b"all NULL", b"rt_render_camera_var_async")
    assert fixed(cam, None, None, odd) == abi.RT_E_INVALID
    said(b"d_var must be 8-byte aligned", b"rt_render_camera_var_async")
    assert fixed(one, None, None, p) == abi.RT_E_INVALID  # samples == 1: no estimate
    said(b"at least 2 samples", b"rt_render_camera_var_async")
    assert adaptive(cam, None, None, None, None) == abi.RT_E_INVALID
    said(b"all NULL", b"rt_render_camera_adaptive_var_async")
    assert adaptive(cam, None, None, None, odd) == abi.RT_E_INVALID
    said(b"d_var must be 8-byte aligned", b"rt_render_camera_adaptive_var_async")
    with pytest.raises(RuntimeError, match="at least 2 samples"):
        ctx.render_camera(one, var=True)
    img = ctx.render_camera(one)  # ... while one sample without a variance still renders
    assert img.shape == (23, 13, 4)
    # the context still renders, through the new call with d_var NULL too
    want = ctx.render_camera(cam, mean=True)
    mean = torch.empty((23, 13, 3), dtype=torch.float64, device=dev)
    assert fixed(cam, None, C.c_void_p(mean.data_ptr()), None) == abi.RT_OK
    torch.cuda.synchronize()
    assert mean.cpu().numpy().tobytes() == want[1].tobytes()
    var = ctx.render_camera(cam, var=True)[1]
    assert_same(var, VR.resolve_var(AR.radiance("c3", cam)), "after the errors")


# 4. end to end: render with variance, the feature buffers, the filter
@pytest.mark.parametrize("name", ["closure", "c3"])
def test_end_to_end_on_a_thin_lens_render(ctx, name):
    cam = rt.RenderContext.camera(samples=4, **THIN)
    rad = AR.radiance(name, cam)
    wvar = VR.resolve_var(rad)
    ctx.set_scene(T.packed(name))
    wimg, wmean = ctx.render_camera(cam, mean=True)
    img, mean, var = ctx.render_camera(cam, mean=True, var=True)
    assert_same(var, wvar, name)
    assert mean.tobytes() == wmean.tobytes() and (var > 0.0).any()
    bufs = ctx.render_camera_aov(cam)
    wide = dict(sigma_color=4.0, sigma_normal=1.0, sigma_depth=4.0, sigma_albedo=0.8)
    dn = rt.RenderContext.denoise_params(3, *wide.values())
    want, wsk = VR.atrous_var(mean, wvar, bufs["normal"], bufs["depth"], bufs["albedo"], 3, **wide)
    assert np.isfinite(want).all() and (want != mean).any()
    got, dimg, sk = ctx.denoise(mean, bufs["normal"], bufs["depth"], bufs["albedo"], dn, rgba=True, var=var,
                                variance_out=True)
    assert_same(got, want, name)
    assert_same(sk, wsk, name + " variance")
    assert np.array_equal(dimg, DR.quantised(want))
    # `params` None: the defaults of the mode
    d = rt.render.DENOISE_DEFAULTS
    auto = ctx.denoise(mean, bufs["normal"], bufs["depth"], bufs["albedo"], var=var)
    want5, _ = VR.atrous_var(mean, wvar, bufs["normal"], bufs["depth"], bufs["albedo"], 5,
                             sigma_color=rt.render.DENOISE_VAR_COLOR, sigma_normal=d["normal"],
                             sigma_depth=d["depth"], sigma_albedo=d["albedo"])
    assert_same(auto, want5, name + " defaults")


# 5. the CLI writes the variance map and the variance-guided frame
def test_cli_writes_the_variance_map_and_the_denoised_frame(ctx, tmp_path):
    from go_raytracer_amd import cli, gml
    path = os.path.join(GML, "checked-cube.gml")
    vmap = str(tmp_path / "variance.npy")
    a = cli.build_parser().parse_args(["--samples", "3", "--size", "13x23", "--denoise", "--denoise-variance",
                                       "--denoise-iterations", "2", "--variance-map", vmap, path])
    cam, dn = cli.camera_from_args(a), cli.denoise_from_args(a)
    assert dn.sigma_color == rt.render.DENOISE_VAR_COLOR
    written = cli.render_program(path, str(tmp_path), camera=cam, denoise=dn, denoise_variance=a.denoise_variance,
                                 variance_map=a.variance_map)
    img = written[0]
    stem, ext = os.path.splitext(img)
    assert written[1:] == [vmap, stem + ".denoised" + ext]
    ctx.set_scene(gml.run_file(path)[0][0][0])
    rgba, mean, var = ctx.render_camera(cam, mean=True, var=True)
    got = np.load(vmap)
    assert got.dtype == np.float64 and got.shape == (23, 13, 3) and got.tobytes() == var.tobytes()
    assert (var > 0.0).any()
    assert np.array_equal(rt.imageio.read_image(img)[..., :3], rgba[..., :3])
    bufs = ctx.render_camera_aov(cam, which=("normal", "depth", "albedo"))
    _, den = ctx.denoise(mean, bufs["normal"], bufs["depth"], bufs["albedo"], dn, rgba=True, var=var)
    assert np.array_equal(rt.imageio.read_image(stem + ".denoised" + ext)[..., :3], den[..., :3])
