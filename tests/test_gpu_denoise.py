"""The guided a-trous filter (rt_denoise_atrous_async) on the device against
tests/denoise_ref.py (needs an MI355X).

Bar: every output double equals the reference's (==, or both NaN). Frames:
37 x 29 (1073 pixels: no multiple of 64, more than one workgroup) and 70 x 9
(wider than a wave, fewer rows than the taps span). The guides have a
discontinuity, a +inf-depth region and the colour one NaN pixel. Each test
first asserts, from the reference's side alone, what it is about.
"""
import ctypes as C

import numpy as np
import pytest

import go_raytracer_amd as rt
import denoise_ref as DR
import trace_ref as T

abi = rt.abi
pytestmark = pytest.mark.gpu

SIG = dict(sigma_color=0.6, sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.25)
TERMS = {"all": tuple(SIG), "color": ("sigma_color",), "normal": ("sigma_normal",), "depth": ("sigma_depth",),
         "albedo": ("sigma_albedo",), "none": ()}
FRAMES = {"37x29": (37, 29, (11, 17)), "70x9": (70, 9, (4, 33))}
_frames = {}
_refs = {}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


def frame(key):
    """(colour with one NaN pixel, normal, depth, albedo) of FRAMES[key], shared and never modified."""
    if key not in _frames:
        W, H, nan_at = FRAMES[key]
        _, noisy, normal, depth, albedo = DR.test_frame(W, H)
        noisy[nan_at] = np.nan
        _frames[key] = (noisy, normal, depth, albedo)
    return _frames[key]


def reference(key, terms, K):
    k = (key, terms, K)
    if k not in _refs:
        color, normal, depth, albedo = frame(key)
        _refs[k] = DR.atrous(color, normal, depth, albedo, K, **{t: SIG[t] for t in TERMS[terms]})
    return _refs[k]


def params(terms, K):
    s = {t: SIG[t] for t in TERMS[terms]}
    return rt.RenderContext.denoise_params(K, s.get("sigma_color", 0.0), s.get("sigma_normal", 0.0),
                                           s.get("sigma_depth", 0.0), s.get("sigma_albedo", 0.0))


def assert_same(got, want, what):
    assert got.shape == want.shape, what
    bad = ~((got == want) | ((got != got) & (want != want)))
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: differs in %d places; first at %s: gpu %r reference %r"
                             % (what, bad.sum(), at, got[at], want[at]))


@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("key", list(FRAMES))
def test_output_equals_the_reference(ctx, key, terms, K):
    import torch
    color, normal, depth, albedo = frame(key)
    W, H, nan_at = FRAMES[key]
    # the frame: a guide discontinuity, a +inf-depth region, one NaN colour
    assert np.isposinf(depth).any() and np.isfinite(depth).any() and len(np.unique(normal.reshape(-1, 3), axis=0)) == 3
    assert np.isnan(color).sum() == 3 and np.isnan(color[nan_at]).all()
    want = reference(key, terms, K)
    assert not np.array_equal(want[0, 0], color[0, 0])  # the filter did something
    if "sigma_color" in TERMS[terms]:
        nan = np.isnan(want)
        assert nan[nan_at].all() and nan.sum() == 3  # the NaN stays where it is
    dev = "cuda:0"
    guides = {"normal": normal, "depth": depth, "albedo": albedo}
    on = {g: torch.from_numpy(a).to(dev) for g, a in guides.items() if "sigma_" + g in TERMS[terms]}  # others: NULL
    col = torch.from_numpy(color).to(dev)
    out = torch.full((H, W, 3), -7.0, dtype=torch.float64, device=dev)
    tmp = torch.empty((H, W, 3), dtype=torch.float64, device=dev) if K > 1 else None  # NULL at K = 1
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    ctx.denoise_async(params(terms, K), col, out, tmp, rgba=rgba, **on)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), want, "%s %s K=%d" % (key, terms, K))
    assert col.cpu().numpy().tobytes() == color.tobytes()  # d_color is never written
    assert np.array_equal(rgba.cpu().numpy(), DR.quantised(want))


def test_default_iterations_are_five(ctx):
    color, normal, depth, albedo = frame("37x29")
    want = reference("37x29", "all", 5)
    assert not np.array_equal(np.nan_to_num(want), np.nan_to_num(reference("37x29", "all", 2)))
    got, img = ctx.denoise(color, normal, depth, albedo, params("all", 0), rgba=True)
    assert_same(got, want, "iterations = 0")
    assert np.array_equal(img, DR.quantised(want))


def test_errors_leave_the_context_usable(ctx):
    import torch
    lib = rt.load_library()
    color, normal, depth, albedo = frame("37x29")
    W, H, _ = FRAMES["37x29"]
    n = W * H * 3
    dev = "cuda:0"
    col = torch.from_numpy(color).to(dev)
    gn, gz, ga = (torch.from_numpy(a).to(dev) for a in (normal, depth, albedo))
    big = torch.empty(3 * n + 8, dtype=torch.float64, device=dev)
    out, tmp = big[:n], big[n:2 * n]
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(dn, w=W, h=H, color=col, normal=gn, depth=gz, albedo=ga, out=out, tmp=tmp, rgba=None):
        return lib.rt_denoise_atrous_async(ctx.handle, None if dn is None else C.byref(dn), w, h, P(color), P(normal),
                                           P(depth), P(albedo), P(out), P(tmp), rgba, None)

    def invalid(text, dn, **kw):
        assert call(dn, **kw) == abi.RT_E_INVALID
        m = lib.rt_last_error()
        assert b"rt_denoise_atrous_async" in m and text in m, m

    good = params("all", 5)
    invalid(b"NULL rt_denoise", None)
    bad = params("all", 5)
    bad.reserved = 1
    invalid(b"reserved", bad)
    for k in (-1, 9):
        invalid(b"iterations", params("all", k))
    for field in ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"):
        for v in (-0.5, float("nan"), -float("inf")):
            bad = params("all", 5)
            setattr(bad, field, v)
            invalid(b"sigma", bad)
    for w, h in ((0, H), (W, 0), (-1, -1), (65536, 65536)):
        invalid(b"width", good, w=w, h=h)
    invalid(b"NULL", good, color=None)
    invalid(b"NULL", good, out=None)
    invalid(b"d_tmp", good, tmp=None)
    for g in ("normal", "depth", "albedo"):
        invalid(b"guide", good, **{g: None})
    # overlap of the byte ranges of d_color, d_out and d_tmp
    invalid(b"overlap", good, out=col)
    invalid(b"overlap", good, tmp=col)
    invalid(b"overlap", good, tmp=out)
    invalid(b"overlap", good, tmp=big[n - 1:2 * n - 1])  # one double into d_out
    invalid(b"overlap", params("all", 1), out=col, tmp=None)
    invalid(b"aligned", good, rgba=C.c_void_p(big.data_ptr() + 2))
    # what is off needs no guide, +inf is off, and the context still filters
    off = rt.RenderContext.denoise_params(2, 0.6, float("inf"), 0.0, 0.25)
    assert call(off, normal=None, depth=None) == abi.RT_OK
    torch.cuda.synchronize()
    want = DR.atrous(color, None, None, albedo, 2, sigma_color=0.6, sigma_albedo=0.25)
    assert_same(out.cpu().numpy().reshape(H, W, 3), want, "after the errors")
    assert col.cpu().numpy().tobytes() == color.tobytes()


@pytest.mark.parametrize("name", ["closure", "c3"])
def test_end_to_end_on_a_thin_lens_render(ctx, name):
    p = T.packed(name)
    cam = rt.RenderContext.camera(model="thinlens", samples=4, size=(24, 16), aperture=0.35, focus=4.5)
    ctx.set_scene(p)
    _, mean = ctx.render_camera(cam, mean=True)
    bufs = ctx.render_camera_aov(cam)
    assert np.isposinf(bufs["depth"]).any() and np.isfinite(bufs["depth"]).any()
    # wide sigmas: the closure frame is piecewise constant (9 colours, each with an albedo of its own), so
    # under SIG no tap crosses an edge there and the filter is the identity
    wide = dict(sigma_color=1.5, sigma_normal=1.0, sigma_depth=4.0, sigma_albedo=0.8)
    dn = rt.RenderContext.denoise_params(3, *wide.values())
    want = DR.atrous(mean, bufs["normal"], bufs["depth"], bufs["albedo"], 3, **wide)
    assert np.isfinite(want).all() and (want != mean).any()
    got, img = ctx.denoise(mean, bufs["normal"], bufs["depth"], bufs["albedo"], dn, rgba=True)
    assert_same(got, want, name)
    assert np.array_equal(img, DR.quantised(want))
