"""Reference for the variance of a camera render's mean and for the
variance-guided a-trous filter (include/rt_abi.h "Variance of a camera render",
"Variance-guided a-trous filter"): the header's two rules restated in Python
floats -- test infrastructure.

Python floats are IEEE doubles with one rounding per operation and every
expression below keeps the header's order, so resolve_var() and atrous_var()
compare with `==`. Nothing here calls the library under test.
"""
import numpy as np

import denoise_ref as DR
import trace_ref as T

EPS = 1e-10  # RT_DENOISE_VAR_EPS
PRE = (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)


def pixel_var(samples):
    """(var_c, e_c) per channel of one pixel's colour samples (a sequence of
    float triples, n >= 2, in sample order): the clamped variance of the mean
    and the estimate before the clamp."""
    n = len(samples)
    assert n >= 2
    total = [float(v) for v in samples[0]]
    sq = [v * v for v in total]
    for s in range(1, n):
        c = [float(v) for v in samples[s]]
        for k in range(3):
            total[k] = total[k] + c[k]
            sq[k] = sq[k] + (c[k] * c[k])
    inv = 1.0 / float(n)
    var, est = [], []
    for k in range(3):
        m = total[k] * inv
        v = sq[k] - total[k] * m
        e = v / float(n * (n - 1))
        est.append(e)
        var.append(0.0 if e < 0.0 else e)
    return var, est


def resolve_var(rad, counts=None, estimates=False):
    """float64 [rows, W, 3] variance of the mean of [rows, W, S] radiance
    records (adaptive_ref.radiance): over all S samples, or over the first
    counts[y, x] samples of each pixel (an adaptive render's sample counts).
    estimates=True: e_c before the clamp instead."""
    rows, W, S = rad.shape
    out = np.zeros((rows, W, 3), dtype=np.float64)
    col = rad["color"]
    for y in range(rows):
        for x in range(W):
            n = S if counts is None else int(counts[y, x])
            var, est = pixel_var(col[y, x, :n])
            out[y, x] = est if estimates else var
    return out


def reduce_var(var):
    """S_0 as nested lists: (var.0 + var.1) + var.2 per pixel."""
    return [[(float(v[0]) + float(v[1])) + float(v[2]) for v in row] for row in np.asarray(var, dtype=np.float64)]


def iteration_var(I, Sv, W, H, step, kc2, n, inn, z, iz, a, ia):
    """One iteration: (I_(i+1), S_(i+1)) of (I_i, S_i); the colour term is on
    when kc2 is not None, a guide's when its constant is not None."""
    out = [[None] * W for _ in range(H)]
    vout = [[None] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            cp = I[y][x]
            icv = None
            if kc2 is not None:
                N = D = 0.0
                for dy in range(-1, 2):
                    qy = y + dy
                    if qy < 0 or qy >= H:
                        continue
                    for dx in range(-1, 2):
                        qx = x + dx
                        if qx < 0 or qx >= W:
                            continue
                        N = N + (PRE[dy + 1] * PRE[dx + 1]) * Sv[qy][qx]
                        D = D + PRE[dy + 1] * PRE[dx + 1]
                g = T._div(N, D)
                icv = T._div(1.0, kc2 * g + EPS)
            s0 = s1 = s2 = 0.0
            wsum = vs = 0.0
            for dy in range(-2, 3):
                qy = y + dy * step
                if qy < 0 or qy >= H:
                    continue
                for dx in range(-2, 3):
                    qx = x + dx * step
                    if qx < 0 or qx >= W:
                        continue
                    w = DR.TAPS[dy + 2] * DR.TAPS[dx + 2]
                    cq = I[qy][qx]
                    if icv is not None:
                        w = w * DR.kern(DR.dist2(cp, cq) * icv)
                    if inn is not None:
                        w = w * DR.kern(DR.dist2(n[y][x], n[qy][qx]) * inn)
                    if iz is not None:
                        zp, zq = z[y][x], z[qy][qx]
                        w = w * DR.kern((0.0 if zp == zq else (zp - zq) * (zp - zq)) * iz)
                    if ia is not None:
                        w = w * DR.kern(DR.dist2(a[y][x], a[qy][qx]) * ia)
                    if w > 0.0:
                        s0 = s0 + w * cq[0]
                        s1 = s1 + w * cq[1]
                        s2 = s2 + w * cq[2]
                        wsum = wsum + w
                        vs = vs + (w * w) * Sv[qy][qx]
            if wsum > 0.0:
                out[y][x] = (T._div(s0, wsum), T._div(s1, wsum), T._div(s2, wsum))
                vout[y][x] = T._div(vs, wsum * wsum)
            else:
                out[y][x] = cp
                vout[y][x] = Sv[y][x]
    return out, vout


def atrous_var(color, var, normal=None, depth=None, albedo=None, iterations=0, sigma_color=0.0, sigma_normal=0.0,
               sigma_depth=0.0, sigma_albedo=0.0):
    """(I_K float64 [H, W, 3], S_K float64 [H, W]) of the frame `color` with
    the per-channel variance `var` of its pixels; sigma_color in standard
    deviations."""
    K = iterations or 5
    assert 1 <= K <= 8
    color = np.asarray(color, dtype=np.float64)
    H, W = color.shape[:2]
    onc, onn, onz, ona = (DR.is_on(sigma_color), DR.is_on(sigma_normal), DR.is_on(sigma_depth),
                          DR.is_on(sigma_albedo))
    kc2 = sigma_color * sigma_color if onc else None
    inn = 1.0 / (sigma_normal * sigma_normal) if onn else None
    iz = 1.0 / (sigma_depth * sigma_depth) if onz else None
    ia = 1.0 / (sigma_albedo * sigma_albedo) if ona else None
    n, z, a = (DR._lists(normal if onn else None, 3), DR._lists(depth if onz else None, 1),
               DR._lists(albedo if ona else None, 3))
    I = DR._lists(color, 3)
    Sv = reduce_var(var)
    for i in range(K):
        I, Sv = iteration_var(I, Sv, W, H, 1 << i, kc2, n, inn, z, iz, a, ia)
    return np.array(I, dtype=np.float64).reshape(H, W, 3), np.array(Sv, dtype=np.float64).reshape(H, W)


def hetero_frame(W=64, H=48, seed=11, samples=4, quiet=0.01, loud=0.25):
    """A synthetic heteroscedastic frame: a smooth ramp whose middle third of
    the rows carries per-sample noise of sigma `loud`, the rest `quiet`.
    -> (clean [H, W, 3], mean of `samples` noisy samples, the samples' variance
    of that mean as resolve_var's rule forms it, vectorised)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    clean = np.stack([0.2 + 0.6 * xx / (W - 1.0), 0.8 - 0.5 * yy / (H - 1.0), np.full((H, W), 0.4)], axis=-1)
    sig = np.where((yy >= H // 3) & (yy < 2 * H // 3), loud, quiet)[..., None, None]
    smp = clean[..., None] + rng.normal(0.0, 1.0, (H, W, 3, samples)) * sig
    mean = smp.mean(axis=-1)
    var = smp.var(axis=-1, ddof=1) / samples
    return clean, mean, var
