"""Reference for the a-trous filter (include/rt_abi.h rt_denoise,
rt_denoise_atrous_async): the header's rule restated in Python floats -- test
infrastructure.

Python floats are IEEE doubles with one rounding per operation and every
expression below keeps the header's order, so atrous() can be compared with
`==`. Nothing here calls the library under test.
"""
import numpy as np

import trace_ref as T

TAPS = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
INF = float("inf")


def is_on(sigma):
    """A sigma > 0 and finite turns its term on; 0 or +inf turns it off."""
    if sigma != sigma or sigma < 0.0:
        raise ValueError("a sigma is negative or NaN")
    return sigma > 0.0 and sigma != INF


def kern(x):
    return (1.0 - x) * (1.0 - x) if x < 1.0 else 0.0


def dist2(a, b):
    d0, d1, d2 = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (d0 * d0 + d1 * d1) + d2 * d2


def _lists(a, per):
    """A numpy frame as nested Python lists of floats / float triples."""
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    if per == 1:
        return [[float(v) for v in row] for row in a]
    return [[(float(v[0]), float(v[1]), float(v[2])) for v in row] for row in a]


def iteration(I, W, H, step, ic, n, inn, z, iz, a, ia):
    """One iteration: I_(i+1) of I_i (nested lists of triples); a term is on
    when its constant is not None."""
    out = [[None] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            cp = I[y][x]
            s0 = s1 = s2 = 0.0
            wsum = 0.0
            for dy in range(-2, 3):
                qy = y + dy * step
                if qy < 0 or qy >= H:
                    continue
                for dx in range(-2, 3):
                    qx = x + dx * step
                    if qx < 0 or qx >= W:
                        continue
                    w = TAPS[dy + 2] * TAPS[dx + 2]
                    cq = I[qy][qx]
                    if ic is not None:
                        w = w * kern(dist2(cp, cq) * ic)
                    if inn is not None:
                        w = w * kern(dist2(n[y][x], n[qy][qx]) * inn)
                    if iz is not None:
                        zp, zq = z[y][x], z[qy][qx]
                        w = w * kern((0.0 if zp == zq else (zp - zq) * (zp - zq)) * iz)
                    if ia is not None:
                        w = w * kern(dist2(a[y][x], a[qy][qx]) * ia)
                    if w > 0.0:
                        s0 = s0 + w * cq[0]
                        s1 = s1 + w * cq[1]
                        s2 = s2 + w * cq[2]
                        wsum = wsum + w
            out[y][x] = (T._div(s0, wsum), T._div(s1, wsum), T._div(s2, wsum)) if wsum > 0.0 else cp
    return out


def atrous(color, normal=None, depth=None, albedo=None, iterations=0, sigma_color=0.0, sigma_normal=0.0,
           sigma_depth=0.0, sigma_albedo=0.0):
    """I_K of the float64 [H, W, 3] frame `color` -> float64 [H, W, 3]."""
    K = iterations or 5
    assert 1 <= K <= 8
    color = np.asarray(color, dtype=np.float64)
    H, W = color.shape[:2]
    onc, onn, onz, ona = is_on(sigma_color), is_on(sigma_normal), is_on(sigma_depth), is_on(sigma_albedo)
    inn = 1.0 / (sigma_normal * sigma_normal) if onn else None
    iz = 1.0 / (sigma_depth * sigma_depth) if onz else None
    ia = 1.0 / (sigma_albedo * sigma_albedo) if ona else None
    n, z, a = _lists(normal if onn else None, 3), _lists(depth if onz else None, 1), _lists(albedo if ona else None, 3)
    I = _lists(color, 3)
    for i in range(K):
        ic = None
        if onc:
            s = sigma_color * 0.5 ** i
            ic = 1.0 / (s * s)
        I = iteration(I, W, H, 1 << i, ic, n, inn, z, iz, a, ia)
    return np.array(I, dtype=np.float64).reshape(H, W, 3)


def quantised(frame):
    """The frame's RGBA8 bytes as the camera renders quantise their mean."""
    H, W = frame.shape[:2]
    img = np.zeros((H, W, 4), dtype=np.uint8)
    img[..., 3] = 255
    for y in range(H):
        for x in range(W):
            img[y, x, :3] = [T.quantise(float(c)) for c in frame[y, x]]
    return img


def test_frame(W=37, H=29, seed=3, sigma=0.15):
    """A two-surface frame plus background with Gaussian noise: (clean, noisy,
    normal, depth, albedo). Left: a wall facing the camera; right: a tilted
    floor with a depth ramp; the top rows: background (depth +inf, zero normal
    and albedo)."""
    rng = np.random.RandomState(seed)
    clean = np.zeros((H, W, 3))
    normal = np.zeros((H, W, 3))
    depth = np.full((H, W), np.inf)
    albedo = np.zeros((H, W, 3))
    top = max(1, H // 5)
    for y in range(H):
        for x in range(W):
            if y < top:
                clean[y, x] = (0.1, 0.2, 0.5)
            elif x < W // 2:
                clean[y, x] = (0.8, 0.3, 0.2)
                normal[y, x] = (0.0, 0.0, -1.0)
                depth[y, x] = 4.0
                albedo[y, x] = (0.9, 0.4, 0.3)
            else:
                clean[y, x] = (0.2, 0.7, 0.3)
                normal[y, x] = (0.0, 0.8, -0.6)
                depth[y, x] = 6.0 + 0.05 * (y - top)
                albedo[y, x] = (0.3, 0.9, 0.4)
    noisy = clean + rng.normal(0.0, sigma, clean.shape)
    return clean, noisy, normal, depth, albedo


test_frame.__test__ = False  # (a fixture builder, not a test)
