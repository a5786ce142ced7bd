"""Reference for the adaptive camera renders (include/rt_abi.h rt_adaptive,
rt_render_camera_adaptive_async): the header's schedule, per-pixel state and
stopping rule restated in Python floats -- test infrastructure.

Python floats are IEEE doubles with one rounding per operation and every
expression keeps the header's order, so resolve() compares with `==`. The
input is the per-sample radiance of the fixed render at the cap, [rows, W, S]
(camera_ref.rays traced by trace_ref or by a radiance query): sample s of an
adaptive render is sample s of that render. Nothing here calls the library.
"""
import numpy as np

import camera_ref as CR
import trace_ref as T

# (scene of trace_ref, cap, min_samples, tolerance) -> {samples: pixels}: the zero camera resized to 13 x 23,
# measured with trace_ref on the CPU
HISTOGRAMS = {
    ("c3", 16, 2, 0.005): {2: 196, 4: 31, 8: 26, 16: 46},
    ("c3", 20, 3, 0.005): {3: 209, 6: 24, 12: 21, 20: 45},
    ("c4csg", 16, 2, 0.005): {2: 197, 4: 19, 8: 26, 16: 57},
    ("c4csg", 20, 3, 0.005): {3: 198, 6: 17, 12: 25, 20: 59},
    ("glass21", 20, 3, 0.02): {3: 278, 6: 10, 12: 3, 20: 8},
    ("glass22", 20, 3, 0.02): {3: 274, 6: 10, 12: 3, 20: 12},
    ("closure", 16, 2, 0.005): {2: 293, 16: 6},
}
_radiance = {}


def radiance(name, cam):
    """Per-sample radiance [H, W, S] of camera `cam` on trace_ref scene `name`,
    on the CPU: camera_ref.rays traced by trace_ref at the camera's depth
    (cached per process, never modified)."""
    key = (name, bytes(cam))
    if key not in _radiance:
        p = T.packed(name)
        rays = CR.rays(p, cam)
        flat = rays.reshape(-1)
        rad = T.trace_many(p, flat["origin"], flat["dir"], int(cam.depth)).reshape(rays.shape)
        rad.setflags(write=False)
        _radiance[key] = rad
    return _radiance[key]


def schedule(S, min_samples=0):
    """[n_0, ..., n_K]: the samples of an active pixel after each pass."""
    n = min(4, S) if min_samples == 0 else min_samples
    assert 2 <= n <= S
    out = [n]
    while n != S:
        n = min(2 * n, S)
        out.append(n)
    return out


def converged(total, sq, n, tol2):
    inv = 1.0 / float(n)
    for c in range(3):
        m = total[c] * inv
        v = sq[c] - total[c] * m
        e = v / float(n * (n - 1))
        if not e <= tol2:
            return False
    return True


def resolve(rad, tolerance, min_samples=0):
    """(bytes uint8 [rows, W, 4], mean float64 [rows, W, 3], samples int32
    [rows, W]) of [rows, W, S] radiance records under the rule."""
    rows, W, S = rad.shape
    ns = schedule(S, min_samples)
    tol2 = float(tolerance) * float(tolerance)
    img = np.zeros((rows, W, 4), dtype=np.uint8)
    img[..., 3] = 255
    mean = np.zeros((rows, W, 3), dtype=np.float64)
    count = np.zeros((rows, W), dtype=np.int32)
    col = rad["color"]
    for y in range(rows):
        for x in range(W):
            c0 = [float(v) for v in col[y, x, 0]]
            total = list(c0)
            sq = [v * v for v in c0]
            s = 1
            for n in ns:
                while s < n:
                    c = [float(v) for v in col[y, x, s]]
                    for k in range(3):
                        total[k] = total[k] + c[k]
                        sq[k] = sq[k] + (c[k] * c[k])
                    s += 1
                if n == S or converged(total, sq, n, tol2):
                    break
            inv = 1.0 / float(n)
            m = [total[k] * inv for k in range(3)]
            mean[y, x] = m
            img[y, x, :3] = [T.quantise(m[0]), T.quantise(m[1]), T.quantise(m[2])]
            count[y, x] = n
    return img, mean, count


def histogram(count):
    """{samples: pixels}"""
    v, n = np.unique(count, return_counts=True)
    return {int(a): int(b) for a, b in zip(v, n)}
