"""Reference for the feature buffers (include/rt_abi.h rt_aov_out,
rt_render_camera_aov_async): the header's "Feature buffers" semantics restated
in Python floats -- test infrastructure.

The rays are camera_ref.rays', the search is trace_ref.closest_hit, the normal
and the material colour (closure surfaces through the interpreter) are
trace_ref.surface_props', and the accumulators below keep the header's order,
so buffers() can be compared with `==`. Nothing here calls the library under
test.
"""
import numpy as np

import go_raytracer_amd as rt
import camera_ref as CR
import trace_ref as T

abi = rt.abi
NAMES = ("depth", "normal", "albedo", "coverage", "ids")
_cache = {}


def sample(sc, o, d):
    """None for a miss, else (t, unit normal, colour, (object, face, kind,
    material), closure?) of the ray's closest hit."""
    hit = T.closest_hit(sc, o, d)
    if hit is None:
        return None
    i, t, _, face = hit
    _, nw, mat = T.surface_props(sc, hit)
    ob = sc.packed.scene.objects[i]
    lf = face
    if ob.kind == abi.RT_CSG:  # the surface is the leaf's
        ob = sc.packed.scene.csg_leaves[ob.csg_first + (face >> 4)]
        lf = face & 7
    mi = int(ob.material[lf])
    return t, T.v_norm(nw), tuple(float(c) for c in mat.color), (i, face, int(ob.kind), mi), mi < 0


def buffers(packed, cam=None, y0=0, y1=None):
    """The five buffers of rows [y0, y1) as a dict of numpy arrays (ids an
    abi.AOV_IDS_DTYPE array), plus "closure": the closure-surface samples met."""
    sc = T.scene_of(packed)
    rays = CR.rays(packed, cam, y0, y1)
    rows, W, S = rays.shape
    out = {"depth": np.zeros((rows, W)), "normal": np.zeros((rows, W, 3)), "albedo": np.zeros((rows, W, 3)),
           "coverage": np.zeros((rows, W)), "ids": np.zeros((rows, W), dtype=abi.AOV_IDS_DTYPE), "closure": 0}
    inv = 1.0 / float(S)
    for y in range(rows):
        for x in range(W):
            zt, N, A, h = 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0
            ids = (-1, 0, 0, 0)
            for s in range(S):
                r = rays[y, x, s]
                got = sample(sc, tuple(float(v) for v in r["origin"]), tuple(float(v) for v in r["dir"]))
                if got is None:
                    continue
                t, n, a, i4, closure = got
                zt = zt + t
                N = T.v_add(N, n)
                A = T.v_add(A, a)
                h += 1
                out["closure"] += 1 if closure else 0
                if s == 0:
                    ids = i4
            out["coverage"][y, x] = float(h) * inv
            out["normal"][y, x] = T.v_scale(N, inv)
            out["albedo"][y, x] = T.v_scale(A, inv)
            out["depth"][y, x] = zt / float(h) if h > 0 else T.INF
            out["ids"][y, x] = ids
    return out


def cam_key(cam):
    return None if cam is None else bytes(cam)


def reference(name, packed, cam, y0=0, y1=None):
    """buffers() computed once per process and shared (never modified)."""
    k = (name, cam_key(cam), y0, y1)
    if k not in _cache:
        _cache[k] = buffers(packed, cam, y0, y1)
    return _cache[k]


def same(a, b):
    """a == b elementwise, or both NaN (the edge-ray tests' NaN contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.names:
        return all(np.array_equal(a[k], b[k]) for k in a.dtype.names)
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))
