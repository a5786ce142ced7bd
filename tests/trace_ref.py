"""Reference for the radiance queries (include/rt_abi.h rt_query_radiance_async,
rt_query_camera_rays_async): a Python restatement of oracle/rt_oracle.c
trace_ray, compute_lighting, in_shadow, refract, fresnel and the material
lookup of surface_props over the oracle's unit hooks -- test infrastructure.

Python floats are IEEE doubles with one rounding per operation, and every
expression below keeps the oracle's operation order, so trace() returns the
oracle's values bit for bit (tests/test_trace_ref.py pins that against
oracle_render_rows). Intersections, surface normals, Pow, Cos / Sin / Tan,
Acos / Atan2 and the PCG stream come from the oracle itself (oracle_intersect,
oracle_surface_normal, oracle_go_*, oracle_pcg_float64); closure surfaces go
through gml.eval_surface_fn as oracle_bind._install_surfaces does.
"""
import ctypes as C
import dataclasses
import math
import random

import numpy as np

import go_raytracer_amd as rt
import oracle_bind
import query_ref

S = rt.scene
abi = rt.abi
INF = float("inf")


# ---- vec.go, as rt_oracle.c restates it -------------------------------------
def v_add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def v_sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def v_mul(a, b):
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def v_dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def v_scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else float("nan")


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return float("nan")
    return math.copysign(INF, a) * math.copysign(1.0, b)


def v_len(v):
    return _sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def v_norm(v):
    m = _sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (_div(v[0], m), _div(v[1], m), _div(v[2], m))


def v_neg(v):
    return (-v[0], -v[1], -v[2])


def v_lerp(a, b, t):
    return (a[0] + (b[0] - a[0]) * t, a[1] + (b[1] - a[1]) * t, a[2] + (b[2] - a[2]) * t)


def go_max(x, y):
    if x == INF:
        return x
    if y == INF:
        return y
    if x != x or y != y:
        return float("nan")
    if x == 0 and x == y:
        return y if math.copysign(1.0, x) < 0 else x
    return x if x > y else y


def go_min(x, y):
    if x == -INF:
        return x
    if y == -INF:
        return y
    if x != x or y != y:
        return float("nan")
    if x == 0 and x == y:
        return x if math.copysign(1.0, x) < 0 else y
    return x if x < y else y


def clampd(lo, hi, x):
    return go_min(go_max(x, lo), hi)


def v_clamp(c):
    return (clampd(0.0, 1.0, c[0]), clampd(0.0, 1.0, c[1]), clampd(0.0, 1.0, c[2]))


# ---- the converted scene's shading data (convert_scene) ---------------------
@dataclasses.dataclass
class _Mat:
    color: tuple
    reflectivity: float
    fuzziness: float
    transparency: float
    refractive_index: float
    kd: float
    ks: float
    specular_exponent: float


_ZERO_MAT = _Mat((0.0, 0.0, 0.0), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


class _Scene:
    def __init__(self, p):
        lib = oracle_bind.lib()
        sc = p.scene
        self.packed = p
        self.addr = C.addressof(sc)
        self.nobj = int(sc.num_objects)
        self.depth = 3 if sc.depth <= 0 else int(sc.depth)
        self.width, self.height = int(sc.width), int(sc.height)
        fov = 90.0 if sc.fov <= 0.0 else float(sc.fov)
        fovr = fov * math.pi / 180.0
        self.vw = 2.0 / lib.oracle_go_tan(fovr / 2.0)
        self.vh = self.vw * (float(self.height) / float(self.width))
        self.ambient = tuple(sc.ambient[:])
        self.bg0, self.bg1 = tuple(sc.bg_start[:]), tuple(sc.bg_end[:])
        self.exp_mode = int(sc.exp_mode)
        self.mats = []
        for i in range(int(sc.num_materials)):
            m = sc.materials[i]
            self.mats.append(_Mat(tuple(m.color[:]), m.reflectivity, m.fuzziness, m.transparency,
                                  m.refractive_index, m.kd, m.ks, m.specular_exponent))
        # lights: (kind, position, colour, direction, cos(cutoff), exponent)
        self.lights = []
        if sc.num_ext_lights > 0:
            for i in range(int(sc.num_ext_lights)):
                l = sc.ext_lights[i]
                pos, col, d = tuple(l.position[:]), tuple(l.color[:]), tuple(l.direction[:])
                ldir, lcos, lexp = (0.0, 0.0, 0.0), 0.0, 0.0
                if l.kind == abi.RT_LIGHT_DIRECTIONAL:
                    ldir = v_norm(v_neg(d))
                if l.kind == abi.RT_LIGHT_SPOT:
                    ldir = v_norm(v_sub(d, pos))
                    lcos = lib.oracle_go_cos(l.cutoff * 0.017453292519943295)
                    lexp = l.exponent
                self.lights.append((int(l.kind), pos, col, ldir, lcos, lexp))
        else:
            for i in range(int(sc.num_lights)):
                l = sc.lights[i]
                self.lights.append((abi.RT_LIGHT_POINT, tuple(l.position[:]), tuple(l.color[:]), (0.0, 0.0, 0.0),
                                    0.0, 0.0))
        # closure surfaces, as oracle_bind._install_surfaces evaluates them
        self.sfs = self.state = None
        if p.programs:
            from go_raytracer_amd import gml
            self.sfs = p.programs[3]
            self.state = p.programs[4].clone() if p.programs[4] is not None else gml.EvalState()


_scenes = {}


def scene_of(p):
    if id(p) not in _scenes:
        _scenes[id(p)] = _Scene(p)
    return _scenes[id(p)]


_t, _pt, _f = C.c_double(), (C.c_double * 3)(), C.c_int()
_nw, _pw = (C.c_double * 3)(), (C.c_double * 3)()


def _intersect(sc, i, o, d):
    ok = oracle_bind.lib().oracle_intersect(sc.addr, i, (C.c_double * 3)(*o), (C.c_double * 3)(*d), C.byref(_t), _pt,
                                            C.byref(_f))
    assert ok in (0, 1), ok
    return (_t.value, tuple(_pt[:]), _f.value) if ok == 1 else None


def closest_hit(sc, o, d, tmax=INF, exclude=-1):
    """closestHit (raytracer.go:469-483) with the query's tmax and exclude."""
    best = None
    for i in range(sc.nobj):
        if i == exclude:
            continue
        h = _intersect(sc, i, o, d)
        if h is None or not h[0] < tmax:
            continue
        if best is None or h[0] < best[1]:
            best = (i, h[0], h[1], h[2])
    return best


def surface_props(sc, hit):
    """(pw, nw, material) of surface_props: the normal and world point from
    oracle_surface_normal, the material from the face's entry or its program."""
    lib = oracle_bind.lib()
    i, _, p, face = hit
    rc = lib.oracle_surface_normal(sc.addr, i, face, (C.c_double * 3)(*p), _nw, _pw)
    assert rc == 0, rc
    pw, nw = tuple(_pw[:]), tuple(_nw[:])
    o = sc.packed.scene.objects[i]
    if o.kind == abi.RT_CSG:  # the surface is the leaf's
        o = sc.packed.scene.csg_leaves[o.csg_first + (face >> 4)]
        face &= 7
    mi = o.material[face]
    if mi >= 0:
        return pw, nw, sc.mats[mi]
    # closure surface: u, v as ComputeSurfaceProps computes them
    u = v = 0.0
    bad = False
    if o.kind == abi.RT_SPHERE:
        bad = abs(p[1]) > 1
        v = (p[1] + 1.0) / 2.0
        if not bad:
            u = lib.oracle_go_acos(_div(p[2], _sqrt(1.0 - p[1] * p[1]))) / (2.0 * math.pi)
    elif o.kind in (abi.RT_PLANE, abi.RT_CUBE):
        u, v = p[0], p[2]
    elif face == 0:
        u = (lib.oracle_go_atan2(p[0], p[2]) + math.pi) / (2.0 * math.pi)
        v = p[1]
    else:
        u, v = p[0], p[2]
    vface = 0 if o.kind == abi.RT_PLANE else face
    if bad:
        return pw, nw, _ZERO_MAT
    from go_raytracer_amd import gml
    try:
        m = gml.eval_surface_fn(vface, u, v, sc.state, sc.sfs[-mi - 1])
    except gml.GMLError:
        return pw, nw, _ZERO_MAT
    return pw, nw, _Mat(tuple(float(c) for c in m.color), float(m.reflectivity), float(m.fuzziness),
                        float(m.transparency), float(m.refractive_index), float(m.kd), float(m.ks),
                        float(m.specular_exponent))


def in_shadow(sc, hit_obj, pw, nw, ldir, dist, rdir):
    so = v_add(pw, v_scale(nw, 1e-4))
    for i in range(sc.nobj):
        if i == hit_obj:
            continue
        h = _intersect(sc, i, so, ldir)
        if h is None:
            continue
        if h[0] * v_len(rdir) < dist:
            return True
    return False


def compute_lighting(sc, hit_obj, pw, nw, mat, rdir):
    lib = oracle_bind.lib()
    V = v_neg(rdir)
    result = v_scale(sc.ambient, mat.kd)
    for kind, lpos, lcol, ldirc, lcos, lexp in sc.lights:
        if kind == abi.RT_LIGHT_DIRECTIONAL:
            ldir, dist = ldirc, INF
        else:
            lth = v_sub(lpos, pw)
            dist = v_len(lth)
            ldir = v_norm(lth)
        if kind == abi.RT_LIGHT_SPOT:
            ca = v_dot(v_neg(ldir), ldirc)
            lcol = v_scale(lcol, lib.oracle_go_pow_mode(ca, lexp, sc.exp_mode) if ca >= lcos else 0.0)
        if in_shadow(sc, hit_obj, pw, nw, ldir, dist, rdir):
            continue
        ndl = go_max(0.0, v_dot(nw, ldir))
        diffuse = v_scale(lcol, ndl * mat.kd)
        H = v_norm(v_add(V, ldir))
        spec = go_max(0.0, v_dot(nw, H))
        specular = v_scale(lcol, mat.ks * lib.oracle_go_pow_mode(spec, mat.specular_exponent, sc.exp_mode))
        result = v_add(v_add(result, diffuse), specular)
    return result


def refract(inc, n, n1, n2):
    ratio = n1 / n2
    cosI = -v_dot(n, inc)
    sinT2 = ratio * ratio * (1.0 - cosI * cosI)
    if sinT2 > 1.0:
        return (0.0, 0.0, 0.0)
    cosT = _sqrt(1.0 - sinT2)
    return v_add(v_scale(inc, ratio), v_scale(n, ratio * cosI - cosT))


def fresnel(n, inc, ior):
    cosi = _div(v_dot(inc, n), v_len(inc) * v_len(n))
    r0 = (1.0 - ior) / (1.0 + ior)
    r0 = r0 * r0
    cost = abs(cosi)
    return r0 + (1 - r0) * oracle_bind.lib().oracle_go_pow(1 - cost, 5.0)


def _trace(sc, o, d, depth, tmax, exclude, count):
    """trace_ray: returns (colour, top-level object of this ray's hit or -1)."""
    lib = oracle_bind.lib()
    if depth <= 0:
        return (0.0, 0.0, 0.0), -1
    count[0] += 1
    hit = closest_hit(sc, o, d, tmax, exclude)
    if hit is None:
        return v_lerp(sc.bg0, sc.bg1, 0.5 * (d[1] + 1.0)), -1
    pw, nw, mat = surface_props(sc, hit)
    lighting = compute_lighting(sc, hit[0], pw, nw, mat, d)
    col = mat.color
    if mat.reflectivity == 0 and mat.transparency == 0:
        return v_clamp(v_mul(lighting, col)), hit[0]
    reflected = (0.0, 0.0, 0.0)
    if mat.reflectivity > 0:
        rd = v_sub(d, v_scale(nw, 2.0 * v_dot(d, nw)))
        fuzz = mat.fuzziness
        if fuzz >= 0:
            cf, sf = lib.oracle_go_cos(fuzz), lib.oracle_go_sin(fuzz)
            rd = v_add(rd, (fuzz * cf * cf, fuzz * sf * sf, 0.0))
        reflected, _ = _trace(sc, v_add(pw, v_scale(nw, 1e-4)), v_norm(rd), depth - 1, INF, -1, count)
    refracted = (0.0, 0.0, 0.0)
    if mat.transparency > 0:
        n1, n2 = 1.0, mat.refractive_index
        normal = nw
        if v_dot(d, normal) > 0.0:
            n1, n2 = n2, n1
            normal = v_scale(normal, -1.0)
        rd = refract(d, normal, n1, n2)
        if not (rd[0] == 0.0 and rd[1] == 0.0 and rd[2] == 0.0):
            refracted, _ = _trace(sc, v_sub(pw, v_scale(normal, 1e-4)), rd, depth - 1, INF, -1, count)
    if mat.transparency == 0:
        return v_clamp(v_mul(v_add(lighting, v_scale(reflected, mat.reflectivity)), col)), hit[0]
    kr = fresnel(nw, d, mat.refractive_index)
    return v_clamp(v_mul(v_add(v_scale(lighting, 1.0 - mat.transparency),
                               v_add(v_scale(reflected, kr), v_scale(refracted, 1.0 - kr))), col)), hit[0]


def trace(packed, origin, dir, depth, tmax=INF, exclude=-1):
    """traceRay(ray, depth) against `packed` -> (color, object, rays): the
    colour, the top-level object the ray itself hit (-1: background) and the
    rays traced (traceRay entered with depth > 0). depth 0: the scene's."""
    sc = scene_of(packed)
    count = [0]
    o = tuple(float(x) for x in origin)
    d = tuple(float(x) for x in dir)
    color, obj = _trace(sc, o, d, sc.depth if depth == 0 else depth, float(tmax), int(exclude), count)
    return color, obj, count[0]


def trace_many(packed, origins, dirs, depth, tmax=None, exclude=None):
    """trace() of every ray -> abi.RADIANCE_DTYPE array."""
    n = len(origins)
    tm = np.full(n, np.inf) if tmax is None else np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,))
    ex = np.full(n, -1) if exclude is None else np.broadcast_to(np.asarray(exclude), (n,))
    out = np.zeros(n, dtype=abi.RADIANCE_DTYPE)
    for r in range(n):
        c, obj, rays = trace(packed, origins[r], dirs[r], depth, tm[r], ex[r])
        out[r] = (c, obj, rays)
    return out


def camera_rays(packed, y0, y1):
    """render_strip's rays (raytracer.go:605-652) for rows [y0, y1):
    abi.RAY_DTYPE array [rows, W, 4]."""
    lib = oracle_bind.lib()
    sc = scene_of(packed)
    W, Hh = sc.width, sc.height
    out = np.zeros((y1 - y0, W, 4), dtype=abi.RAY_DTYPE)
    out["tmax"] = np.inf
    out["exclude"] = -1
    eye = (0.0, 0.0, -1.0)
    draws = (C.c_double * 160)()
    for x in range(W):
        for ymin in range(y0 // 20 * 20, y1, 20):
            lib.oracle_pcg_float64(0xDEAD ^ x, 0xBEEF ^ ymin, 160, draws)
            for y in range(max(ymin, y0), min(ymin + 20, Hh, y1)):
                for k in range(4):
                    dx = draws[(y - ymin) * 8 + 2 * k] - 0.5
                    dy = draws[(y - ymin) * 8 + 2 * k + 1] - 0.5
                    u = (float(x) + dx) / float(W - 1) * sc.vw - sc.vw / 2.0
                    v = (float(y) + dy) / float(Hh - 1) * sc.vh - sc.vh / 2.0
                    o = (u, -v, 0.0)
                    out[y - y0, x, k]["origin"] = o
                    out[y - y0, x, k]["dir"] = v_norm(v_sub(o, eye))
    return out


def quantise(c):
    """vec.go:104-107 for one component: uint8(uint32(c * 65535) >> 8)."""
    v = c * 65535.0
    if not (-9223372036854775808.0 < v < 9223372036854775808.0):
        return 0
    return ((int(v) & 0xffffffff) >> 8) & 0xff


def image(rad, samples=4):
    """Render()'s pixels from [rows, W, samples] radiance records: the samples
    summed in order from zero, scaled by 1 / samples, quantised."""
    rows, W = rad.shape[:2]
    img = np.zeros((rows, W, 4), dtype=np.uint8)
    img[..., 3] = 255
    for y in range(rows):
        for x in range(W):
            total = (0.0, 0.0, 0.0)
            for k in range(samples):
                total = v_add(total, tuple(float(c) for c in rad[y, x, k]["color"]))
            c = v_scale(total, 1.0 / samples)
            img[y, x, :3] = [quantise(c[0]), quantise(c[1]), quantise(c[2])]
    return img


def render(packed):
    """(pixels, rays traced) of the whole frame through trace() over camera_rays()."""
    sc = scene_of(packed)
    rays = camera_rays(packed, 0, sc.height)
    flat = rays.reshape(-1)
    rad = trace_many(packed, flat["origin"], flat["dir"], 0).reshape(rays.shape)
    return image(rad), int(rad["rays"].sum()), rad


def mixed_glass(seed, n):
    """query_ref.mixed's construction with reflecting and refracting
    materials (mats[i % 4] per object), no duplicated objects, a mirror ground
    plane and a matte back plane, two lights, depth 5."""
    rng = random.Random(seed)
    mats = [S.material((0.8, 0.5, 0.3), 0.0, 0.0, 0.0, 1.0, 0.9, 0.3, 8.0),       # matte
            S.material((0.9, 0.9, 0.9), 0.6, 0.05, 0.0, 1.0, 0.5, 0.8, 60.0),     # fuzzy mirror
            S.material((0.9, 1.0, 0.9), 0.2, -1.0, 0.8, 1.5, 0.5, 0.8, 2.5),      # glass: no fuzz, fractional exponent
            S.material((0.7, 0.8, 1.0), 0.0, 0.0, 0.9, 1.3, 0.6, 0.4, 20.0)]      # clear
    objs = []
    for i in range(n):
        o = rng.choice([S.Sphere, S.Cube, S.Cylinder, S.Cone])(mats[i % 4])
        o = (o.translate(rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(4, 8))
             .rotatex(rng.uniform(-90, 90)).rotatey(rng.uniform(-90, 90))
             .scale(0.3 + rng.random() * 0.7, 0.3 + rng.random() * 0.7, 0.3 + rng.random() * 0.7))
        objs.append(o)
    objs.append(S.Plane(mats[1]).translate(0.0, -2.0, 0.0))
    objs.append(S.Plane(mats[0]).rotatex(80.0).translate(0.0, 0.0, 10.0))
    rng.shuffle(objs)
    return S.RenderArgs(ambient=(0.1,) * 3,
                        lights=[S.PointLight((5.0, 6.0, 0.0), (0.6,) * 3), S.PointLight((-4.0, 5.0, 3.0), (0.5, 0.4, 0.3))],
                        scene=S.Union(tuple(objs)), depth=5, fov=75.0, width=16, height=16)


def closure_fixture(width=24, height=16):
    """The reference's checked-cube.gml fixture (closure surfaces), resized."""
    import os
    from go_raytracer_amd import gml
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gml", "checked-cube.gml")
    rendered, _ = gml.run_file(path)
    args = rendered[0][0]
    args.width, args.height = width, height
    return args


SCENES = {
    "c2": lambda: rt.configs.c2(24, 16),
    "c3": lambda: rt.configs.c3(24, 16),
    "c3cone": lambda: rt.configs.c3cone(24, 16),
    "canned": lambda: rt.configs.canned(24, 16),
    "c4csg": lambda: rt.configs.c4csg(16, 12),
    "closure": closure_fixture,
    "c4": lambda: rt.configs.c4(16, 12),
    "glass21": lambda: mixed_glass(21, 8),
    "glass22": lambda: mixed_glass(22, 40),
}
_packed = {}
_cache = {}


def packed(name):
    """The converted scene `name` of SCENES (one per process: shared, never modified)."""
    if name not in _packed:
        _packed[name] = S.convert(SCENES[name]())
    return _packed[name]


def ray_set(n):
    """n of the rays query_ref.rays(1024, 5), evenly strided (both of its
    halves: camera-like rays and rays starting inside the scene box)."""
    o, d = query_ref.rays(1024, 5)
    return o[::1024 // n][:n], d[::1024 // n][:n]


def reference(name, n, depth, tmax=None, exclude=None, key=None):
    """trace_many of ray_set(n) against scene `name`, computed once per
    process and shared (never modified). `key` names a tmax / exclude variant."""
    k = (name, n, depth, key)
    if k not in _cache:
        o, d = ray_set(n)
        _cache[k] = trace_many(packed(name), o, d, depth, tmax, exclude)
    return _cache[k]
