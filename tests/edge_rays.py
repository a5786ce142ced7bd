"""Edge rays for the ray-query, radiance and camera kernels -- test
infrastructure (no tests in here; tests/test_edge_rays_ref.py asserts from the
oracle's side what each family covers, tests/test_gpu_edge_rays.py sends them
to the device).

The rays of query_ref.rays() / trace_ref.ray_set() are random origins with
generic directions. The families here are what those never send: directions
with exact zero components (A, B), far origins on an axis (B), rays within
ulps of tangent (C), origins exactly on a surface (D), directions of length
2^-600 .. 2^600 (E) and zero, denormal, NaN and infinite components (F).

Every family is `(origins [n,3], dirs [n,3], tmax [n], exclude [n])`;
records() packs one into abi.RAY_DTYPE. Everything is deterministic, computed
once per process and never modified.
"""
import ctypes as C

import numpy as np

import go_raytracer_amd as rt
import oracle_bind
import query_ref as Q

S = rt.scene
abi = rt.abi
INF = float("inf")
NAN = float("nan")

# ---- the lattice scene -------------------------------------------------------
LX = [-6.0, -5.5, -3.0, -2.0, 0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.5]
LY = [-1.0, 0.0, 0.5, 1.0, 2.0, 3.0]
LZ = [4.0, 4.5, 5.0, 6.0, 7.0]
LY_SIDE = [-1.0, 0.0, 0.5, 1.0, 2.0]


def lattice(materials="plain"):
    """Objects on axis-aligned lattice coordinates, translation and scale only
    (the diagonal and has_transform == 0 paths): 19 bounded objects, two planes
    and two composites. A transform written first applies last
    (scene.SceneObject.transform), so `.translate(t).scale(s)` is the object
    scaled by s, then moved to t.

    "plain": three matte materials, one light. "glass": matte, mirror
    (reflectivity 0.6, no fuzz, so axis-aligned reflections stay on their
    axis) and glass (transparency 0.8, index 1.5, reflectivity 0.2: two children
    per hit) in turn, and a second light."""
    assert materials in ("plain", "glass")
    if materials == "plain":
        mats = [S.material(c, 0.0, 0.0, 0.0, 1.0, 0.5, 0.5, 5.0)
                for c in ((0.8, 0.3, 0.2), (0.2, 0.7, 0.4), (0.3, 0.4, 0.9))]
        lights = [S.PointLight((5.0, 6.0, 0.0), (0.6,) * 3)]
    else:
        mats = [S.material((0.8, 0.5, 0.3), 0.0, 0.0, 0.0, 1.0, 0.9, 0.3, 8.0),
                S.material((0.9, 0.9, 0.9), 0.6, -1.0, 0.0, 1.0, 0.5, 0.8, 60.0),
                S.material((0.9, 1.0, 0.9), 0.2, -1.0, 0.8, 1.5, 0.5, 0.8, 2.5)]
        lights = [S.PointLight((5.0, 6.0, 0.0), (0.6,) * 3), S.PointLight((0.5, 9.0, 4.5), (0.5, 0.4, 0.3))]
    n = [0]

    def m():
        n[0] += 1
        return mats[(n[0] - 1) % 3]

    objs = [
        S.Cube(m()).translate(0, 0, 4),
        S.Cube(m()).translate(2, 0, 4).scale(1, 2, 0.5),
        S.Sphere(m()).translate(-3, 0, 6),
        S.Sphere(m()).translate(0.5, 3, 6).uscale(0.5),
        S.Cylinder(m()).translate(4, -1, 6),
        S.Cone(m()).translate(-3, 2, 5),
        S.Sphere(m()),
        S.Plane(mats[0]).translate(0, -1, 0),
        S.Plane(mats[1] if materials == "glass" else mats[2]).translate(0, 0, 10).rotatex(90),
    ]
    for i in range(4):
        for j in range(3):
            objs.append(S.Sphere(m()).translate(-3 + 2 * i, 5, 4 + 2 * j).uscale(0.25))
    # (the spheres sit on lattice points of their cube's surface, so that axis
    # rays through lattice points end on the sphere leaves: inside the hole of
    # the difference, flipped normal, and on the cap of the intersection)
    objs.append(S.Difference(S.Cube(m()).translate(-6, 0, 4), S.Sphere(m()).translate(-5.5, 1, 4).uscale(0.75)))
    objs.append(S.Intersect(S.Cube(m()).translate(6, 0, 4), S.Sphere(m()).translate(6.5, 0.5, 4).uscale(0.6)))
    return S.RenderArgs(ambient=(0.1,) * 3, lights=lights, scene=S.Union(tuple(objs)), depth=4, fov=75.0,
                        width=32, height=24)


SCENES = {"lattice": lambda: lattice("plain"), "lattice-glass": lambda: lattice("glass")}
_packed = {}
_cache = {}


def packed(name):
    """The converted scene `name`: one of SCENES here, else query_ref's."""
    if name not in SCENES:
        return Q.packed(name)
    if name not in _packed:
        _packed[name] = S.convert(SCENES[name]())
    return _packed[name]


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _fam(o, d, tmax=None, exclude=None):
    o = np.ascontiguousarray(o, dtype=np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1, 3)
    n = len(o)
    tm = np.full(n, INF) if tmax is None else np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,)).copy()
    ex = np.full(n, -1, dtype=np.int32) if exclude is None else \
        np.broadcast_to(np.asarray(exclude, dtype=np.int32), (n,)).copy()
    return o, d, tm, ex


def records(fam):
    """A family as abi.RAY_DTYPE records."""
    o, d, tm, ex = fam
    rec = np.zeros(len(o), dtype=abi.RAY_DTYPE)
    rec["origin"], rec["dir"], rec["tmax"], rec["exclude"] = o, d, tm, ex
    return rec


def family(rec):
    """abi.RAY_DTYPE records as a family."""
    return rec["origin"].copy(), rec["dir"].copy(), rec["tmax"].copy(), rec["exclude"].copy()


def concat(fams):
    return tuple(np.concatenate([f[k] for f in fams]) for k in range(4))


# ---- A: axis rays ------------------------------------------------------------
def axis_rays():
    """Family A's origins with their unit directions: lattice points on the six
    planes around the scene, each looking along its axis towards the scene."""
    def make():
        o, d = [], []
        for z, s in ((0.0, 1.0), (9.0, -1.0)):
            for x in LX:
                for y in LY:
                    o.append((x, y, z))
                    d.append((0.0, 0.0, s))
        for x, s in ((-8.0, 1.0), (8.0, -1.0)):
            for z in LZ:
                for y in LY_SIDE:
                    o.append((x, y, z))
                    d.append((s, 0.0, 0.0))
        for y, s in ((9.0, -1.0), (-0.5, 1.0)):
            for x in LX:
                for z in LZ:
                    o.append((x, y, z))
                    d.append((0.0, s, 0.0))
        return np.array(o), np.array(d)
    return _once("axis", make)


def family_a():
    """Every axis ray in four forms: unit, length 2.5, and a -0.0 in one and in
    the other zero component (blocks of len(axis_rays()[0]) in that order)."""
    def make():
        o, d = axis_rays()
        zero = [np.flatnonzero(v == 0.0) for v in d]
        d2, d3 = d.copy(), d.copy()
        for r, z in enumerate(zero):
            d2[r, z[0]] = -0.0
            d3[r, z[1]] = -0.0
        return _fam(np.concatenate([o] * 4), np.concatenate([d, 2.5 * d, d2, d3]))
    return _once("A", make)


# ---- B: far axis rays --------------------------------------------------------
def family_b():
    """Family A's unit rays from 1e3, 1e5 and 1e7 further back (ray_slack above
    1e-3: far_shift runs with two zero direction components), then 64 whose
    perpendicular coordinates are +-1e4 as well: those miss the BVH's box."""
    def make():
        o, d = axis_rays()
        oo = [o - dist * d for dist in (1e3, 1e5, 1e7)]
        dd = [d] * 3
        # (half of them along x: parallel to both planes, so they meet nothing)
        alongx = np.flatnonzero(d[:, 0] != 0.0)
        other = np.flatnonzero(d[:, 0] == 0.0)
        pick = np.concatenate([alongx[np.arange(32) * (len(alongx) // 32)], other[np.arange(32) * (len(other) // 32)]])
        po = o[pick] - 1e5 * d[pick]
        for r in range(64):
            z = np.flatnonzero(d[pick[r]] == 0.0)
            po[r, z[0]] = 1e4 if r % 2 == 0 else -1e4
            po[r, z[1]] = 1e4 if r % 4 < 2 else -1e4
        return _fam(np.concatenate(oo + [po]), np.concatenate(dd + [d[pick]]))
    return _once("B", make)


# ---- C: grazing rays, by bisection against the oracle --------------------------
G0, G1, G2, G3 = (0.3, -0.2, 1.0), (-0.7, 0.5, 0.4), (0.2, 0.9, -0.3), (1.1, 0.1, 0.6)
_OBJ_CENTRE = {abi.RT_SPHERE: (0.0, 0.0, 0.0), abi.RT_CUBE: (0.5, 0.5, 0.5), abi.RT_CYLINDER: (0.0, 0.5, 0.0),
               abi.RT_CONE: (0.0, 0.75, 0.0)}
C_SNAPSHOTS = (10, 20, 30, 40)


def oracle_hits(p, i, o, d):
    """oracle_intersect of object i alone: a result closestHit could keep."""
    t, pt, f = C.c_double(), (C.c_double * 3)(), C.c_int()
    ok = oracle_bind.lib().oracle_intersect(C.addressof(p.scene), int(i), (C.c_double * 3)(*o), (C.c_double * 3)(*d),
                                            C.byref(t), pt, C.byref(f))
    return ok == 1 and t.value < INF


def scene_winner(p, o, d):
    """closestHit's winner among all objects (-1: none), from oracle_intersect."""
    t, pt, f = C.c_double(), (C.c_double * 3)(), C.c_int()
    best, bt = -1, INF
    oo, dd = (C.c_double * 3)(*o), (C.c_double * 3)(*d)
    for j in range(int(p.scene.num_objects)):
        if oracle_bind.lib().oracle_intersect(C.addressof(p.scene), j, oo, dd, C.byref(t), pt, C.byref(f)) == 1 \
                and t.value < bt:
            best, bt = j, t.value
    return best


def _centre(p, i):
    o = p.scene.objects[i]
    if o.kind == abi.RT_CSG:
        o = p.scene.csg_leaves[o.csg_first]
    c = np.array(_OBJ_CENTRE[o.kind] + (1.0,))
    if not o.has_transform:
        return c[:3]
    return (np.array(o.transform[:]).reshape(4, 4) @ c)[:3]


def _perp(d):
    e = np.zeros(3)
    e[int(np.argmin(np.abs(d)))] = 1.0
    pv = np.cross(d, e)
    pv /= np.linalg.norm(pv)
    qv = np.cross(d, pv)
    return pv, qv / np.linalg.norm(qv)


def ulps(a, b):
    """Distance of two finite doubles in units in the last place."""
    ia, ib = (int(np.float64(v).view(np.int64)) for v in (a, b))
    ia, ib = (v if v >= 0 else -(v & 0x7fffffffffffffff) for v in (ia, ib))
    return abs(ia - ib)


def bisect(p, i, d):
    """Origins on a line perpendicular to d between which object i goes from
    hit to miss: [(halvings, o_hit, o_miss)] after 10, 20, 30 and 40 halvings
    and at the end (50 halvings, then until every coordinate of the two is
    within 4 ulp; halvings = -1)."""
    d = np.asarray(d, dtype=np.float64)
    pv, qv = _perp(d)
    c = _centre(p, i)
    lo = None
    # start 20 units back, or nearer if another object lies in between: the grazed object is to
    # be the ray's closest hit where the scene allows it, or the query never reports it
    for dist in (20.0, 6.0, 3.0, 2.0, 1.5):
        back = d * (dist / np.linalg.norm(d))
        for a, b in [(0.0, 0.0)] + [(a, b) for a in (0.2, -0.2, 0.4, -0.4, 0.0) for b in (0.2, -0.2, 0.4, -0.4, 0.0)]:
            cand = c + a * pv + b * qv - back
            if oracle_hits(p, i, cand, d) and (lo is None or scene_winner(p, cand, d) == i):
                first = lo is None
                lo = cand
                if not first or scene_winner(p, cand, d) == i:
                    break
        if lo is not None and scene_winner(p, lo, d) == i:
            break
    assert lo is not None, "no hitting ray for object %d" % i
    hi = lo + 6.0 * pv
    assert not oracle_hits(p, i, hi, d), "object %d still hit 6 units off" % i
    out = []
    for k in range(1, 120):
        mid = 0.5 * (lo + hi)
        if (mid == lo).all() or (mid == hi).all():
            break
        if oracle_hits(p, i, mid, d):
            lo = mid
        else:
            hi = mid
        if k in C_SNAPSHOTS:
            out.append((k, lo.copy(), hi.copy()))
        if k >= 50 and max(ulps(lo[q], hi[q]) for q in range(3)) <= 4:
            break
    out.append((-1, lo.copy(), hi.copy()))
    return out


# (more directions for composites: each gives ten unit-length rays, and whole
# 64-ray waves of those are what reaches csg_hit's leaf and group culls)
_MORE = [tuple(v) for v in np.round(np.random.default_rng(4).standard_normal((10, 3)) * 1.5, 3)]


def _c_dirs(name, kind):
    if name == "lattice":
        return [(0.0, 0.0, 2.0), G0, (2.0, 0.0, 0.0), G1, G2, G3] + _MORE[:2] if kind == abi.RT_CSG \
            else [(0.0, 0.0, 2.0), G0]
    return [G0, G1, G2, G3] + _MORE if kind == abi.RT_CSG else [G0, G1]


def is_unit(d):
    """SceneSearch's unit_dir predicate per ray: | |d|^2 - 1 | <= 1e-9."""
    with np.errstate(all="ignore"):
        return np.abs((d * d).sum(axis=1) - 1.0) <= 1e-9


def unit_waves(d):
    """Per whole 64-ray wave of a batch: every direction is unit length (the
    wave votes unit_dir and its composites go through csg_hit)."""
    u = is_unit(d)
    return u[:len(u) // 64 * 64].reshape(-1, 64).all(axis=1)


def family_c(name):
    """(family, pairs): for every bounded top-level object of `name` (mixed12,
    lattice) or every composite (c4csg), and each of its directions as given
    and normalised, bisect()'s origins. pairs: rows (object, kind, halvings,
    hit row, miss row). Order: the normalised rays first, those aimed at
    composites leading, then the rays as given. unit_dir is a vote of the
    whole wave, so only a wave of nothing but unit directions takes csg_hit
    with its FP32 leaf and group culls: sent from a 64-ray boundary, the first
    waves of the family are such waves."""
    def make():
        p = packed(name)
        found = []  # (sort key, object, kind, halvings, o_hit, o_miss, direction)
        for i in range(int(p.scene.num_objects)):
            kind = int(p.scene.objects[i].kind)
            if kind == abi.RT_PLANE or (name == "c4csg" and kind != abi.RT_CSG):
                continue
            for dr in _c_dirs(name, kind):
                dr = np.array(dr, dtype=np.float64)
                for unit, dv in ((False, dr), (True, dr / np.linalg.norm(dr))):
                    for k, oh, om in bisect(p, i, dv):
                        found.append((0 if unit and kind == abi.RT_CSG else 1 if unit else 2, i, kind, k, oh, om, dv))
        found.sort(key=lambda f: f[0])  # (stable)
        o, d, pairs = [], [], []
        for _, i, kind, k, oh, om, dv in found:
            pairs.append((i, kind, k, len(o), len(o) + 1))
            o += [oh, om]
            d += [dv, dv]
        return _fam(o, d), np.array(pairs, dtype=np.int64)
    return _once(("C", name), make)


# ---- D: origins on a surface ---------------------------------------------------
def _d_source(name):
    """Rays whose oracle hits give family D's origins."""
    if name in SCENES:
        ao, ad = axis_rays()
        ro, rd = Q.rays(512, 9)
        o, d = np.concatenate([ro, ao]), np.concatenate([rd, ad])
        return Q.Table(packed(name), o, d)
    return Q.table(name)


D_HITS = {"lattice": 256}  # (others: 128)


def family_d(name):
    """(family, own, kinds): from D_HITS oracle hits of scene `name` (on the
    lattice most surface points are exact and a ray from one rarely meets its
    own surface again at t > 0, hence more of them), spread over the
    surface kinds and the composites, rays that start at point_world exactly
    along +n, -n, the incoming direction and a tangent n x e, each with exclude
    = -1 (first half of the family) and with the hit object excluded (second
    half). Each half is four blocks, one per direction, in that order: the
    normals are unit length, so the +n and -n blocks are whole waves of unit
    directions (csg_hit for a composite), the other two are not. own: the hit
    object of every ray; kinds: the surface kinds among the hits, -1 for a
    composite."""
    def make():
        count = D_HITS.get(name, 128)
        T = _d_source(name)
        p = T.packed
        hits = T.closest()
        good = (hits["object"] >= 0) & np.isfinite(hits["normal_world"]).all(axis=1)
        cat = {}
        for r in np.flatnonzero(good):
            top = p.scene.objects[int(hits["object"][r])].kind
            key = -1 if top == abi.RT_CSG else int(hits["kind"][r])
            if key != abi.RT_PLANE or len(cat.get(key, ())) < 8:  # (a plane is never met again from its own surface)
                cat.setdefault(key, []).append(r)
        rows, depth = [], 0
        while len(rows) < count and any(depth < len(v) for v in cat.values()):
            for key in sorted(cat):
                if depth < len(cat[key]) and len(rows) < count:
                    rows.append(cat[key][depth])
            depth += 1
        assert len(rows) == count, (name, len(rows))
        o, d, own = [], [], []
        for which in range(4):
            for r in rows:
                n = hits["normal_world"][r]
                e = np.zeros(3)
                e[int(np.argmin(np.abs(n)))] = 1.0
                o.append(hits["point_world"][r])
                d.append((n, -n, T.dirs[r], np.cross(n, e))[which])
                own.append(int(hits["object"][r]))
        own = np.array(own, dtype=np.int32)
        fam = _fam(np.concatenate([o, o]), np.concatenate([d, d]), None, np.concatenate([np.full(len(own), -1), own]))
        return fam, np.concatenate([own, own]), sorted(cat)
    return _once(("D", name), make)


# ---- E: scaled directions ------------------------------------------------------
E_K = (-600, -200, -64, -61, -60, -59, -56, 56, 59, 60, 61, 64, 200, 600)


def e_base():
    """128 unit-length rays: 64 of family A's and 64 of query_ref.rays, normalised."""
    def make():
        ao, ad = axis_rays()
        pick = np.arange(64) * (len(ao) // 64) + 1
        ro, rd = Q.rays(64, 17)
        rd = rd / np.linalg.norm(rd, axis=1)[:, None]
        return np.concatenate([ao[pick], ro]), np.concatenate([ad[pick], rd])
    return _once("Ebase", make)


def family_e():
    """(family, k): e_base()'s rays with the direction times 2^k for every k of
    E_K (blocks of 128 in that order; the products are exact or, at -600 with a
    tiny component, rounded once)."""
    def make():
        o, d = e_base()
        return (_fam(np.concatenate([o] * len(E_K)), np.concatenate([d * 2.0 ** k for k in E_K])),
                np.repeat(np.array(E_K), len(o)))
    return _once("E", make)


# ---- F: degenerate rays --------------------------------------------------------
F_ZERO_DIRS = [(0.0, 0.0, 0.0), (-0.0, 0.0, 0.0)]
F_TINY_HUGE_DIRS = [(0.0, 0.0, 5e-324), (1e-200, 0.0, 0.0), (0.0, 0.0, 1e200)]
F_NAN_DIRS = [(NAN, 0.0, 1.0), (0.0, NAN, 1.0), (0.0, 0.0, NAN)]
F_INF_DIRS = [(INF, 0.0, 1.0), (-INF, 0.0, 1.0), (0.0, INF, 1.0), (0.0, -INF, 1.0), (0.0, 0.0, INF), (0.0, 0.0, -INF)]
F_DIRS = F_ZERO_DIRS + F_TINY_HUGE_DIRS + F_NAN_DIRS + F_INF_DIRS + [(0.0, 0.0, 1.0)]
F_ORIGINS = [(0.5, 0.5, 0.0), (0.5, 0.5, 4.5), (-3.0, 0.0, 6.0), (0.0, 0.0, 0.0),
             (NAN, 0.0, 0.0), (INF, 0.0, 0.0), (-INF, 0.0, 0.0), (1e20, 0.0, 0.0), (1e31, 0.0, 0.0)]
F_TMAX = [NAN, 0.0, -1.0, -INF, 5e-324]


def family_f(num_objects):
    """(family, dir class): every F_ORIGINS x F_DIRS ray, then (0.5, 0.5, 0) ->
    (0, 0, 1) with each tmax of F_TMAX and with exclude = num_objects, 2^31 - 1,
    -2^31 and -2. dir class per ray: "zero", "tiny", "nan", "inf" or "unit"."""
    cls = ["zero"] * len(F_ZERO_DIRS) + ["tiny"] * len(F_TINY_HUGE_DIRS) + ["nan"] * len(F_NAN_DIRS) + \
        ["inf"] * len(F_INF_DIRS) + ["unit"]
    o, d, tm, ex, c = [], [], [], [], []
    for oo in F_ORIGINS:
        for dd, cc in zip(F_DIRS, cls):
            o.append(oo)
            d.append(dd)
            tm.append(INF)
            ex.append(-1)
            c.append(cc)
    for t in F_TMAX:
        o.append(F_ORIGINS[0])
        d.append((0.0, 0.0, 1.0))
        tm.append(t)
        ex.append(-1)
        c.append("unit")
    for x in (int(num_objects), 2 ** 31 - 1, -2 ** 31, -2):
        o.append(F_ORIGINS[0])
        d.append((0.0, 0.0, 1.0))
        tm.append(INF)
        ex.append(x)
        c.append("unit")
    return _fam(o, d, tm, ex), np.array(c)


# ---- what the CPU and the GPU tests share ----------------------------------------
def winner_t(Tb, tmax=None, exclude=None):
    """The oracle winner's t per ray of a query_ref.Table (+inf: a miss)."""
    w = Tb.winners(tmax, exclude)
    return np.array([Tb.t[r, w[r]] if w[r] >= 0 else INF for r in range(len(w))])


def radiance_rays():
    """The batch of the radiance tests: families A + B + F (for the lattice's
    23 objects)."""
    return _once("radiance", lambda: concat([family_a(), family_b(), family_f(packed("lattice").scene.num_objects)[0]]))


# ---- comparing and mixing ------------------------------------------------------
def same(a, b):
    """[(field, rows)] in which the structured arrays a and b differ. Integer
    fields compare with ==; a float component is equal when a == b (so +0
    equals -0) or when both are NaN: the sign and payload of a NaN are not part
    of the contract (the rule rt_render.h states for asin / acos)."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    bad = []
    for k in a.dtype.names:
        x, y = a[k], b[k]
        ne = x != y
        if x.dtype.kind == "f":
            ne &= ~(np.isnan(x) & np.isnan(y))
        ne = np.asarray(ne).reshape(len(a), -1).any(axis=1)
        if ne.any():
            bad.append((k, np.flatnonzero(ne)))
    return bad


def assert_same(got, want, what):
    bad = same(got, want)
    if bad:
        k, rows = bad[0]
        r = int(rows[0])
        raise AssertionError("%s: fields %s differ; %s in %d of %d records; first ray %d: gpu %s oracle %s"
                             % (what, [f for f, _ in bad], k, len(rows), len(got), r, got[r], want[r]))


def interleave(fams, seed):
    """(batch, perm): the families' rays in one batch in which each family is
    spread evenly over the whole length (ray j of a family of n sits at
    position (j + u) / n, u random), so neighbours come from different families
    and every 64-ray wave holds several kinds. batch = concat(fams)[perm]."""
    g = np.random.default_rng(seed)
    key = np.concatenate([(np.arange(len(f[0])) + g.random(len(f[0]))) / max(1, len(f[0])) for f in fams])
    perm = np.argsort(key, kind="stable")
    allr = concat(fams)
    return tuple(v[perm] for v in allr), perm
