"""Scenes and rays at the limits of the FP32 culls -- test infrastructure (no
tests in here; tests/test_cull_limits_ref.py asserts from the oracle's side
what each family contains, tests/test_gpu_cull_limits.py sends them to the
device).

Every cull rests on "the exact FP64 test can only report a hit whose point
lies inside the object's bounding sphere". That holds only where the FP64
intersection code is itself accurate; the contract is the oracle's records, not
geometry. The families here are where the two part, and where the BVH builder
meets layouts it was never given:

  far      rays that start 1e2 .. 1e12 units from an object and pass it at 0 .. 3
           padded radii: from 1e7 units (small objects) the sign of the quadric
           discriminant is rounding noise and the oracle reports hits of rays
           that pass well outside the bounding sphere
  needle   objects under scale(1/s, 1, s) between rotations, s = 1 .. 1e8: the
           cofactor inverse and the object-space quadratic lose the object
  layout   geometric arms, coincident centroids, one sphere around everything,
           the 11 / 12 / 13 object boundary of the BVH, every leaf size
  horizon  a frame whose ground hits lie 1e6 .. 3e7 units out, with small
           spheres on the way to the light (rt_render.h's own far_shift sites)

A family is `(origins [n,3], dirs [n,3], tmax [n], exclude [n])` as in
edge_rays.py. Every scene has a linear form (11 bounded objects) and a BVH form
(16), both with one plane. Rays come in batches of at most BATCH; half of every
batch has unit directions (its first whole waves: csg_hit is taken only by a
wave of nothing but unit directions), the other half directions of length 0.1
to 3. Everything is deterministic, computed once per process and never modified.
"""
import math
import random

import numpy as np

import go_raytracer_amd as rt
import edge_rays as E
import query_ref as Q

S = rt.scene
abi = rt.abi
INF = float("inf")
BATCH = 512
FORMS = {"linear": 11, "bvh": 16}
KINDS = (abi.RT_SPHERE, abi.RT_CUBE, abi.RT_CYLINDER, abi.RT_CONE)
KIND_NAME = {abi.RT_SPHERE: "sphere", abi.RT_CUBE: "cube", abi.RT_CYLINDER: "cylinder", abi.RT_CONE: "cone"}
_CTOR = {abi.RT_SPHERE: S.Sphere, abi.RT_CUBE: S.Cube, abi.RT_CYLINDER: S.Cylinder, abi.RT_CONE: S.Cone}
# rt_set_scene's bounding sphere of the unit primitives: local centre, local radius
LC = {abi.RT_SPHERE: (0.0, 0.0, 0.0), abi.RT_CUBE: (0.5, 0.5, 0.5), abi.RT_CYLINDER: (0.0, 0.5, 0.0),
      abi.RT_CONE: (0.0, 0.5, 0.0)}
LR = {abi.RT_SPHERE: 1.0, abi.RT_CUBE: 0.8660254037844387, abi.RT_CYLINDER: 1.118033988749895,
      abi.RT_CONE: 1.118033988749895}
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _mats():
    """Two matte materials around a mirror (reflectivity 0.5, no fuzz)."""
    m = [S.material(c, 0.0, 0.0, 0.0, 1.0, 0.5, 0.5, 5.0) for c in ((0.8, 0.3, 0.2), (0.2, 0.7, 0.4), (0.3, 0.4, 0.9))]
    m[1] = S.material((0.9, 0.9, 0.9), 0.5, -1.0, 0.0, 1.0, 0.5, 0.8, 30.0)
    return m


def _args(objs, depth=3, lights=None, fov=75.0, width=48, height=32):
    return S.RenderArgs(ambient=(0.1,) * 3, lights=lights or [S.PointLight((5.0, 6.0, 0.0), (0.6,) * 3)],
                        scene=S.Union(tuple(objs)), depth=depth, fov=fov, width=width, height=height)


# ---- the host's bounding spheres, restated -----------------------------------------
def o2w_of(o):
    """An rt_object's object-to-world matrix [4, 4]."""
    return np.array(o.transform[:]).reshape(4, 4) if o.has_transform else np.eye(4)


def bound_of(o):
    """(centre [3], padded radius, unpadded radius) of a bounded rt_object: rt_set_scene's
    `fro`, `cc`, `cmax` and `rad = fro * lr * 1.0001 + 1e-4 * (1 + cmax + fro)`."""
    m = o2w_of(o)
    fro = math.sqrt(sum(float(m[r][k]) * float(m[r][k]) for r in range(3) for k in range(3)))
    lc = LC[o.kind]
    cc = [float(m[r][0]) * lc[0] + float(m[r][1]) * lc[1] + float(m[r][2]) * lc[2] + float(m[r][3]) for r in range(3)]
    cmax = max(abs(c) for c in cc)
    return np.array(cc), fro * LR[o.kind] * 1.0001 + 1e-4 * (1.0 + cmax + fro), fro * LR[o.kind]


def targets(p):
    """The bounded primitives of a packed scene: [(top-level object, rt_object)], a
    composite's leaves under the composite's index."""
    out = []
    for i in range(int(p.scene.num_objects)):
        o = p.scene.objects[i]
        if o.kind == abi.RT_CSG:
            out += [(i, p.scene.csg_leaves[o.csg_first + j]) for j in range(o.csg_count)
                    if p.scene.csg_leaves[o.csg_first + j].kind != abi.RT_PLANE]
        elif o.kind != abi.RT_PLANE:
            out.append((i, o))
    return out


def line_distance(o, d, c):
    """Distance of the points c [m, 3] from the lines o + t d [n, 3] as the doubles
    stand, in long double -> [n, m]."""
    L = np.longdouble
    o, d, c = o.astype(L), d.astype(L), np.asarray(c).astype(L)
    v = c[None, :, :] - o[:, None, :]
    dd = d[:, None, :]
    cr = np.stack([v[..., 1] * dd[..., 2] - v[..., 2] * dd[..., 1], v[..., 2] * dd[..., 0] - v[..., 0] * dd[..., 2],
                   v[..., 0] * dd[..., 1] - v[..., 1] * dd[..., 0]], axis=-1)
    return np.sqrt((cr * cr).sum(axis=-1)) / np.sqrt((d * d).sum(axis=-1))[:, None]


def point_distance(o, d, t, c):
    """|o + t d - c| per ray in long double (t, c per ray)."""
    L = np.longdouble
    q = o.astype(L) + t.astype(L)[:, None] * d.astype(L) - np.asarray(c).astype(L)
    return np.sqrt((q * q).sum(axis=-1))


def _perp(g, u):
    w = np.cross(u, g.standard_normal(3))
    return w / np.linalg.norm(w)


def _lengths(d, n_unit):
    """Directions normalised; from row n_unit on, scaled by 0.1 .. 3."""
    d = d / np.linalg.norm(d, axis=1)[:, None]
    k = np.arange(len(d) - n_unit)
    d[n_unit:] *= (0.1 + 2.9 * ((k * 0.6180339887498949) % 1.0))[:, None]
    return d


# ---- far: far ray origins ---------------------------------------------------------
FAR_D = (1e2, 1e4, 1e6, 1e7, 1e8, 1e10, 1e12)
FAR_USCALE = (1.0, 0.04)


# max over every rung's oracle hits of (distance of the ray's line from the bounding centre -
# enclosing radius) / D and of (|t |d| - distance to the closest approach| - enclosing radius) / D,
# long double: how far beside and how far along the ray the oracle's hit lies from the object
# (test_cull_limits_ref.py measures both per rung: 2.42e-8 beside at D = 1e8, 2.68e-8 along at
# 1e12; about sqrt(2^-53) = 1.05e-8 as the discriminant's error 2^-53 D^2 predicts), and the bound
# rt_render.h's RT_FAR_ERR takes from it: the next power of two above 8 x the measurement
FAR_ERR_MEASURED = 2.7e-8
FAR_ERR_BOUND = 2.0 ** -22


def far_scene(form):
    """"linear" / "bvh": FORMS[form] objects of the four bounded kinds in turn, uscale
    1 and 0.04 in turn per round of four, mildly rotated, within 10 units of
    (0, 0, 8), and a plane below. "csg": the bvh form's first 12 objects, one
    difference and one intersection of such leaves, and the plane."""
    def make():
        rng = random.Random(31)
        mats = _mats()
        objs = []
        for i in range(16):
            k = KINDS[i % 4]
            s = FAR_USCALE[(i // 4) % 2]
            objs.append(_CTOR[k](mats[i % 3]).translate(rng.uniform(-5, 5), rng.uniform(-4, 5), rng.uniform(4, 13))
                        .rotatex(rng.uniform(-25, 25)).rotatey(rng.uniform(-25, 25)).uscale(s))
        plane = S.Plane(mats[0]).translate(0.0, -8.0, 0.0)
        if form == "csg":
            diff = S.Difference(S.Sphere(mats[1]).translate(-7.0, 3.0, 9.0).rotatex(15.0),
                                S.Cylinder(mats[2]).translate(-6.6, 2.6, 8.6).rotatey(-20.0))
            inter = S.Intersect(S.Sphere(mats[2]).translate(6.0, 2.0, 5.0).rotatey(10.0).uscale(0.04),
                                S.Cube(mats[0]).translate(5.99, 1.98, 4.98).rotatex(-12.0).uscale(0.04))
            objs = objs[:6] + [diff] + objs[6:12] + [plane, inter]
        else:
            objs = objs[:FORMS[form]]
            objs.insert(5, plane)
        return S.convert(_args(objs))
    return _once(("far", form), make)


def _aimed(g, c, R, D, bs):
    """Rays from c + D u (u random) that pass c at impact parameters bs * R."""
    o, d = [], []
    for b in bs:
        u = g.standard_normal(3)
        u /= np.linalg.norm(u)
        oo = c + D * u
        o.append(oo)
        d.append(c + b * R * _perp(g, u) - oo)
    return o, d


# D -> {(kind, uscale): (rays, from, to)}: further whole batches aimed at those objects alone, at
# impact parameters spread over [from, to] padded radii, where a rung's first batch holds fewer
# than 8 oracle hits outside the padded sphere for that class (rates measured on the CPU from the
# oracle alone, 4096 rays over [0.9, 3]: unit cylinder at 1e8 5 hits, all within [1, 1.2];
# cylinder of 0.04 73 at 1e7, 119 .. 142 from 1e8; unit sphere at 1e8 138).
# test_cull_limits_ref.py asserts the counts.
FAR_EXTRA = {
    1e7: {(abi.RT_SPHERE, 0.04): (512, 0.9, 3.0), (abi.RT_CYLINDER, 0.04): (1024, 1.0, 2.0)},
    1e8: {(abi.RT_SPHERE, 1.0): (512, 0.9, 3.0), (abi.RT_CYLINDER, 1.0): (3072, 1.0, 1.2),
          (abi.RT_CYLINDER, 0.04): (512, 0.9, 3.0)},
    1e10: {(abi.RT_CYLINDER, 0.04): (512, 0.9, 3.0)},
    1e12: {(abi.RT_CYLINDER, 0.04): (512, 0.9, 3.0)},
}


def _far_impacts(n):
    """n impact parameters in padded radii: 2 at the centre, a quarter of the rest
    over [0, 0.9), the others over [0.9, 3]."""
    m = n - 2
    a = m // 4
    return np.concatenate([[0.0, 0.0], 0.9 * (np.arange(a) + 0.5) / a, 0.9 + 2.1 * (np.arange(m - a) + 0.5) / (m - a)])


def far_rays(form, D):
    """The rung's rays, a multiple of BATCH: per bounded primitive of far_scene(form)
    BATCH // primitives rays from D units out (then FAR_EXTRA's batches), the
    primitives interleaved; per batch the first half unit length."""
    def make():
        p = far_scene(form)
        tg = targets(p)
        g = np.random.default_rng([int(math.log10(D)), len(tg)])
        per = BATCH // len(tg)
        oo, dd = [], []
        for _, ob in tg:
            c, R, _ = bound_of(ob)
            o, d = _aimed(g, c, R, D, _far_impacts(per))
            oo.append(o)
            dd.append(d)
        # ray j of every primitive in turn, so each half of the batch holds every impact class
        order = g.permutation(per)
        o = [oo[i][j] for j in order for i in range(len(tg))]
        d = [dd[i][j] for j in order for i in range(len(tg))]
        while len(o) < BATCH:  # (pad to a whole batch with centre rays)
            o.append(oo[len(o) % len(tg)][0])
            d.append(dd[len(d) % len(tg)][0])
        batches = [(np.array(o), _lengths(np.array(d), BATCH // 2))]
        for (kind, us), (n, b0, b1) in sorted(FAR_EXTRA.get(D, {}).items()):
            assert n % BATCH == 0
            sel = [ob for _, ob in tg if ob.kind == kind and abs(bound_of(ob)[2] / LR[kind] / math.sqrt(3.0) - us) < 1e-9]
            assert sel
            for _ in range(0, n, BATCH):
                eo, ed = [], []
                bs = b0 + (b1 - b0) * (g.permutation(BATCH) + 0.5) / BATCH
                for j in range(BATCH):
                    c, R, _ = bound_of(sel[j % len(sel)])
                    a, b = _aimed(g, c, R, D, [bs[j]])
                    eo += a
                    ed += b
                batches.append((np.array(eo), _lengths(np.array(ed), BATCH // 2)))
        return E._fam(np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches]))
    return _once(("far-rays", form, D), make)


def far_tmax(fam):
    """A bound just past the far scenes per ray: the parameter at which the ray is 40
    units beyond its closest approach to their middle (0, 0, 8)."""
    o, d = fam[0], fam[1]
    dd = (d * d).sum(axis=1)
    return (((np.array([0.0, 0.0, 8.0]) - o) * d).sum(axis=1) + 40.0 * np.sqrt(dd)) / dd


# ---- needle: ill-conditioned transforms ---------------------------------------------
NEEDLE_K = tuple(range(17))  # s = 10^(k/2)
NEEDLE_DIST = (0.01, 0.3, 2.0)  # origins, in bounding radii from the target
NEEDLE_CSG_K = (0, 5, 7, 8, 12, 16)  # the rungs of the csg form: either side of the host's bound, the first marked rungs, the last


# kind -> the first rung with an oracle hit point outside the padded bounding sphere (measured on
# the CPU from the oracle alone, test_cull_limits_ref.py; no rung below has one in its batch)
NEEDLE_FIRST_OUTSIDE = {abi.RT_SPHERE: 8, abi.RT_CUBE: 12, abi.RT_CYLINDER: 8, abi.RT_CONE: 8}


def needle_s(k):
    return 10.0 ** (k / 2.0)


def _needle(kind, mat, s):
    return (_CTOR[kind](mat).rotatez(33.0).rotatex(21.0).scale(1.0 / s, 1.0, s).rotatey(37.0).rotatex(-50.0)
            .translate(0.0, 0.0, 5.0))


def needle_scene(form, k):
    """Rung k: one object of every bounded kind under
    rotatez(33).rotatex(21).scale(1/s, 1, s).rotatey(37).rotatex(-50).translate(0, 0, 5),
    s = 10^(k/2), then well-conditioned fillers up to FORMS[form] bounded objects
    and a plane. "csg": the needles as leaves instead -- object 0 is (the needle
    sphere and 16 small spheres, united) minus the needle cube: 18 leaves, so the
    host groups them, the needles in a group of their own; object 1 is the needle
    cylinder intersected with a well-conditioned sphere around it -- then 12 fillers
    (a BVH) and the plane."""
    def make():
        s = needle_s(k)
        rng = random.Random(57)
        mats = _mats()
        nfill = 12 if form == "csg" else FORMS[form] - 4
        fill = [_CTOR[KINDS[i % 4]](mats[i % 3]).translate(rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(4, 9))
                .rotatex(rng.uniform(-60, 60)).rotatey(rng.uniform(-60, 60)).uscale(0.3 + 0.5 * rng.random())
                for i in range(nfill)]
        if form == "csg":
            small = [S.Sphere(mats[i % 3]).translate(rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(4, 9)).uscale(0.25)
                     for i in range(16)]
            cyl = _needle(abi.RT_CYLINDER, mats[2], s)
            m = cyl.transform_mat
            c = [m[r][1] * 0.5 + m[r][3] for r in range(3)]  # (the cylinder's bounding centre)
            around = S.Sphere(mats[0]).translate(c[0], c[1], c[2]).uscale(0.8 * s + 1.0)
            objs = [S.Difference(S.Union((_needle(abi.RT_SPHERE, mats[0], s),) + tuple(small)), _needle(abi.RT_CUBE, mats[1], s)),
                    S.Intersect(cyl, around)] + fill
        else:
            objs = [_needle(kd, mats[i % 3], s) for i, kd in enumerate(KINDS)] + fill
        objs.insert(6, S.Plane(mats[0]).translate(0.0, -6.0, 0.0))
        return S.convert(_args(objs))
    return _once(("needle", form, k), make)


def needles(p):
    """[(top-level object, rt_object)] of the needles of a needle scene: its first four
    objects, or on the csg form the needle leaves of its two composites."""
    tg = targets(p)
    if p.scene.objects[0].kind != abi.RT_CSG:
        return tg[:4]
    first = [ob for i, ob in tg if i == 0]
    return [(0, first[0]), (0, first[-1]), (1, [ob for i, ob in tg if i == 1][0])]


# rungs whose first batch holds fewer than 32 oracle hits of some kind get further batches (on the
# upper rungs the needle is thinner than the spacing of the doubles around it: 1 / s against
# 2^-52 * 5 s; measured on the CPU, asserted in test_cull_limits_ref.py)
NEEDLE_BATCHES = {14: 2, 15: 3}


def needle_rays(form, k):
    """Rung k's rays, NEEDLE_BATCHES batches of BATCH: per needle and distance of
    NEEDLE_DIST, origins that far (in the needle's padded bounding radii) from
    uniform object-space points of [-1, 1]^3 mapped through o2w, in a random
    direction; aimed at that point. -> (family, needle object index per ray)"""
    def make():
        p = needle_scene(form, k)
        g = np.random.default_rng([k, 7])
        need = needles(p)
        per = BATCH // (len(need) * len(NEEDLE_DIST))
        fo, fd, own = [], [], []
        for _ in range(NEEDLE_BATCHES.get(k, 1)):
            o, d = [], []
            for j in range(per):
                for dist in NEEDLE_DIST:
                    for i, ob in need:
                        m = o2w_of(ob)
                        _, R, _ = bound_of(ob)
                        tgt = (m @ np.append(g.uniform(-1.0, 1.0, 3), 1.0))[:3]
                        u = g.standard_normal(3)
                        u /= np.linalg.norm(u)
                        o.append(tgt + dist * R * u)
                        d.append(-u)
                        own.append(i)
            while len(o) < BATCH:  # (pad to a whole batch with copies)
                o.append(o[len(o) - 3 * len(need)])
                d.append(d[len(d) - 3 * len(need)])
                own.append(own[len(own) - 3 * len(need)])
            fo.append(np.array(o))
            fd.append(_lengths(np.array(d), BATCH // 2))
        return E._fam(np.concatenate(fo), np.concatenate(fd)), np.array(own)
    return _once(("needle-rays", form, k), make)


# ---- oracle tables ------------------------------------------------------------------
def table(key, p, fam):
    """query_ref.Table of `fam` on `p`, shared under `key`."""
    return _once(("table",) + tuple(key), lambda: Q.Table(p, fam[0], fam[1]))


def outside_pairs(p, Tb, how):
    """(ray, object) pairs with an oracle hit outside the object's padded bounding
    sphere -> rows (ray, object, kind, distance, padded radius, unpadded radius).
    how "line": the ray's line passes the centre beyond the radius (long double);
    "point": the hit point o + t d lies beyond it. Composites are left out."""
    rows = []
    objs = [(i, p.scene.objects[i]) for i in range(int(p.scene.num_objects))]
    objs = [(i, o) for i, o in objs if o.kind not in (abi.RT_PLANE, abi.RT_CSG)]
    bd = [bound_of(o) for _, o in objs]
    if how == "line":
        dist = line_distance(Tb.origins, Tb.dirs, np.array([b[0] for b in bd]))
    for q, (i, o) in enumerate(objs):
        hit = np.flatnonzero(Tb.ok[:, i] & (Tb.t[:, i] < INF))
        if how == "point" and len(hit):
            dq = point_distance(Tb.origins[hit], Tb.dirs[hit], Tb.t[hit, i], bd[q][0][None, :])
        else:
            dq = dist[hit, q] if len(hit) else []
        for r, x in zip(hit, dq):
            if x > bd[q][1]:
                rows.append((int(r), i, int(o.kind), float(x), bd[q][1], bd[q][2]))
    return rows


# ---- layout: what the BVH builder was never given ----------------------------------
LAYOUTS = ("arm", "arms", "concentric", "enclosed", "n11", "n12", "n13", "n17")
# (the BVH is used from 12 bounded objects: rt_kernel.hip BVH_MIN)
LAYOUT_BVH = {"arm": True, "arms": True, "concentric": True, "enclosed": True, "n11": False, "n12": True, "n13": True,
              "n17": True}
ARM_RATIO = 16.0


def _ball(kind, mat, c, s):
    """A primitive of `kind` at uniform scale s whose bounding centre is c."""
    lc = LC[kind]
    return _CTOR[kind](mat).translate(c[0] - s * lc[0], c[1] - s * lc[1], c[2] - s * lc[2]).uscale(s)


def _scatter(seed, n):
    """n random bounded objects as query_ref.mixed makes them, without duplicates."""
    rng = random.Random(seed)
    mats = _mats()
    return [_CTOR[KINDS[rng.randrange(4)]](mats[i % 3])
            .translate(rng.uniform(-2.5, 2.5), rng.uniform(-1.5, 1.8), rng.uniform(4, 8))
            .rotatex(rng.uniform(-90, 90)).rotatey(rng.uniform(-90, 90))
            .scale(0.3 + rng.random() * 0.5, 0.3 + rng.random() * 0.5, 0.3 + rng.random() * 0.5) for i in range(n)]


def layout_scene(name):
    """arm        13 objects, centres 16^k (cos k, sin k, 1), k = -8 .. 4, scale 0.2 * 16^k:
                  the SAH splits one object off per level
       arms       48 objects on three such arms (k = -11 .. 4) along +-x, +-y (the sign
                  alternates with k) and +z: the builder passes depth 40 and falls
                  back to median splits
       concentric 16 spheres of radii 1 .. 16 around (0, 0, 20) and an exact duplicate
                  of each: every centroid is equal
       enclosed   a sphere of scale 50 around the camera and a cluster of 14 small objects
       n11, n12, n13, n17   that many scattered objects of one seed (the BVH starts at
                  12; 17 makes leaves of 1 .. 4 objects)
    Each with one plane, which is a mirror."""
    def make():
        mats = _mats()
        if name == "arm":
            objs = [_ball(KINDS[(k + 8) % 4], mats[(k + 8) % 3],
                          tuple(ARM_RATIO ** k * v for v in (math.cos(k), math.sin(k), 1.0)), 0.2 * ARM_RATIO ** k)
                    for k in range(-8, 5)]
            plane_y = -3.0e5
        elif name == "arms":
            objs = []
            for k in range(-11, 5):
                sg = 1.0 if k % 2 == 0 else -1.0
                for a, axis in enumerate(((sg, 0.0, 0.0), (0.0, sg, 0.0), (0.0, 0.0, 1.0))):
                    objs.append(_ball(KINDS[(k + 11 + a) % 4], mats[(k + a) % 3],
                                      tuple(ARM_RATIO ** k * v for v in axis), 0.2 * ARM_RATIO ** k))
            plane_y = -3.0e5
        elif name == "concentric":
            objs = [S.Sphere(mats[r % 3]).translate(0.0, 0.0, 20.0).uscale(float(r)) for r in range(1, 17)]
            objs = objs + list(objs)
            plane_y = -18.0
        elif name == "enclosed":
            objs = _scatter(77, 14)
            objs.insert(3, S.Sphere(mats[0]).translate(0.0, 0.0, 8.0).uscale(50.0))
            plane_y = -4.0
        else:
            objs = _scatter(91, int(name[1:]))
            plane_y = -3.0
        objs.insert(2, S.Plane(mats[1]).translate(0.0, plane_y, 0.0))
        return S.convert(_args(objs, lights=[S.PointLight((5.0, 6.0, 0.0), (0.6,) * 3),
                                             S.PointLight((-3.0, 9.0, 4.0), (0.3, 0.3, 0.4))]))
    return _once(("layout", name), make)


def layout_rays(name):
    """BATCH rays on layout_scene(name), their classes in turn so every wave holds all:
    camera-like rays from the origin at every object (jittered within 1.3 radii:
    some miss), rays that start 1.5 .. 4 radii from an object's centre (inside
    whatever encloses it) towards it or away, and on arm / arms / concentric rays
    that start between consecutive shells towards the inner and the outer one.
    concentric: every second round over the objects excludes the object the
    oracle would report, so its duplicate answers. -> family"""
    def make():
        p = layout_scene(name)
        g = np.random.default_rng([len(name), int(p.scene.num_objects)])
        tg = [bound_of(ob) for _, ob in targets(p)]
        cen = [b[0] for b in tg]
        rad = [b[2] / math.sqrt(3.0) for b in tg]  # (uniform scales: the enclosing radius)
        n = len(tg)
        o, d = [], []

        def unit():
            u = g.standard_normal(3)
            return u / np.linalg.norm(u)

        shells = name in ("arm", "arms", "concentric")
        j = 0
        while len(o) < BATCH:
            i = j % n
            cls = (j // n) % (3 if shells else 2)
            j += 1
            if cls == 0:  # camera-like
                oo = np.zeros(3)
                tgt = cen[i] + 1.3 * rad[i] * g.uniform(0.0, 1.0) ** (1 / 3) * unit()
                if name == "concentric":
                    tgt = cen[i] + (rad[i] + 0.3) * _perp(g, cen[i] / np.linalg.norm(cen[i])) * g.uniform(0.0, 1.0)
                dv = tgt - oo
            elif cls == 1:  # from nearby, inside the scene
                u = unit()
                oo = cen[i] + g.uniform(1.5, 4.0) * rad[i] * u
                dv = cen[i] + 0.8 * rad[i] * unit() - oo
                if g.random() < 0.25:
                    dv = -dv
            else:  # between shell i and the next one out
                if name == "concentric":
                    r0 = rad[i] + 0.5
                    oo = cen[i] + r0 * unit()
                    dv = unit()
                else:
                    k = i if name == "arm" else i // 3
                    r0 = ARM_RATIO ** (k - (8 if name == "arm" else 11) + 0.5)
                    oo = r0 * np.abs(unit())
                    other = (i + (1 if name == "arm" else 3)) % n if g.random() < 0.5 else i
                    dv = cen[other] + 0.8 * rad[other] * unit() - oo
            o.append(oo)
            d.append(dv)
        fam = E._fam(np.array(o), _lengths(np.array(d), BATCH // 2))
        if name == "concentric":
            w = Q.Table(p, fam[0], fam[1]).winners()
            ex = np.where((np.arange(BATCH) // n) % 2 == 1, w, -1).astype(np.int32)
            fam = (fam[0], fam[1], fam[2], ex)
        return fam
    return _once(("layout-rays", name), make)


# ---- horizon: the render kernel's own far_shift sites --------------------------------
HORIZON_LIGHT = (0.0, 50.0, 100.0)


def horizon_scene():
    """24 x 16, depth 3: the view is so narrow (the reference's viewport is 2 / tan(fov / 2)
    wide) that the reflective ground plane is met 1e6 .. 3e7 units out. The plane
    is y = -30: the oracle's plane test rejects |d . n| < 1e-6, so no ray reaches
    a plane at depth h further out than 1e6 h, and y = -2 ends at 2e6. 16 spheres
    of radius 0.04 .. 0.3 sit 2 .. 32 units behind the point light on the line the
    shadow rays arrive along, below it by their radius plus 0.01 .. 0.5: the
    shadow rays are 3e-3 units apart there at the most, and from 1e6 .. 3e7
    units away the exact test's own error (2e-8 of the distance: 0.02 .. 0.6
    units) decides which of them a sphere shadows."""
    def make():
        mats = _mats()
        ground = S.material((0.7, 0.7, 0.6), 0.4, -1.0, 0.0, 1.0, 0.6, 0.4, 20.0)
        g = np.random.default_rng(5)
        objs = []
        for s in range(16):
            r = 0.04 + 0.26 * ((s * 7) % 16) / 15.0
            off = r + (0.01, 0.03, 0.08, 0.2, 0.5)[s % 5]
            a = -0.5 * math.pi + g.uniform(-0.5, 0.5)
            objs.append(S.Sphere(mats[s % 3]).translate(HORIZON_LIGHT[0] + off * math.cos(a),
                                                         HORIZON_LIGHT[1] + off * math.sin(a),
                                                         HORIZON_LIGHT[2] + 2.0 * (s + 1)).uscale(r))
        objs.insert(4, S.Plane(ground).translate(0.0, -30.0, 0.0))
        # vh = vw * 16 / 24 = 6e-5: the lower rows' v = 2e-6 .. 3e-5 reach y = -30 after 30 / v units
        fov = 2.0 * math.degrees(math.atan(2.0 / 9.0e-5))
        return S.convert(_args(objs, depth=3, lights=[S.PointLight(HORIZON_LIGHT, (0.8,) * 3)], fov=fov, width=24,
                               height=16))
    return _once("horizon", make)


def horizon_shadow_rays():
    """The frame's shadow rays as a family, from the oracle's own primary hits on the
    ground (trace_ref.camera_rays through query_ref.Table): origin point_world +
    1e-4 normal_world, direction to the light (tmax = 1 reaches it), the plane
    excluded. -> (family, distance of each origin from the light)"""
    def make():
        import trace_ref as T
        p = horizon_scene()
        rays = T.camera_rays(p, 0, int(p.scene.height)).reshape(-1)
        hits = Q.Table(p, rays["origin"], rays["dir"]).closest()
        hits = hits[hits["object"] >= 0]
        o = hits["point_world"] + 1e-4 * hits["normal_world"]
        d = np.array(HORIZON_LIGHT)[None, :] - o
        return E._fam(o, d, 1.0, hits["object"].astype(np.int32)), np.linalg.norm(d, axis=1)
    return _once("horizon-shadow", make)
