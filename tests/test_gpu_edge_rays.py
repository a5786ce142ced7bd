"""The ray-query, radiance and camera kernels on the edge rays of
tests/edge_rays.py against the oracle (needs an MI355X): directions with zero
components, far origins on an axis, rays within ulps of tangent, origins on a
surface, directions of length 2^-600 .. 2^600, and zero, NaN and infinite
components.

Bar: every field of every record equals the oracle's under edge_rays.same()
(==, or both NaN: no tolerance anywhere), every occlusion byte equals the
oracle predicate. What the families cover is asserted from the oracle's side
in tests/test_edge_rays_ref.py. The degenerate family F runs on its own last.
"""
import numpy as np
import pytest

import go_raytracer_amd as rt
import camera_ref as CR
import edge_rays as E
import oracle_bind
import query_ref as Q
import trace_ref as T
from test_gpu_query import gpu_closest, gpu_occluded
from test_gpu_trace import gpu_radiance

abi = rt.abi
pytestmark = pytest.mark.gpu

ACCEL = (0, abi.RT_ACCEL_CULL, abi.RT_ACCEL_BVH, abi.RT_ACCEL_BVH | abi.RT_ACCEL_CULL)
BVH_SCENES = ("lattice", "lattice-glass", "mixed12")
_tables = {}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0)
    yield c
    c.close()


def fam_of(key, name):
    """Family `key` ("A" .. "F") for scene `name`."""
    if key == "A":
        return E.family_a()
    if key == "B":
        return E.family_b()
    if key == "C":
        return E.family_c(name)[0]
    if key == "D":
        return E.family_d(name)[0]
    if key == "E":
        return E.family_e()[0]
    return E.family_f(E.packed(name).scene.num_objects)[0]


def table(key, name):
    """(family, its oracle table on scene `name`): shared, never modified."""
    if (key, name) not in _tables:
        fam = fam_of(key, name)
        _tables[(key, name)] = (fam, Q.Table(E.packed(name), fam[0], fam[1]))
    return _tables[(key, name)]


def mid_bound(Tb, fam):
    """A bound in the middle of things: just short of / just past the oracle's
    hit in turn, 6 world units where it misses."""
    t = E.winner_t(Tb, fam[2], fam[3])
    with np.errstate(all="ignore"):
        free = 6.0 / np.sqrt((fam[1] * fam[1]).sum(axis=1))
    return np.where(np.isfinite(t), t * np.where(np.arange(len(t)) % 2 == 0, 0.999, 1.001), free)


def set_scene(c, name):
    p = c.set_scene(E.packed(name))
    assert bool(c.scene_info() & abi.RT_INFO_BVH) == (name in BVH_SCENES), name
    assert bool(c.scene_info() & abi.RT_INFO_CSG) == (name in ("lattice", "lattice-glass", "c4csg")), name
    return p


def assert_miss_is_zero(got):
    raw = got.view(np.uint8).reshape(len(got), abi.HIT_DTYPE.itemsize)
    assert not raw[got["object"] < 0, :80].any()  # a miss: zero in every other field


def check_queries(c, Tb, fam, what, bounds=()):
    """Closest records and occlusion bytes of `fam` against the oracle table,
    the latter at the family's own tmax and at every bound of `bounds`."""
    o, d, tm, ex = fam
    got = gpu_closest(c, o, d, tm, ex)
    E.assert_same(got, Tb.closest(tm, ex), what)
    assert_miss_is_zero(got)
    for label, b in (("own tmax", tm),) + tuple(bounds):
        occ = gpu_occluded(c, o, d, b, ex)
        assert set(occ.tolist()) <= {0, 1}
        bad = np.flatnonzero(occ.astype(bool) != Tb.occluded(b, ex))
        assert len(bad) == 0, "%s, occluded at %s: %d of %d differ, first ray %d" % (what, label, len(bad), len(o), bad[0])


# 1. families A - E, closest and occluded, against the oracle table
@pytest.mark.parametrize("key,name", [("A", "lattice"), ("A", "mixed12"), ("A", "c4csg"), ("B", "lattice"),
                                      ("B", "mixed12"), ("C", "mixed12"), ("C", "lattice"), ("C", "c4csg"),
                                      ("D", "lattice"), ("D", "mixed12"), ("D", "c4csg"), ("D", "c3cone"),
                                      ("E", "lattice"), ("E", "mixed12"), ("E", "c4csg")])
def test_families_equal_the_oracle(ctx, key, name):
    fam, Tb = table(key, name)
    o, d, tm, ex = fam
    set_scene(ctx, name)
    mid = mid_bound(Tb, fam)
    occ = Tb.occluded(mid, ex)
    assert occ.sum() >= 20 and (~occ).sum() >= 20
    check_queries(ctx, Tb, fam, "%s on %s" % (key, name), (("a mid bound", mid),))
    if key == "E":  # the strict bound at the oracle's own t of each scaled ray, and one ulp past it
        t = E.winner_t(Tb, tm, ex)
        hit = np.isfinite(t)
        past = np.nextafter(t, np.inf)
        assert not Tb.occluded(t, ex).any() and np.array_equal(Tb.occluded(past, ex), hit)
        check_queries(ctx, Tb, (o, d, t, ex), "E on %s, tmax = t" % name)
        check_queries(ctx, Tb, (o, d, past, ex), "E on %s, tmax = t + 1 ulp" % name)


def batch_of(name, keys):
    """The families `keys` of scene `name` with the oracle's records, in family order."""
    fams, wants = [], []
    for key in keys:
        fam, Tb = table(key, name)
        fams.append(fam)
        wants.append(Tb.closest(fam[2], fam[3]))
    return fams, np.concatenate(wants)


# 2. all four accel settings return identical bytes for the interleaved batch
@pytest.mark.parametrize("name", ["lattice", "mixed12"])
def test_accel_settings_give_identical_bytes(name):
    fams, want = batch_of(name, "ABCDEF")
    (o, d, tm, ex), perm = E.interleave(fams, 11)
    mid = np.concatenate([mid_bound(table(k, name)[1], f) for k, f in zip("ABCDEF", fams)])[perm]
    c = rt.RenderContext(0)
    try:
        res = []
        for flags in ACCEL:
            c.set_accel(flags)
            c.set_scene(E.packed(name))
            assert bool(c.scene_info() & abi.RT_INFO_BVH) == bool(flags & abi.RT_ACCEL_BVH)
            res.append((gpu_closest(c, o, d, tm, ex).tobytes(), gpu_occluded(c, o, d, mid, ex).tobytes()))
        for r in res[1:]:
            assert r[0] == res[0][0] and r[1] == res[0][1]
        E.assert_same(np.frombuffer(res[0][0], dtype=abi.HIT_DTYPE), want[perm], name + ", accel 0")
    finally:
        c.close()


# 3. a ray's answer does not depend on which rays share its wave
@pytest.mark.parametrize("name", ["lattice", "c4csg"])
def test_wave_composition_does_not_matter(ctx, name):
    keys = "ABCDEF" if name == "lattice" else "ACDEF"
    fams, want = batch_of(name, keys)
    set_scene(ctx, name)
    # grouped: whole waves of one family (each padded to a multiple of 64 with its first ray)
    padded, keep = [], []
    for f in fams:
        n = len(f[0])
        pad = -n % 64
        padded.append(tuple(np.concatenate([v, np.repeat(v[:1], pad, axis=0)]) for v in f))
        keep.append(np.concatenate([np.ones(n, dtype=bool), np.zeros(pad, dtype=bool)]))
    go, gd, gt, gx = E.concat(padded)
    assert len(go) % 64 == 0
    grouped = gpu_closest(ctx, go, gd, gt, gx)[np.concatenate(keep)]
    # The rays at a composite's edge: unit-length family C rays grazing one, and family D's +-n
    # rays from a point on one. In the grouped batch they sit in waves of nothing but unit
    # directions, which vote unit_dir and search composites with csg_hit and its FP32 leaf and
    # group culls ...
    edge, at = [], 0
    for key, f in zip(keys, fams):
        sel = np.zeros(len(f[0]), dtype=bool)
        if key == "C":
            pairs = E.family_c(name)[1]
            sel[pairs[pairs[:, 1] == abi.RT_CSG][:, 3:5].ravel()] = True
            sel &= E.is_unit(f[1])
        if key == "D":
            own = E.family_d(name)[1]
            sel = np.array([E.packed(name).scene.objects[int(i)].kind == abi.RT_CSG for i in own]) & E.is_unit(f[1])
        edge.append(at + np.flatnonzero(sel))
        at += len(f[0])
    edge = np.concatenate(edge)
    where_grouped = np.flatnonzero(np.concatenate(keep))[edge]
    in_unit_wave = E.unit_waves(gd)[where_grouped // 64]
    assert in_unit_wave.sum() >= 300, (in_unit_wave.sum(), len(edge))
    # ... interleaved, every wave holds several families (unit and longer directions, near and
    # far origins, lanes that take the culls and lanes that pass them all): no wave is all unit,
    # so the same rays go through csg_search_nocull; and that batch reversed
    (o, d, tm, ex), perm = E.interleave(fams, 5)
    back = np.empty_like(perm)
    back[perm] = np.arange(len(perm))
    assert not E.unit_waves(d).any() and not E.unit_waves(d[::-1]).any()
    mixed = gpu_closest(ctx, o, d, tm, ex)[back]
    rev = gpu_closest(ctx, o[::-1].copy(), d[::-1].copy(), tm[::-1].copy(), ex[::-1].copy())[::-1][back]
    E.assert_same(grouped, want, name + ", grouped by family")
    E.assert_same(mixed, want, name + ", interleaved")
    E.assert_same(rev, want, name + ", interleaved and reversed")
    assert E.same(grouped, mixed) == [] and E.same(mixed, rev) == []


# 5. radiance: traceRay of the axis, far and degenerate rays
def padded_image(c, rad_bytes, n, samples, W):
    """image_from_radiance of the first n records padded with copies of record 0
    to whole rows of W pixels -> (image, the padded records)."""
    import torch
    total = -(-n // (W * samples)) * W * samples
    rec = np.frombuffer(rad_bytes, dtype=abi.RADIANCE_DTYPE)
    rec = np.concatenate([rec, np.repeat(rec[:1], total - n)])
    dev = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    img = c.image_from_radiance(dev, samples)
    torch.cuda.synchronize()
    return img.cpu().numpy(), rec.reshape(-1, W, samples)


def test_radiance_equals_the_reference(ctx):
    name = "lattice-glass"
    p = set_scene(ctx, name)
    o, d, tm, ex = E.radiance_rays()
    n = len(o)
    for depth in (1, 4):
        want = T.trace_many(p, o, d, depth, tm, ex)
        first = want  # (after the loop: depth 4)
        if depth == 1:
            assert (want["rays"] == 1).all()
        else:
            assert (want["rays"] > 1).sum() >= 150 and want["rays"].max() >= 8
            assert np.isnan(want["color"]).any(axis=1).sum() >= 4
        got = gpu_radiance(ctx, o, d, depth, tm, ex)
        E.assert_same(got, want, "%s depth %d" % (name, depth))
        for samples in (1, 4):
            img, rec = padded_image(ctx, got.tobytes(), n, samples, p.width)
            assert np.array_equal(img, T.image(rec, samples)), "depth %d, %d samples" % (depth, samples)
    # the query's own ray bounded at the oracle's t (strict: that winner is gone) and one ulp past it
    Tb = Q.Table(p, o, d)
    t = E.winner_t(Tb, tm, ex)
    for label, b in (("t", t), ("t + 1 ulp", np.nextafter(t, np.inf))):
        b = np.where(np.isfinite(t), b, tm)
        want = T.trace_many(p, o, d, 4, b, ex)
        if label == "t":
            hit = first["object"] >= 0
            assert hit.sum() >= 500 and (want["object"][hit] != first["object"][hit]).all()
        else:
            assert E.same(want, first) == []
        got = gpu_radiance(ctx, o, d, 4, b, ex)
        E.assert_same(got, want, "%s depth 4, tmax = %s" % (name, label))
        for samples in (1, 4):
            img, rec = padded_image(ctx, got.tobytes(), n, samples, p.width)
            assert np.array_equal(img, T.image(rec, samples)), "tmax = %s, %d samples" % (label, samples)


# 6. an orthographic camera looking down an axis: every primary ray has two zero components
@pytest.mark.parametrize("pose", ["+z", "-y"])
def test_orthographic_camera_down_an_axis(ctx, pose):
    import torch
    p = set_scene(ctx, "lattice-glass")
    kw = dict(eye=(0.5, 1.0, -2.0), look_at=(0.5, 1.0, 6.0), up=(0.0, 1.0, 0.0)) if pose == "+z" else \
        dict(eye=(0.5, 9.0, 5.5), look_at=(0.5, 0.0, 5.5), up=(0.0, 0.0, 1.0))
    cam = rt.RenderContext.camera(model="ortho", extent=14.0, samples=4, size=(32, 24), **kw)
    rays = CR.rays(p, cam)
    assert rays.shape == (24, 32, 4)
    dirs = rays["dir"].reshape(-1, 3)
    axis = 2 if pose == "+z" else 1
    assert (dirs[:, axis] == (1.0 if pose == "+z" else -1.0)).all() and (np.delete(dirs, axis, axis=1) == 0.0).all()
    flat = rays.reshape(-1)
    rad = T.trace_many(p, flat["origin"], flat["dir"], 0).reshape(rays.shape)
    assert len(set(rad["object"].reshape(-1).tolist())) >= 6 and (rad["rays"] > 1).sum() >= 100
    img, mean = CR.resolve(rad)
    got, gmean = ctx.render_camera(cam, mean=True)
    both_nan = np.isnan(gmean) & np.isnan(mean)
    assert ((gmean == mean) | both_nan).all(), "%d means differ" % (~((gmean == mean) | both_nan)).any(axis=2).sum()
    assert np.array_equal(got, img)
    torch.cuda.synchronize()


# 4. the degenerate family on its own, last in the file
@pytest.mark.parametrize("name", ["lattice", "mixed12", "c4csg"])
def test_degenerate_rays_equal_the_oracle_and_leave_the_context_usable(ctx, name):
    """Zero, denormal, huge, NaN and infinite directions, NaN, infinite and huge
    origins, tmax NaN / 0 / negative, exclude outside the scene: inputs the
    ABI accepts. Why every loop these rays reach ends whatever the values:

    - SceneSearch's object lists run i = 0 .. nobj - 1 and p = 0 .. nplanes - 1:
      integer counts from the scene. A ray's values only decide `test`.
    - The BVH walk visits a node once per pop or hand-over: bvh_next pushes at
      most one child per inner node and hands the other over, both only with a
      non-empty lane mask, and a leaf pushes nothing. The walk is a traversal of
      a finite tree and ends when the stack is empty. A lane whose values are not
      usable FP32 numbers (nocull) sets its bit in every mask, which visits more
      nodes, never a node twice. The stack cannot overflow: the host uses the
      BVH only when its depth + 2 < BVH_STACK, and the pushes of a path are
      bounded by that depth whatever the masks.
    - far_shift: straight-line code; a lane with NaN or inf in it either keeps
      its origin (nocull: `fsh` is false for it) or gets a NaN interval, for
      which !(tn <= tf) retires it from the culls only.
    - object_hit and leaf_interval are straight-line code per kind.
    - csg_hit, csg_hit_all and csg_search_nocull each pick the smallest end
      point te with te > tc among at most 2 * leaves values and then set tc =
      te: tc strictly increases over a finite set, a NaN end point fails both
      comparisons and is never picked, +inf is never below te = +inf, so after
      at most 2 * leaves rounds je < 0 returns. csg_hit's far-origin shift is
      taken only for t0 > 0 (false for NaN). A NaN or infinite direction makes
      the wave vote !unit_dir (|d|^2 - 1 <= 1e-9 is false), so csg_hit itself
      sees non-finite values in the origin only, where may_hit's compare is
      false and the leaf is skipped.
    - The radiance kernel's outer loop: a lane's tree has at most depth - 1
      frames, each frame is left after its one or two children, every search
      above ends, and tickets only increase up to n. A NaN ray misses (t < tmax
      is false) and returns the background; a hit with a NaN normal (the cone's
      apex) sends NaN children, which miss. go_pow's loops count the bits of
      the material's integer exponent, not of a ray's value.
    """
    fam, Tb = table("F", name)
    set_scene(ctx, name)
    check_queries(ctx, Tb, fam, "F on %s" % name, (("tmax 6", 6.0), ("tmax 1e-199", 1e-199)))
    if name != "lattice":
        return
    # the context still answers family A and still renders the scene
    famA, TA = table("A", name)
    check_queries(ctx, TA, famA, "A on lattice after F")
    p = E.packed(name)
    ref, ost = oracle_bind.render_rows(p)
    ctx.read_stats(reset=True)
    img = ctx.render()
    st = ctx.read_stats(reset=True)
    assert np.array_equal(img, ref), "%d pixels differ" % (img != ref).any(axis=2).sum()
    assert st.as_dict() == ost.as_dict()
