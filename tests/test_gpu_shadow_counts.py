"""inShadow's per-kind test counts in the specialised small-scene kernels
(the GPU tests need an MI355X).

Those kernels (compile-time objects and lights, rt_render.h SC_BUILD) form the
reference's counts -- #{i < first occluder + 1, i != hit} per kind
(raytracer.go:411-429) -- from packed literal prefix words: 8-bit fields per
SHADE pass, 16-bit per-lane accumulators, per-wave u64 totals in LDS after a
flush. What can go wrong is a field's position (which kinds are present, four
or five of them), the prefix at the first occluder (index 0, a middle one, the
last, none), the hit's own exclusion (hit below or above the occluder), a
carry between fields (eight objects of one kind, eight lights) and the flush.
Every case is the CPU oracle's frame and counters (tests/oracle_bind.py), bytes
and every rt_stats field, with ==.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import go_raytracer_amd as rt
import oracle_bind

S = rt.scene
A = rt.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H, DEPTH = 70, 30, 3  # (70: not a multiple of the 8-pixel tile)

MATTE = S.material((0.8, 0.5, 0.3), 0.0, 0.0, 0.0, 0.0, 0.9, 0.3, 8.0)
SHINY = S.material((0.6, 0.7, 0.9), 0.5, 0.0, 0.0, 0.0, 0.7, 0.6, 30.0)
GLASS = S.material((0.9, 0.9, 1.0), 0.3, 0.0, 0.7, 1.4, 0.6, 0.9, 40.0)
FLOOR = S.material((0.7, 0.7, 0.7), 0.35, 0.0, 0.0, 0.0, 1.0, 0.1, 5.0)
GREY = (0.5, 0.5, 0.5)
# up to eight lights around and above the objects; LOW grazes along the rows
LOW = S.PointLight((8.0, 2.5, 6.0), GREY)
LIGHTS = [S.PointLight(p, GREY) for p in ((5.0, 5.0, 0.0), (-5.0, 5.0, 0.0), (5.0, 5.0, 10.0), (-5.0, 5.0, 10.0),
                                          (0.0, 6.0, 5.0), (-8.0, 2.5, 6.0), (0.0, 3.0, -1.0))] + [LOW]
KIND = {S.Sphere: A.RT_SPHERE, S.Plane: A.RT_PLANE, S.Cube: A.RT_CUBE, S.Cylinder: A.RT_CYLINDER, S.Cone: A.RT_CONE}


def args(objs, lights, w=W, h=H):
    return S.RenderArgs(ambient=(0.1, 0.1, 0.1), lights=list(lights), scene=S.Union(tuple(objs)), depth=DEPTH,
                        fov=90.0, width=w, height=h, file="t.ppm", bg_start=(0.0, 0.0, 0.0), bg_end=(0.5, 0.7, 1.0))


def plane():
    return S.Plane(FLOOR).translate(0.0, -1.0, 0.0)


def sphere(x, y, z, r, m=MATTE):
    return S.Sphere(m).translate(x, y, z).uscale(r)


def row(n):
    """n spheres in a row along x over the plane. The low light at +x (LOW)
    throws each one's shadow on the plane and on the neighbours behind it, so
    the first occluder of a shadow ray is any sphere of the row or none, and a
    sphere's own hits lie on both sides of their occluders."""
    return [sphere(-3.0 + 6.0 * i / max(1, n - 1), -0.2, 6.0, 0.45, (MATTE, SHINY, GLASS)[i % 3]) for i in range(n)]


def five_kinds():
    return [plane(),
            sphere(-2.2, -0.4, 5.0, 0.6, GLASS),
            S.Cube(SHINY).translate(-0.9, -1.0, 5.5).rotatey(25.0).uscale(1.0),
            S.Cylinder(GLASS).translate(1.4, -1.0, 5.0).scale(0.5, 1.3, 0.5),
            S.Cone(MATTE).translate(3.0, 0.5, 6.0).scale(0.55, -1.5, 0.55)]


SCENES = {
    # one object: nothing but the hit itself, which inShadow skips
    "one": lambda: args([sphere(0.0, 0.0, 4.0, 1.0, SHINY)], LIGHTS[:1]),
    "two": lambda: args([plane(), sphere(0.0, -0.2, 4.0, 0.8, GLASS)], LIGHTS[:4]),
    # five kinds present: the fifth field lies in the second word
    "five": lambda: args(five_kinds(), LIGHTS[:4]),
    "five_rev": lambda: args(five_kinds()[::-1], LIGHTS[:4]),
    # eight of one kind (the largest prefix) under eight lights (the largest
    # sum of a pass): the ground is a sphere too
    "eight_spheres": lambda: args([sphere(0.0, -1001.0, 5.0, 1000.0, FLOOR)] + row(7), LIGHTS),
    # the plane below a row of seven, one low light: occluder 1..7 or none,
    # the plane's hits below every occluder; reversed, the plane is last: its
    # hits above every occluder, and the occluders from index 0; then the
    # plane in the middle of two rows
    "row": lambda: args([plane()] + row(7), [LOW]),
    "row_rev": lambda: args(row(7)[::-1] + [plane()], [LOW]),
    "row_mid": lambda: args(row(4) + [plane()] + [sphere(-2.0 + 2.0 * i, 0.9, 5.0, 0.3) for i in range(3)],
                            [LOW, LIGHTS[4]]),
    "c3": lambda: rt.configs.c3(width=96, height=54),
    "c3cone": lambda: rt.configs.c3cone(width=96, height=54),
}

SCHEDULES = {"serial": A.RT_SCHED_PIXEL, "quads": A.RT_SCHED_QUADS, "pairs": A.RT_SCHED_PAIRS}
# every scene in every schedule with the default accel; brute force
# (rt_set_accel(0)) for every scene serially, and in the other schedules where
# the tallies take two words
CASES = [(s, k, None) for s in sorted(SCENES) for k in SCHEDULES]
CASES += [(s, "serial", 0) for s in sorted(SCENES)] + [("five", k, 0) for k in ("quads", "pairs")]

_refs = {}


def reference(name):
    """The scene, and the oracle's frame and counters: once per scene."""
    if name not in _refs:
        packed = S.convert(SCENES[name]())
        ref, ost = oracle_bind.render_rows(packed)
        ref.setflags(write=False)
        _refs[name] = (packed, ref, ost.as_dict())
    return _refs[name]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_count_shadow_tests_of_every_kind_they_hold(name):
    """(No device: the oracle alone.) Each field of the packed words is only
    checked by a scene that counts tests of its kind."""
    objs = S.flatten(SCENES[name]().scene)
    ost = reference(name)[2]
    assert ost["shaded_hits"] > 0 and ost["shadow_rays"] > 0
    for k in range(A.RT_NUM_KINDS):
        held = any(KIND[type(o)] == k for o in objs)
        # (a lone object is the hit itself, which inShadow skips)
        assert (ost["shadow_tests"][k] > 0) == (held and len(objs) > 1), (name, k, ost["shadow_tests"])


def test_row_scenes_end_at_different_occluders():
    """(No device.) The same eight objects in another order count other
    totals: the counts depend on where the first occluder and the hit stand."""
    a, b = reference("row")[2], reference("row_rev")[2]
    assert a["shadow_rays"] == b["shadow_rays"] and a["shadow_tests"] != b["shadow_tests"]
    # no occluder at all would count (objects - 1) tests per shadow ray
    for st in (a, b):
        assert sum(st["shadow_tests"]) < 7 * st["shadow_rays"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = rt.RenderContext(0, specialize=True)
    c.set_work_sharing(A.RT_SHARE_OFF)
    yield c
    c.close()


def render(c, packed):
    c.set_scene(packed)
    assert c.specialized()[0]
    c.read_stats(reset=True)
    img = c.render()
    return img, c.read_stats(reset=True).as_dict()


@pytest.mark.gpu
@pytest.mark.parametrize("name,sched,accel", CASES, ids=["%s-%s-%s" % (s, k, "default" if a is None else "accel%d" % a)
                                                         for s, k, a in CASES])
def test_specialised_kernel_matches_oracle(ctx, name, sched, accel):
    packed, ref, ost = reference(name)
    try:
        if accel is not None:
            ctx.set_accel(accel)
        ctx.set_schedule(SCHEDULES[sched])
        img, st = render(ctx, packed)
    finally:
        ctx.set_schedule(A.RT_SCHED_AUTO)
        if accel is not None:
            ctx.set_accel(A.RT_ACCEL_BVH | A.RT_ACCEL_CULL)
    print("%s %s: shadow tests gpu %s oracle %s" % (name, sched, st["shadow_tests"], ost["shadow_tests"]))
    assert np.array_equal(img, ref), "%d pixels differ" % int((img != ref).any(axis=-1).sum())
    assert st == ost


CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from __graft_entry__ import load_package
rt = load_package()
import test_gpu_shadow_counts as T
c = rt.RenderContext(0, specialize=True)
c.set_work_sharing(rt.abi.RT_SHARE_OFF)
out = {}
for name in sys.argv[1:]:
    img, st = T.render(c, T.S.convert(T.SCENES[name]()))
    out[name] = {"sha256": hashlib.sha256(img.tobytes()).hexdigest(), "stats": st}
c.close()
print("RESULT " + json.dumps(out))
''' % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.gpu
def test_forced_flushes_count_the_same(ctx):
    """A flush every second SHADE pass (-DRT_SC_FLUSH=2, compiled in a fresh
    process: the library snapshots the environment at load): c3 and the
    five-kind scene count what the oracle counts, and what the default build
    (a flush every ~1000 passes and at exit) counts."""
    names = ["c3", "five"]
    env = dict(os.environ, RT_SPEC_EXTRA_FLAGS="-DRT_SC_FLUSH=2")
    r = subprocess.run([sys.executable, "-c", CHILD] + names, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    for name in names:
        packed, ref, ost = reference(name)
        img, st = render(ctx, packed)
        assert got[name]["stats"] == ost, name
        assert got[name]["stats"] == st, name
        assert got[name]["sha256"] == hashlib.sha256(ref.tobytes()).hexdigest(), name
