"""The frame stack on both sides of its LDS / HBM split (needs an MI355X).

A lane's frame cores live in LDS for the first `lds_levels` recursion levels
and in HBM below (rt_render.h core_load / core_store; the launch plan picks
the count from the LDS left over at full occupancy). RT_LDS_LEVELS caps the
count, so 1 and 2 put lanes of one wave on both sides of the split, 0 puts
every frame in HBM, and unset is the product's plan. Where a frame lives may
not change a byte or a counter: every render is compared with the CPU oracle
(tests/oracle_bind.py).

The library reads its environment once, at load, so every value runs in a
fresh child process. The children run one after another; after one that
failed the rest do not start.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import go_raytracer_amd as rt
import oracle_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SCENES = {
    # depth 6, a glass cylinder: frames with both children, FL_STAGE and
    # pending rays at every level
    "c3": lambda: rt.configs.c3(width=96, height=64),
    "c2": lambda: rt.configs.c2(width=96, height=64),  # a glass sphere, depth 4
    "canned": lambda: rt.configs.canned(width=95, height=60),  # depth 7
    "c4csg": lambda: rt.configs.c4csg(width=96, height=64),  # depth 8, a CSG composite of glass
}

# Renders the scenes named in argv against the stored oracle frames: PLAIN
# scenes with the generic and the specialised kernel; SHARING scenes with the
# specialised kernel, the device-wide board, quads then pairs; NOSHARE scenes
# with the specialised kernel, sharing off.
CHILD = r'''
import json, os, sys
from concurrent.futures import ThreadPoolExecutor
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from __graft_entry__ import load_package
rt = load_package()
A = rt.abi
refdir, jobs = sys.argv[1], sys.argv[2:]
ok = True
def check(what, ctx, name):
    global ok
    ref = np.load(os.path.join(refdir, name + ".npy"))
    with open(os.path.join(refdir, name + ".json")) as f:
        ost = json.load(f)
    ctx.read_stats(reset=True)
    img = ctx.render()
    st = ctx.read_stats(reset=True).as_dict()
    bad = int((img != ref).any(axis=-1).sum())
    same = st == ost
    print("%%s: %%d pixels differ, counters %%s" %% (what, bad, "equal" if same else "DIFFER: %%s oracle %%s" %% (st, ost)))
    ok = ok and bad == 0 and same
def scene(name):
    w, h = {"canned": (95, 60)}.get(name, (96, 64))
    return rt.scene.convert(rt.configs.CONFIGS[name](width=w, height=h))
todo = []
for job in jobs:
    mode, name = job.split(":")
    c = rt.RenderContext(0, specialize=True)
    if mode == "SHARING":
        c.set_work_sharing(A.RT_SHARE_DEVICE)
        c.set_schedule(A.RT_SCHED_QUADS)
    elif mode == "NOSHARE":
        c.set_work_sharing(A.RT_SHARE_OFF)
    todo.append((mode, name, c, scene(name)))
# (the specialised kernels compile side by side: each in the helper's process)
with ThreadPoolExecutor(len(todo)) as ex:
    list(ex.map(lambda t: t[2].set_scene(t[3]), todo))
for mode, name, c, packed in todo:
    print("scene %%s" %% name, file=sys.stderr, flush=True)
    if mode == "PLAIN":
        g = rt.RenderContext(0)
        g.set_scene(packed)
        check(name + " generic", g, name)
        g.close()
        check(name + " specialised", c, name)
    elif mode == "SHARING":
        assert c.scene_info() & A.RT_INFO_SHARE_DEVICE
        check(name + " device-wide sharing, quads", c, name)
        c.set_schedule(A.RT_SCHED_PAIRS)
        c.set_scene(packed)
        assert c.scene_info() & A.RT_INFO_SHARE_DEVICE
        check(name + " device-wide sharing, pairs", c, name)
    else:
        assert not c.scene_info() & A.RT_INFO_WAVEFRONT
        check(name + " specialised, sharing off", c, name)
    c.close()
print("frame levels ok" if ok else "frame levels MISMATCH")
''' % (ROOT, os.path.join(ROOT, "tests"))

PLAIN = ["PLAIN:c3", "PLAIN:c2", "PLAIN:canned"]
# (id, RT_LDS_LEVELS or None, jobs)
CHILDREN = [
    ("levels0", "0", PLAIN),
    ("levels1", "1", PLAIN),
    ("levels2", "2", PLAIN),
    ("default", None, PLAIN),
    ("sharing_default", None, ["SHARING:c4csg"]),
    ("c4csg_levels1", "1", ["NOSHARE:c4csg"]),
]

_failed = []  # the first child that failed: nothing more starts on the device after it


@pytest.fixture(scope="module")
def refdir(tmp_path_factory):
    """The oracle's frame and counters of every scene, once, for all children."""
    d = tmp_path_factory.mktemp("frame_levels")
    for name, make in SCENES.items():
        ref, ost = oracle_bind.render_rows(rt.scene.convert(make()))
        np.save(str(d / (name + ".npy")), ref)
        (d / (name + ".json")).write_text(json.dumps(ost.as_dict()))
    return str(d)


@pytest.mark.parametrize("case", CHILDREN, ids=[c[0] for c in CHILDREN])
def test_frames_on_both_sides_of_the_split_match_oracle(refdir, case):
    cid, levels, jobs = case
    if _failed:
        pytest.fail("not started: the child %s failed before it" % _failed[0])
    env = dict(os.environ, RT_DEBUG_LAUNCH="1")
    env.pop("RT_LDS_LEVELS", None)
    if levels is not None:
        env["RT_LDS_LEVELS"] = levels
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, refdir] + jobs, env=env, capture_output=True, text=True,
                           timeout=180)
    except subprocess.TimeoutExpired:
        _failed.append(cid)
        raise
    print(r.stdout)
    # the plan each launch ran with, per scene: "[launch] ... frame cores N levels), frames F"
    plans, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"scene (\w+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"frame cores (\d+) levels\), frames (\d+)", line)
        if m and cur:
            plans.setdefault(cur, set()).add((int(m.group(1)), int(m.group(2))))
    print("launch plans (LDS levels, frames) with RT_LDS_LEVELS=%s: %s" % (levels, {k: sorted(v) for k, v in plans.items()}))
    if r.returncode != 0 or "frame levels ok" not in r.stdout:
        _failed.append(cid)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "frame levels ok" in r.stdout, r.stdout + r.stderr
    # the cap reached the launch plan: every launch kept exactly that many
    # levels in LDS (each scene has more frames, and LDS has room for two)
    assert plans, r.stderr
    for name, seen in plans.items():
        for n, frames in seen:
            assert 0 <= n <= frames
            if levels is not None:
                assert n == int(levels) and n < frames, (name, n, frames)
