"""Throughput of the batched ray queries (rt_query_closest_async /
rt_query_occluded_async / rt_query_radiance_async), recorded and not targeted:
one JSON line per case.

1920x1080 camera rays, one per pixel through a seeded position inside the
pixel, from the origin through a viewport of the scene's field of view at
z = 1 (the reference's camera, raytracer.go:589-609), against c3, c4csg and the
full 100 k-sphere c5. Closest mode: unit directions, no bound. Occluded mode:
the same rays with directions that end on the far plane z = 20 and tmax = 1
(so these directions are not unit length). Timing: device events around 20
launches after 3 warm-ups. Needs a HIP device: there is no CPU path.

Radiance mode: the scene's own camera rays at 1920x1080 x 4 samples, produced
on the device by rt_query_camera_rays_async, traced at the scene's depth;
Mrays/s over the rays traced (the sum of the records' `rays`: primary and
secondary, as the renderer counts them). The line also carries the time of
rt_render_rows_async for the same frame on the same context (specialisation
off: the generic megakernel, which traces the same rays) and the ratio of the
two. Device events around 5 launches after 1 warm-up.

usage: python scripts/query_rate.py [--configs c3,c4csg,c5] [--modes closest,occluded,radiance] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

W, H, ZFAR, WARMUP, LAUNCHES = 1920, 1080, 20.0, 3, 20
RAD_WARMUP, RAD_LAUNCHES = 1, 5


def timed(torch, launch, warmup, launches):
    for _ in range(warmup):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def radiance_line(torch, abi, ctx, name, seed):
    """The scene's camera rays (4 per pixel) through rt_query_radiance_async,
    beside the generic render of the same frame."""
    n = W * H * 4
    rays = torch.empty(n * abi.RAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(n * abi.RADIANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    img = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    ctx.camera_rays_async(0, H, rays)
    ms = timed(torch, lambda: ctx.query_radiance_async(rays, out), RAD_WARMUP, RAD_LAUNCHES)
    traced = int(out.view(torch.int32).view(n, 8)[:, 7].sum(dtype=torch.int64).item())
    ctx.read_stats(reset=True)
    render_ms = timed(torch, lambda: ctx.render_rows_async(0, H, img), RAD_WARMUP, RAD_LAUNCHES)
    st = ctx.read_stats(reset=True)
    frames = RAD_WARMUP + RAD_LAUNCHES
    render_traced = (int(st.primary_rays) + int(st.secondary_rays)) // frames
    same = bool(torch.equal(ctx.image_from_radiance(out, 4), img))
    return {"metric": "query_rate", "config": name, "mode": "radiance", "rays": n, "rays_traced": traced,
            "depth": int(ctx.packed.scene.depth), "lanes": ctx.radiance_lanes(),
            "objects": int(ctx.packed.scene.num_objects), "bvh": bool(ctx.scene_info() & abi.RT_INFO_BVH),
            "ms_per_launch": round(ms, 4), "value": round(traced / ms / 1e3, 2), "unit": "Mrays/s",
            "render_generic_ms": round(render_ms, 4), "render_rays_traced": render_traced,
            "render_specialized": ctx.specialized()[0], "render_over_radiance": round(render_ms / ms, 4),
            "image_equals_render": same, "launches": RAD_LAUNCHES, "warmup": RAD_WARMUP, "seed": seed}


def camera_rays(fov_deg, seed):
    g = np.random.default_rng(seed)
    vw = 2.0 * math.tan(math.radians(fov_deg) / 2.0)
    vh = vw * H / W
    x = (np.arange(W)[None, :] + g.random((H, W))) / W * vw - vw / 2.0
    y = vh / 2.0 - (np.arange(H)[:, None] + g.random((H, W))) / H * vh
    d = np.stack([x, y, np.ones_like(x)], axis=-1).reshape(-1, 3)
    return np.zeros_like(d), d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c4csg,c5")
    ap.add_argument("--modes", default="closest,occluded,radiance")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("query_rate: no HIP device visible (the queries have no CPU path)")
    abi = pkg.abi
    ctx = pkg.RenderContext(0)
    lines = []
    for name in args.configs.split(","):
        rargs = pkg.configs.CONFIGS[name](width=W, height=H)
        ctx.set_scene(rargs)
        o, d = camera_rays(rargs.fov, args.seed)
        n = len(o)
        unit = d / np.linalg.norm(d, axis=1)[:, None]
        far = d * ZFAR  # d.z == 1: ends on z = ZFAR at t = 1
        hits = torch.empty(n * abi.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        occ = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        modes = args.modes.split(",")
        for mode, dirs, tmax in (("closest", unit, None), ("occluded", far, 1.0)):
            if mode not in modes:
                continue
            _, rays = ctx._upload_rays(o, dirs, tmax, None)
            launch = (lambda: ctx.query_closest_async(rays, hits)) if mode == "closest" else \
                (lambda: ctx.query_occluded_async(rays, occ))
            ms = timed(torch, launch, WARMUP, LAUNCHES)
            if mode == "closest":
                answered = int((hits.cpu().numpy().view(abi.HIT_DTYPE)["object"] >= 0).sum())
            else:
                answered = int(occ.sum().item())
            lines.append({"metric": "query_rate", "config": name, "mode": mode, "rays": n,
                          "objects": int(ctx.packed.scene.num_objects), "bvh": bool(ctx.scene_info() & abi.RT_INFO_BVH),
                          "ms_per_launch": round(ms, 4), "value": round(n / ms / 1e3, 2), "unit": "Mrays/s",
                          "hits" if mode == "closest" else "occluded": answered, "launches": LAUNCHES,
                          "warmup": WARMUP, "seed": args.seed})
            print(json.dumps(lines[-1]), flush=True)
        if "radiance" in modes:
            del hits, occ
            lines.append(radiance_line(torch, abi, ctx, name, args.seed))
            print(json.dumps(lines[-1]), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
