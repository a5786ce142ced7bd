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

Camera mode (not in the default modes; writes profiles/camera/camera_rate.jsonl
unless --out says otherwise): the zero camera at 1920x1080 x 4 samples through
rt_render_camera_async (fused: no ray array, chunked sample buffer, resolve
kernel) beside the three-step route it replaces -- camera_rays_async +
query_radiance_async + image_from_radiance -- three runs each of device
events around 5 frames after 1 warm-up, with the times of each chunk's trace +
resolve, and beside rt_render_rows_async generic and specialised. On c3 also
S = 1, 4, 16, 64. Every line asserts that the fused bytes equal render()'s.

Adaptive mode (not in the default modes; writes
profiles/adaptive/adaptive_rate.jsonl unless --out says otherwise): the zero
camera at 1920x1080 with a cap of 64 samples through
rt_render_camera_adaptive_async, min_samples 4, tolerances 0.002 and 0.005,
beside the fixed 64-sample rt_render_camera_async of the same build -- three
runs each of device events around 5 frames after 1 warm-up. Per line: both
times, the mean samples per pixel and the histogram of the counts, passes x
chunks launched, and rt_ssim_rgba8 and the largest byte difference against the
fixed 64-sample frame; also the time of the same call at an infinite
tolerance (every pass after the first is empty: what the launches alone cost)
and of the fixed render at min_samples.

Aov mode (not in the default modes; writes profiles/aov/aov_rate.jsonl unless
--out says otherwise): the zero camera's five feature buffers at 1920x1080 x 4
and x 64 samples through rt_render_camera_aov_async beside the materialised
route -- camera_rays_ex_async + query_closest_async + a reduction in torch in
sample order -- median of 5 timed repeats each after a warm-up; the margin of
the comparison is the spread of the route's own repeats. Each line also says
whether the route's buffers equal the fused call's.

Denoise mode (same file): rt_denoise_atrous_async, 5 iterations, all terms on
with the default sigmas, on a 4-sample thin-lens frame of the scene and its
feature buffers at 1920x1080 and 3840x2160: ms per iteration beside the memory
floor (104 B per pixel at 8 TB/s) and the FP64 floor (1.1 k operations per
pixel at 78.6 TFLOP/s); at 1080p also the mean squared error of the raw and of
the denoised mean against a 256-sample mean for a few sigma sets.

Variance mode (not in the default modes; writes
profiles/variance/variance_rate.jsonl unless --out says otherwise), device
events, one warm-up, the median of 5: rt_render_camera_var_async with and
without d_var at 1920x1080 x 4 and x 64 samples, and
rt_render_camera_adaptive_var_async likewise (tolerance 0.005, cap 64);
rt_denoise_atrous_async beside rt_denoise_atrous_var_async per call and per
iteration at 1920x1080 and 3840x2160, with the memory floor (104 + 16 B per
pixel at 8 TB/s) and the FP64 floor (1.2 k operations per pixel); and the mean
squared error against a 256-sample mean of the 4-sample thin-lens frame: raw,
the plain filter at its defaults and colour-only, the variance-guided filter
at 1, 2, 4 and 8 standard deviations with and without the guides, and one
adaptive frame (tolerance 0.005, cap 64) filtered with its own variance.

usage: python scripts/query_rate.py [--configs c3,c4csg,c5]
                                    [--modes closest,occluded,radiance,camera,adaptive,aov,denoise,variance] [--out FILE]
"""
import argparse
import ctypes
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


def camera_line(torch, abi, ctx, name, seed):
    """The fused camera render of the zero camera beside the three-step route
    and the megakernel; on c3 also other sample counts."""
    img = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    fused = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    ctx.set_specialize(False)
    ctx.render_rows_async(0, H, img)
    zero = ctx.camera()
    fused_ms = [timed(torch, lambda: ctx.render_camera_async(zero, 0, H, rgba=fused), RAD_WARMUP, RAD_LAUNCHES)
                for _ in range(3)]
    torch.cuda.synchronize()
    same = bool(torch.equal(fused, img))
    assert same, "%s: the fused zero-camera frame differs from render()" % name
    chunks = ctx.render_camera_chunks(zero)
    # the rows that cover each chunk, rendered on their own (one chunk each), to show the tails
    cpix = 2097152 // 4  # pixels per chunk at 4 samples (include/rt_abi.h)
    chunk_ms = []
    for k in range(chunks):
        y0 = (k * cpix) // W
        y1 = min(H, -(-((k + 1) * cpix) // W))
        band = torch.empty((y1 - y0, W, 4), dtype=torch.uint8, device="cuda:0")
        chunk_ms.append(round(timed(torch, lambda: ctx.render_camera_async(zero, y0, y1, rgba=band), RAD_WARMUP,
                                    RAD_LAUNCHES), 4))
        del band
    n = W * H * 4
    rays = torch.empty(n * abi.RAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(n * abi.RADIANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    res = {}

    def three_step():
        ctx.camera_rays_async(0, H, rays)
        ctx.query_radiance_async(rays, out)
        res["img"] = ctx.image_from_radiance(out, 4)

    route_ms = [timed(torch, three_step, RAD_WARMUP, RAD_LAUNCHES) for _ in range(3)]
    route_same = bool(torch.equal(res["img"], img))
    traced = int(out.view(torch.int32).view(n, 8)[:, 7].sum(dtype=torch.int64).item())
    del rays, out, res
    generic_ms = timed(torch, lambda: ctx.render_rows_async(0, H, img), RAD_WARMUP, RAD_LAUNCHES)
    ctx.set_specialize(True)
    ctx.render_rows_async(0, H, img)
    torch.cuda.synchronize()
    spec_on = bool(ctx.specialized()[0])
    spec_ms = timed(torch, lambda: ctx.render_rows_async(0, H, img), RAD_WARMUP, RAD_LAUNCHES)
    ctx.set_specialize(False)
    fm, rm = min(fused_ms), min(route_ms)
    line = {"metric": "camera_rate", "config": name, "mode": "camera", "width": W, "height": H, "samples": 4,
            "depth": int(ctx.packed.scene.depth), "objects": int(ctx.packed.scene.num_objects),
            "bvh": bool(ctx.scene_info() & abi.RT_INFO_BVH), "chunks": chunks, "rays_traced": traced,
            "fused_ms": [round(v, 4) for v in fused_ms], "route_ms": [round(v, 4) for v in route_ms],
            "route_spread_ms": round(max(route_ms) - min(route_ms), 4),
            "fused_over_route": round(fm / rm, 4), "chunk_rows_ms": chunk_ms,
            "value": round(traced / fm / 1e3, 2), "unit": "Mrays/s",
            "render_generic_ms": round(generic_ms, 4), "render_specialized_ms": round(spec_ms, 4),
            "render_specialized": spec_on, "generic_over_fused": round(generic_ms / fm, 4),
            "specialized_over_fused": round(spec_ms / fm, 4), "fused_equals_render": same,
            "route_equals_render": route_same, "launches": RAD_LAUNCHES, "warmup": RAD_WARMUP, "runs": 3, "seed": seed}
    if name == "c3":
        sweep = []
        for S in (1, 4, 16, 64):
            cam = ctx.camera(samples=S)
            ms = timed(torch, lambda: ctx.render_camera_async(cam, 0, H, rgba=fused), RAD_WARMUP, RAD_LAUNCHES)
            sweep.append({"samples": S, "ms": round(ms, 4), "chunks": ctx.render_camera_chunks(cam),
                          "primary_Mrays_per_s": round(W * H * S / ms / 1e3, 2)})
        line["samples_sweep"] = sweep
    return line


ADAPT_CAP, ADAPT_MIN, ADAPT_TOLS = 64, 4, (0.002, 0.005)


def adaptive_lines(torch, abi, ctx, name, seed):
    """The adaptive render of the zero camera at a cap of 64 samples beside
    the fixed 64-sample render: one line per tolerance."""
    cam = ctx.camera(samples=ADAPT_CAP)
    fixed = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    cnt = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
    fixed_ms = [timed(torch, lambda: ctx.render_camera_async(cam, 0, H, rgba=fixed), RAD_WARMUP, RAD_LAUNCHES)
                for _ in range(3)]
    # what the launches alone cost: an infinite tolerance stops every pixel at min_samples, so passes 1.. are
    # empty, beside the fixed render at min_samples (one trace launch per chunk, the same rays)
    stop = ctx.adaptive(math.inf, ADAPT_MIN)
    empty_ms = timed(torch, lambda: ctx.render_camera_adaptive_async(cam, stop, 0, H, rgba=rgba, samples=cnt),
                     RAD_WARMUP, RAD_LAUNCHES)
    low = ctx.camera(samples=ADAPT_MIN)
    low_ms = timed(torch, lambda: ctx.render_camera_async(low, 0, H, rgba=rgba), RAD_WARMUP, RAD_LAUNCHES)
    lines = []
    for tol in ADAPT_TOLS:
        ad = ctx.adaptive(tol, ADAPT_MIN)
        ms = [timed(torch, lambda: ctx.render_camera_adaptive_async(cam, ad, 0, H, rgba=rgba, samples=cnt), RAD_WARMUP,
                    RAD_LAUNCHES) for _ in range(3)]
        torch.cuda.synchronize()
        chunks, passes = ctx.render_camera_adaptive_plan(cam, ad)
        v, k = torch.unique(cnt, return_counts=True)
        hist = {int(a): int(b) for a, b in zip(v.tolist(), k.tolist())}
        mean_spp = float(cnt.sum(dtype=torch.int64).item()) / (W * H)
        diff = int((rgba.to(torch.int16) - fixed.to(torch.int16)).abs().max().item())
        am, fm = min(ms), min(fixed_ms)
        lines.append({"metric": "adaptive_rate", "config": name, "mode": "adaptive", "width": W, "height": H,
                      "cap": ADAPT_CAP, "min_samples": ADAPT_MIN, "tolerance": tol,
                      "depth": int(ctx.packed.scene.depth), "objects": int(ctx.packed.scene.num_objects),
                      "bvh": bool(ctx.scene_info() & abi.RT_INFO_BVH),
                      "adaptive_ms": [round(x, 4) for x in ms], "fixed_ms": [round(x, 4) for x in fixed_ms],
                      "fixed_chunks": ctx.render_camera_chunks(cam), "passes": passes, "chunks": chunks,
                      "trace_launches": passes * chunks, "mean_samples": round(mean_spp, 4), "histogram": hist,
                      "time_ratio": round(am / fm, 4), "ray_ratio": round(mean_spp / ADAPT_CAP, 4),
                      "ssim_vs_fixed": ctx.ssim(rgba, fixed), "max_byte_diff": diff,
                      "empty_passes_ms": round(empty_ms, 4), "fixed_min_samples_ms": round(low_ms, 4),
                      "fixed_min_samples_chunks": ctx.render_camera_chunks(low),
                      "launches": RAD_LAUNCHES, "warmup": RAD_WARMUP, "runs": 3, "seed": seed})
    return lines


AOV_SAMPLES, AOV_REPEATS = (4, 64), 5


def repeats(torch, launch, warmup, n):
    """Device-event time of each of n launches after `warmup` warm-ups."""
    for _ in range(warmup):
        launch()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def aov_lines(torch, abi, ctx, name, seed):
    """rt_render_camera_aov_async (all five buffers) of the zero camera at 4
    and 64 samples beside the materialised route it replaces: the camera's
    rays written out, the closest-hit query, the buffers reduced in torch in
    sample order. Median of 5 timed repeats each after one warm-up; the margin
    of the comparison is the spread of the route's own repeats."""
    dev = "cuda:0"
    mats = torch.tensor([list(ctx.packed.scene.materials[i].color[:]) for i in range(int(ctx.packed.scene.num_materials))],
                        dtype=torch.float64, device=dev).reshape(-1, 3)
    lines = []
    for S in AOV_SAMPLES:
        cam = ctx.camera(samples=S)
        n = W * H * S
        bufs = {"depth": torch.empty((H, W), dtype=torch.float64, device=dev),
                "normal": torch.empty((H, W, 3), dtype=torch.float64, device=dev),
                "albedo": torch.empty((H, W, 3), dtype=torch.float64, device=dev),
                "coverage": torch.empty((H, W), dtype=torch.float64, device=dev),
                "ids": torch.empty((H, W, 4), dtype=torch.int32, device=dev)}
        fused = repeats(torch, lambda: ctx.render_camera_aov_async(cam, 0, H, **bufs), 1, AOV_REPEATS)
        rays = torch.empty(n * abi.RAY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        hits = torch.empty(n * abi.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        res = {}

        def route():
            ctx.camera_rays_ex_async(cam, 0, H, rays)
            ctx.query_closest_async(rays, hits)
            f = hits.view(torch.float64).view(H * W, S, 12)
            i = hits.view(torch.int32).view(H * W, S, 24)
            zt = torch.zeros(H * W, dtype=torch.float64, device=dev)
            N = torch.zeros((H * W, 3), dtype=torch.float64, device=dev)
            A = torch.zeros((H * W, 3), dtype=torch.float64, device=dev)
            h = torch.zeros(H * W, dtype=torch.int32, device=dev)
            for s in range(S):
                hit = i[:, s, 20] >= 0
                nw = f[:, s, 7:10]
                ln = torch.sqrt((nw[:, 0] * nw[:, 0] + nw[:, 1] * nw[:, 1]) + nw[:, 2] * nw[:, 2])
                m = hit.unsqueeze(1)
                zt = zt + torch.where(hit, f[:, s, 0], 0.0)
                N = N + torch.where(m, nw / ln.unsqueeze(1), 0.0)
                A = A + torch.where(m, mats[i[:, s, 23].clamp(min=0).long()], 0.0)
                h = h + hit.to(torch.int32)
            inv = 1.0 / S
            hd = h.to(torch.float64)
            res["coverage"] = hd * inv
            res["normal"] = N * inv
            res["albedo"] = A * inv
            res["depth"] = torch.where(h > 0, zt / hd, math.inf)
            res["ids"] = i[:, 0, 20:24].clone()

        route_ms = repeats(torch, route, 1, AOV_REPEATS)
        closures = bool((hits.view(torch.int32).view(-1, 24)[:, 23] < 0).any().item())
        same = {k: bool(torch.equal(res[k].reshape(bufs[k].shape), bufs[k])) for k in bufs}
        hit_frac = float(bufs["coverage"].mean().item())
        del rays, hits, res
        fm, rm = float(np.median(fused)), float(np.median(route_ms))
        spread = max(route_ms) - min(route_ms)
        lines.append({"metric": "aov_rate", "config": name, "mode": "aov", "width": W, "height": H, "samples": S,
                      "objects": int(ctx.packed.scene.num_objects), "bvh": bool(ctx.scene_info() & abi.RT_INFO_BVH),
                      "fused_ms": [round(v, 4) for v in fused], "route_ms": [round(v, 4) for v in route_ms],
                      "fused_median_ms": round(fm, 4), "route_median_ms": round(rm, 4),
                      "route_spread_ms": round(spread, 4), "fused_over_route": round(fm / rm, 4),
                      "fused_wins_beyond_spread": bool(fm < rm - spread),
                      "value": round(n / fm / 1e3, 2), "unit": "Mrays/s", "mean_coverage": round(hit_frac, 4),
                      "route_equals_fused": same, "closure_samples": closures,
                      "route_bytes_per_ray": abi.RAY_DTYPE.itemsize * 2 + abi.HIT_DTYPE.itemsize * 2,
                      "repeats": AOV_REPEATS, "warmup": 1, "seed": seed})
    return lines


DN_SIZES = ((1920, 1080), (3840, 2160))
DN_HBM_BYTES_PER_S, DN_FP64_FLOPS = 8.0e12, 78.6e12  # the spec peaks DESIGN.md's roofline uses
DN_BYTES_PER_PIXEL, DN_FLOP_PER_PIXEL = 104, 1100
DN_CANDIDATES = ((0.6, 0.5, 1.0, 0.25), (0.3, 0.5, 1.0, 0.25), (1.2, 0.5, 1.0, 0.25), (0.0, 0.5, 1.0, 0.25),
                 (0.6, 0.25, 0.5, 0.1), (0.6, 1.0, 2.0, 0.5), (0.6, 0.0, 0.0, 0.0))


def denoise_lines(torch, abi, ctx, name, seed, default_sigmas):
    """rt_denoise_atrous_async, K = 5, all terms on, on a 4-sample thin-lens
    frame of the scene with its feature buffers, at 1080p and 4K: ms per
    iteration (median of 5 repeats of the 5-iteration call) beside the memory
    and FP64 floors; at 1080p also the mean squared error of the raw and of
    the denoised mean against a 256-sample mean, for each candidate sigma set."""
    dev = "cuda:0"
    lines = []
    for (w, h) in DN_SIZES:
        kw = dict(model="thinlens", size=(w, h), aperture=0.2, focus=4.5)
        cam = ctx.camera(samples=4, **kw)
        mean = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
        ctx.render_camera_async(cam, 0, h, mean=mean)
        g = {"normal": torch.empty((h, w, 3), dtype=torch.float64, device=dev),
             "depth": torch.empty((h, w), dtype=torch.float64, device=dev),
             "albedo": torch.empty((h, w, 3), dtype=torch.float64, device=dev)}
        ctx.render_camera_aov_async(cam, 0, h, **g)
        out, tmp = torch.empty_like(mean), torch.empty_like(mean)
        dn = ctx.denoise_params(5, *default_sigmas)
        ms = repeats(torch, lambda: ctx.denoise_async(dn, mean, out, tmp, **g), 1, AOV_REPEATS)
        one = []
        for i in range(5):  # the first i + 1 iterations (a later iteration cannot be launched alone)
            dk = ctx.denoise_params(i + 1, *default_sigmas)
            one.append(round(float(np.median(repeats(torch, lambda: ctx.denoise_async(dk, mean, out, tmp, **g), 1, 3))), 4))
        px = w * h
        line = {"metric": "denoise_rate", "config": name, "mode": "denoise", "width": w, "height": h, "iterations": 5,
                "sigmas": list(default_sigmas), "variant": "LDS tile with halo for steps 1 and 2, global loads beyond; thread per pixel",
                "ms": [round(v, 4) for v in ms], "ms_per_iteration": round(float(np.median(ms)) / 5, 4),
                "first_k_iterations_ms": one,
                "floor_memory_ms": round(px * DN_BYTES_PER_PIXEL / DN_HBM_BYTES_PER_S * 1e3, 4),
                "floor_fp64_ms": round(px * DN_FLOP_PER_PIXEL / DN_FP64_FLOPS * 1e3, 4),
                "repeats": AOV_REPEATS, "warmup": 1, "seed": seed}
        if (w, h) == DN_SIZES[0]:
            ref = torch.empty_like(mean)
            ctx.render_camera_async(ctx.camera(samples=256, **kw), 0, h, mean=ref)
            torch.cuda.synchronize()
            line["mse_raw_vs_256"] = float(((mean - ref) ** 2).mean().item())
            q = []
            for sg in DN_CANDIDATES:
                ctx.denoise_async(ctx.denoise_params(5, *sg), mean, out, tmp, **g)
                torch.cuda.synchronize()
                q.append({"sigmas": list(sg), "mse_vs_256": float(((out - ref) ** 2).mean().item())})
            line["quality"] = q
            del ref
        lines.append(line)
        del mean, out, tmp, g
    return lines


VAR_SIGMAS = (1.0, 2.0, 4.0, 8.0)
VAR_COLOR = 8.0  # render.DENOISE_VAR_COLOR, set by main()
DN_VAR_BYTES_PER_PIXEL, DN_VAR_FLOP_PER_PIXEL = DN_BYTES_PER_PIXEL + 16, 1200  # S_i read and S_(i+1) written; 4 ops a tap


def variance_lines(torch, abi, ctx, name, seed, defaults):
    """The cost of the variance outputs, the time of the variance-guided
    filter beside the plain one, and both filters' error against a 256-sample
    mean (module docstring, "Variance mode")."""
    dev = "cuda:0"
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    r4 = lambda v: [round(x, 4) for x in v]  # noqa: E731
    base = {"config": name, "mode": "variance", "repeats": AOV_REPEATS, "warmup": 1, "seed": seed}
    lines = []
    # 1. the renders with and without d_var (both through the new entry points: d_var NULL is the old call)
    lib = ctx.lib
    mean = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
    var = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
    cnt = torch.empty((H, W), dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    stream = lambda: vp(torch.cuda.current_stream(0).cuda_stream)  # noqa: E731
    for S in AOV_SAMPLES:
        cam = ctx.camera(samples=S)

        def fixed(v):
            rc = lib.rt_render_camera_var_async(ctx.handle, ctypes.byref(cam), 0, H, None, vp(mean.data_ptr()), v, stream())
            assert rc == 0, lib.rt_last_error()

        without = repeats(torch, lambda: fixed(None), 1, AOV_REPEATS)
        with_ = repeats(torch, lambda: fixed(vp(var.data_ptr())), 1, AOV_REPEATS)
        lines.append(dict(base, metric="variance_cost", call="rt_render_camera_var_async", width=W, height=H, samples=S,
                          without_var_ms=r4(without), with_var_ms=r4(with_), without_median_ms=med(without),
                          with_median_ms=med(with_), with_over_without=round(med(with_) / med(without), 4),
                          without_spread_ms=round(max(without) - min(without), 4)))
    cam = ctx.camera(samples=64)
    ad = ctx.adaptive(0.005, 4)

    def adaptive(v):
        rc = lib.rt_render_camera_adaptive_var_async(ctx.handle, ctypes.byref(cam), ctypes.byref(ad), 0, H, None,
                                                     vp(mean.data_ptr()), vp(cnt.data_ptr()), v, stream())
        assert rc == 0, lib.rt_last_error()

    without = repeats(torch, lambda: adaptive(None), 1, AOV_REPEATS)
    with_ = repeats(torch, lambda: adaptive(vp(var.data_ptr())), 1, AOV_REPEATS)
    lines.append(dict(base, metric="variance_cost", call="rt_render_camera_adaptive_var_async", width=W, height=H,
                      samples=64, min_samples=4, tolerance=0.005, mean_samples=round(float(cnt.double().mean().item()), 3),
                      without_var_ms=r4(without), with_var_ms=r4(with_), without_median_ms=med(without),
                      with_median_ms=med(with_), with_over_without=round(med(with_) / med(without), 4),
                      without_spread_ms=round(max(without) - min(without), 4)))
    del mean, var, cnt
    # 2. the filters' time, 3. their error
    for (w, h) in DN_SIZES:
        kw = dict(model="thinlens", size=(w, h), aperture=0.2, focus=4.5)
        cam = ctx.camera(samples=4, **kw)
        mean = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
        var = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
        ctx.render_camera_async(cam, 0, h, mean=mean, var=var)
        g = {"normal": torch.empty((h, w, 3), dtype=torch.float64, device=dev),
             "depth": torch.empty((h, w), dtype=torch.float64, device=dev),
             "albedo": torch.empty((h, w, 3), dtype=torch.float64, device=dev)}
        ctx.render_camera_aov_async(cam, 0, h, **g)
        out, tmp = torch.empty_like(mean), torch.empty_like(mean)
        vo = torch.empty((h, w), dtype=torch.float64, device=dev)
        vt = torch.empty_like(vo)
        vkw = dict(var=var, var_out=vo, var_tmp=vt)
        guides = tuple(defaults[1:])
        vsig = (VAR_COLOR,) + guides
        plain = repeats(torch, lambda: ctx.denoise_async(ctx.denoise_params(5, *defaults), mean, out, tmp, **g), 1, AOV_REPEATS)
        guided = repeats(torch, lambda: ctx.denoise_async(ctx.denoise_params(5, *vsig), mean, out, tmp, **g, **vkw), 1,
                         AOV_REPEATS)
        firstk = {"plain": [], "variance": []}
        for i in range(5):  # the first i + 1 iterations (a later iteration cannot be launched alone)
            dk, dv = ctx.denoise_params(i + 1, *defaults), ctx.denoise_params(i + 1, *vsig)
            firstk["plain"].append(med(repeats(torch, lambda: ctx.denoise_async(dk, mean, out, tmp, **g), 1, 3)))
            firstk["variance"].append(med(repeats(torch, lambda: ctx.denoise_async(dv, mean, out, tmp, **g, **vkw), 1, 3)))
        px = w * h
        line = dict(base, metric="denoise_var_rate", width=w, height=h, iterations=5, plain_sigmas=list(defaults),
                    variance_sigmas=list(vsig), plain_ms=r4(plain), variance_ms=r4(guided), plain_call_ms=med(plain),
                    variance_call_ms=med(guided), plain_ms_per_iteration=round(med(plain) / 5, 4),
                    variance_ms_per_iteration=round(med(guided) / 5, 4),
                    variance_over_plain=round(med(guided) / med(plain), 4), first_k_iterations_ms=firstk,
                    plain_floor_memory_ms=round(px * DN_BYTES_PER_PIXEL / DN_HBM_BYTES_PER_S * 1e3, 4),
                    plain_floor_fp64_ms=round(px * DN_FLOP_PER_PIXEL / DN_FP64_FLOPS * 1e3, 4),
                    variance_floor_memory_ms=round(px * DN_VAR_BYTES_PER_PIXEL / DN_HBM_BYTES_PER_S * 1e3, 4),
                    variance_floor_fp64_ms=round(px * DN_VAR_FLOP_PER_PIXEL / DN_FP64_FLOPS * 1e3, 4))
        if (w, h) == DN_SIZES[0]:
            ref = torch.empty_like(mean)
            ctx.render_camera_async(ctx.camera(samples=256, **kw), 0, h, mean=ref)
            torch.cuda.synchronize()
            mse = lambda t: float(((t - ref) ** 2).mean().item())  # noqa: E731

            def run(sig, m, v=None):
                kv = dict(var=v, var_out=vo, var_tmp=vt) if v is not None else {}
                gg = {k: t for k, t, sg in (("normal", g["normal"], sig[1]), ("depth", g["depth"], sig[2]),
                                            ("albedo", g["albedo"], sig[3])) if sg > 0.0}
                ctx.denoise_async(ctx.denoise_params(5, *sig), m, out, tmp, **gg, **kv)
                torch.cuda.synchronize()
                return mse(out)

            q = [{"filter": "raw", "mse_vs_256": mse(mean)},
                 {"filter": "plain", "sigmas": list(defaults), "mse_vs_256": run(defaults, mean)},
                 {"filter": "plain", "sigmas": [defaults[0], 0.0, 0.0, 0.0],
                  "mse_vs_256": run((defaults[0], 0.0, 0.0, 0.0), mean)}]
            for sc in VAR_SIGMAS:
                for gs in (guides, (0.0, 0.0, 0.0)):
                    q.append({"filter": "variance", "sigmas": [sc] + list(gs), "mse_vs_256": run((sc,) + gs, mean, var)})
            line["quality"] = q
            line["mean_variance"] = float(var.sum(dim=2).mean().item())
            # one adaptive frame filtered with its own variance
            acam = ctx.camera(samples=64, **kw)
            amean, avar = torch.empty_like(mean), torch.empty_like(var)
            acnt = torch.empty((h, w), dtype=torch.int32, device=dev)
            ctx.render_camera_adaptive_async(acam, ctx.adaptive(0.005, 4), 0, h, mean=amean, samples=acnt, var=avar)
            torch.cuda.synchronize()
            qa = [{"filter": "raw", "mse_vs_256": mse(amean)},
                  {"filter": "plain", "sigmas": list(defaults), "mse_vs_256": run(defaults, amean)},
                  {"filter": "plain", "sigmas": [defaults[0], 0.0, 0.0, 0.0],
                   "mse_vs_256": run((defaults[0], 0.0, 0.0, 0.0), amean)}]
            for sc in VAR_SIGMAS:
                for gs in (guides, (0.0, 0.0, 0.0)):
                    qa.append({"filter": "variance", "sigmas": [sc] + list(gs),
                               "mse_vs_256": run((sc,) + gs, amean, avar)})
            line["adaptive"] = {"tolerance": 0.005, "min_samples": 4, "cap": 64,
                                "mean_samples": round(float(acnt.double().mean().item()), 3), "quality": qa}
            del ref, amean, avar, acnt
        lines.append(line)
        del mean, var, out, tmp, vo, vt, g
    return lines


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
        del hits, occ
        if "radiance" in modes:
            lines.append(radiance_line(torch, abi, ctx, name, args.seed))
            print(json.dumps(lines[-1]), flush=True)
        if "camera" in modes:
            lines.append(camera_line(torch, abi, ctx, name, args.seed))
            print(json.dumps(lines[-1]), flush=True)
        if "adaptive" in modes:
            for ln in adaptive_lines(torch, abi, ctx, name, args.seed):
                lines.append(ln)
                print(json.dumps(ln), flush=True)
        if "aov" in modes:
            for ln in aov_lines(torch, abi, ctx, name, args.seed):
                lines.append(ln)
                print(json.dumps(ln), flush=True)
        if "denoise" in modes:
            d = pkg.render.DENOISE_DEFAULTS
            for ln in denoise_lines(torch, abi, ctx, name, args.seed, (d["color"], d["normal"], d["depth"], d["albedo"])):
                lines.append(ln)
                print(json.dumps(ln), flush=True)
        if "variance" in modes:
            d = pkg.render.DENOISE_DEFAULTS
            global VAR_COLOR
            VAR_COLOR = pkg.render.DENOISE_VAR_COLOR
            for ln in variance_lines(torch, abi, ctx, name, args.seed, (d["color"], d["normal"], d["depth"], d["albedo"])):
                lines.append(ln)
                print(json.dumps(ln), flush=True)
    ctx.close()
    if args.out is None and "variance" in args.modes.split(","):
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "variance",
                                "variance_rate.jsonl")
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        lines = [ln for ln in lines if ln["mode"] == "variance"]
    if args.out is None and ("aov" in args.modes.split(",") or "denoise" in args.modes.split(",")):
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "aov",
                                "aov_rate.jsonl")
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        lines = [ln for ln in lines if ln["mode"] in ("aov", "denoise")]
    if args.out is None and "adaptive" in args.modes.split(","):
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "adaptive",
                                "adaptive_rate.jsonl")
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        lines = [ln for ln in lines if ln["mode"] == "adaptive"]
    if args.out is None and "camera" in args.modes.split(","):
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "camera",
                                "camera_rate.jsonl")
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        lines = [ln for ln in lines if ln["mode"] == "camera"]
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
