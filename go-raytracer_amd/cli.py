"""Render GML programs through the HIP path and write the images.

The reference's `render` builtin calls EvalState.Render, which renders and
writes a PNG named by the program (raytracer.go:700-708, cmd/gml/main.go:
383-390). Here each render call of the program is converted and rendered on
the device as it happens (the hook runs mid-program, so later frames see the
state as it was then), then written by imageio.

usage: python -m go_raytracer_amd.cli [--out-dir DIR] [--device N] [--stats] [camera flags] file.gml ...

Camera flags (--samples N, --camera pinhole|ortho|equirect|thinlens, --eye,
--look-at, --up, --fov, --extent, --aperture, --focus, --size WxH) route each
`render` of the program through a camera render (RenderContext.render_camera)
instead; without any of them the render path is the one above.
--adaptive TOL makes that camera render adaptive (RenderContext.
render_camera_adaptive): --samples is then the cap, --min-samples N the first
pass, and --samples-map FILE receives the per-pixel sample counts as grey
levels, count * 255 // cap.
(from the repo root the package directory is go-raytracer_amd/; see
__graft_entry__.load_package)
"""
import argparse
import json
import os
import sys


def camera_from_args(a):
    """The abi.rt_camera the camera flags of `a` describe, or None when none was given."""
    given = {k: getattr(a, k) for k in ("samples", "camera", "eye", "look_at", "up", "fov", "extent", "aperture",
                                        "focus", "size") if getattr(a, k, None) is not None}
    if not given:
        return None
    from .render import RenderContext
    kw = {k: given[k] for k in ("samples", "eye", "look_at", "up", "fov", "extent", "aperture", "focus") if k in given}
    if "size" in given:
        w, _, h = given["size"].lower().partition("x")
        kw["size"] = (int(w), int(h))
    return RenderContext.camera(model=given.get("camera", "pinhole"), **kw)


def adaptive_from_args(a):
    """The abi.rt_adaptive of --adaptive / --min-samples, or None without --adaptive."""
    if getattr(a, "adaptive", None) is None:
        if getattr(a, "min_samples", None) is not None or getattr(a, "samples_map", None) is not None:
            raise SystemExit("--min-samples and --samples-map need --adaptive")
        return None
    from .render import RenderContext
    return RenderContext.adaptive(a.adaptive, a.min_samples or 0)


def samples_image(counts, cap):
    """The sample counts as an opaque grey frame: count * 255 // cap."""
    import numpy as np
    g = (counts.astype(np.int64) * 255 // int(cap)).astype(np.uint8)
    return np.stack([g, g, g], axis=-1)


def render_program(path, out_dir=None, device=0, stats=False, log=sys.stdout, extensions=False, camera=None,
                   adaptive=None, samples_map=None):
    from . import gml, imageio, scene
    from .render import RenderContext
    ctx = RenderContext(device)
    written = []

    def hook(e, args):
        args.state = e.clone()
        packed = scene.convert(args)
        ctx.set_scene(packed)
        ctx.read_stats(reset=True)
        if adaptive is not None:
            cam = RenderContext.camera() if camera is None else camera
            img, counts = ctx.render_camera_adaptive(cam, adaptive, samples=True)
            if samples_map:
                imageio.write_image(samples_map, samples_image(counts, int(cam.samples) or 4))
        else:
            img = ctx.render() if camera is None else ctx.render_camera(camera)
        st = ctx.read_stats(reset=True)  # (camera renders count nothing)
        name = os.path.basename(args.file) if out_dir else args.file
        dst = os.path.join(out_dir, name) if out_dir else name
        imageio.write_image(dst, img)
        written.append(dst)
        if stats:
            d = st.as_dict()
            d.update(file=dst, kernel_ms=round(st.kernel_ms, 3), width=img.shape[1], height=img.shape[0])
            print(json.dumps(d), file=log)

    try:
        st = gml.EvalState(render=hook, extensions=extensions)
        st.parse_and_eval_file(path)
    finally:
        ctx.close()
    return written


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("files", nargs="+")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--extensions", action="store_true",
                    help="enable cone, light, spotlight, real, asin, acos, intersect (ICFP operators the reference lacks)")
    ap.add_argument("--samples", type=int, default=None, help="samples per pixel (1..1024) of a camera render")
    ap.add_argument("--camera", choices=["pinhole", "ortho", "equirect", "thinlens"], default=None)
    for flag in ("--eye", "--look-at", "--up"):
        ap.add_argument(flag, type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--fov", type=float, default=None, help="degrees (pinhole, thinlens)")
    ap.add_argument("--extent", type=float, default=None, help="ortho: world width of the view")
    ap.add_argument("--aperture", type=float, default=None, help="thinlens: lens diameter")
    ap.add_argument("--focus", type=float, default=None, help="thinlens: focal-plane distance")
    ap.add_argument("--size", default=None, metavar="WxH", help="frame size of a camera render")
    ap.add_argument("--adaptive", type=float, default=None, metavar="TOL",
                    help="adaptive camera render: stop a pixel at this standard error; --samples is the cap")
    ap.add_argument("--min-samples", type=int, default=None, metavar="N", help="samples of the first adaptive pass")
    ap.add_argument("--samples-map", default=None, metavar="FILE", help="write the per-pixel sample counts as grey levels")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    cam = camera_from_args(a)
    ad = adaptive_from_args(a)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
    for f in a.files:
        for w in render_program(f, a.out_dir, a.device, a.stats, extensions=a.extensions, camera=cam,
                                adaptive=ad, samples_map=a.samples_map):
            print("wrote", w)
    return 0


if __name__ == "__main__":
    sys.exit(main())
