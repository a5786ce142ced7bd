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
--aov LIST (comma-separated names of depth, normal, albedo, coverage, ids)
also writes the camera's feature buffers (RenderContext.render_camera_aov) as
<image>.<name>.npy, and a PNG view <image>.<name>.png of each but ids.
--denoise filters the camera render's float64 mean with the guided a-trous
filter (RenderContext.denoise; guides: normal, depth, albedo) and writes
<image stem>.denoised<ext>; --denoise-iterations K and --denoise-sigmas C,N,Z,A
(colour, normal, depth, albedo; 0 turns a term off) replace the defaults.
--denoise-variance (with --denoise) renders the per-pixel variance of the mean
too and runs the variance-guided filter: C is then in standard deviations
(default render.DENOISE_VAR_COLOR). --variance-map FILE writes that variance
as an .npy of float64 [H, W, 3].
Either flag alone selects the camera render of the scene's own camera.
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


def aov_from_args(a):
    """The feature-buffer names of --aov as a tuple, or None without the flag."""
    if getattr(a, "aov", None) is None:
        return None
    from . import abi
    names = tuple(n.strip() for n in a.aov.split(",") if n.strip())
    bad = [n for n in names if n not in abi.AOV_NAMES]
    if bad or not names:
        raise SystemExit("--aov takes a comma-separated list of: %s" % ", ".join(abi.AOV_NAMES))
    return names


def denoise_from_args(a):
    """The abi.rt_denoise of --denoise / --denoise-iterations / --denoise-sigmas, or None without --denoise.
    With --denoise-variance the default colour sigma is render.DENOISE_VAR_COLOR standard deviations."""
    if not getattr(a, "denoise", False):
        if getattr(a, "denoise_iterations", None) is not None or getattr(a, "denoise_sigmas", None) is not None:
            raise SystemExit("--denoise-iterations and --denoise-sigmas need --denoise")
        if getattr(a, "denoise_variance", False):
            raise SystemExit("--denoise-variance needs --denoise")
        return None
    from .render import DENOISE_DEFAULTS, DENOISE_VAR_COLOR, RenderContext
    d = DENOISE_DEFAULTS
    sig = [DENOISE_VAR_COLOR if getattr(a, "denoise_variance", False) else d["color"], d["normal"], d["depth"],
           d["albedo"]]
    if a.denoise_sigmas is not None:
        try:
            sig = [float(v) for v in a.denoise_sigmas.split(",")]
        except ValueError:
            sig = []
        if len(sig) != 4:
            raise SystemExit("--denoise-sigmas takes four numbers: C,N,Z,A")
    return RenderContext.denoise_params(a.denoise_iterations or 0, *sig)


def aov_view(name, buf):
    """An opaque 8-bit view [rows, W, 3] of the feature buffer `name`: depth
    near white to far black over the finite range (background black), normal
    as (n + 1) / 2, albedo and coverage clipped to [0, 1]."""
    import numpy as np
    if name == "depth":
        fin = np.isfinite(buf)
        g = np.zeros(buf.shape)
        if fin.any():
            lo, hi = buf[fin].min(), buf[fin].max()
            g[fin] = 1.0 - (buf[fin] - lo) / (hi - lo) * 0.9 if hi > lo else 1.0
        v = np.stack([g, g, g], axis=-1)
    elif name == "normal":
        v = (np.nan_to_num(buf) + 1.0) / 2.0
    elif name == "albedo":
        v = np.nan_to_num(buf)
    elif name == "coverage":
        v = np.stack([buf, buf, buf], axis=-1)
    else:
        raise ValueError("no view of feature buffer %r" % name)
    return (np.clip(v, 0.0, 1.0) * 255.0).astype(np.uint8)


def render_program(path, out_dir=None, device=0, stats=False, log=sys.stdout, extensions=False, camera=None,
                   adaptive=None, samples_map=None, aov=None, denoise=None, denoise_variance=False, variance_map=None):
    from . import gml, imageio, scene
    from .render import RenderContext
    ctx = RenderContext(device)
    written = []

    def hook(e, args):
        args.state = e.clone()
        packed = scene.convert(args)
        ctx.set_scene(packed)
        ctx.read_stats(reset=True)
        cam = camera
        want_var = bool(denoise_variance or variance_map)
        if cam is None and (adaptive is not None or aov or denoise is not None or want_var):
            cam = RenderContext.camera()
        mean = None  # the float64 mean: wanted by --denoise only
        var = None   # the variance of that mean: wanted by --denoise-variance and --variance-map
        if adaptive is not None:
            got = ctx.render_camera_adaptive(cam, adaptive, mean=denoise is not None, samples=True, var=want_var)
            img, counts = got[0], got[-2 if want_var else -1]
            if denoise is not None:
                mean = got[1]
            if want_var:
                var = got[-1]
            if samples_map:
                imageio.write_image(samples_map, samples_image(counts, int(cam.samples) or 4))
        elif want_var:
            got = ctx.render_camera(cam, mean=denoise is not None, var=True)
            img, var = got[0], got[-1]
            if denoise is not None:
                mean = got[1]
        elif cam is not None and denoise is not None:
            img, mean = ctx.render_camera(cam, mean=True)
        else:
            img = ctx.render() if cam is None else ctx.render_camera(cam)
        st = ctx.read_stats(reset=True)  # (camera renders count nothing)
        name = os.path.basename(args.file) if out_dir else args.file
        dst = os.path.join(out_dir, name) if out_dir else name
        imageio.write_image(dst, img)
        written.append(dst)
        if variance_map:
            import numpy as np
            with open(variance_map, "wb") as f:  # (the name as given: numpy.save would append .npy to a path)
                np.save(f, var)
            written.append(variance_map)
        if aov or denoise is not None:
            import numpy as np
            need = set(aov or ())
            if denoise is not None:
                need |= {n for n, sg in (("normal", denoise.sigma_normal), ("depth", denoise.sigma_depth),
                                         ("albedo", denoise.sigma_albedo)) if 0.0 < sg < float("inf")}
            bufs = ctx.render_camera_aov(cam, which=tuple(need)) if need else {}
            for n in aov or ():
                np.save(dst + "." + n + ".npy", bufs[n])
                written.append(dst + "." + n + ".npy")
                if n != "ids":
                    imageio.write_image(dst + "." + n + ".png", aov_view(n, bufs[n]))
                    written.append(dst + "." + n + ".png")
            if denoise is not None:
                _, dimg = ctx.denoise(mean, bufs.get("normal"), bufs.get("depth"), bufs.get("albedo"), denoise,
                                      rgba=True, var=var if denoise_variance else None)
                stem, ext = os.path.splitext(dst)
                imageio.write_image(stem + ".denoised" + ext, dimg)
                written.append(stem + ".denoised" + ext)
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
    ap.add_argument("--aov", default=None, metavar="LIST",
                    help="write these feature buffers (depth,normal,albedo,coverage,ids) of the camera render")
    ap.add_argument("--denoise", action="store_true", help="also write the camera render's mean through the a-trous filter")
    ap.add_argument("--denoise-iterations", type=int, default=None, metavar="K", help="iterations of the filter (1..8)")
    ap.add_argument("--denoise-sigmas", default=None, metavar="C,N,Z,A",
                    help="sigmas of the colour, normal, depth and albedo terms (0: off)")
    ap.add_argument("--denoise-variance", action="store_true",
                    help="with --denoise: the variance-guided filter; C of --denoise-sigmas is in standard deviations")
    ap.add_argument("--variance-map", default=None, metavar="FILE",
                    help="write the variance of the camera render's mean as an .npy of float64 [H, W, 3]")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    cam = camera_from_args(a)
    ad = adaptive_from_args(a)
    aov = aov_from_args(a)
    dn = denoise_from_args(a)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
    for f in a.files:
        for w in render_program(f, a.out_dir, a.device, a.stats, extensions=a.extensions, camera=cam,
                                adaptive=ad, samples_map=a.samples_map, aov=aov, denoise=dn,
                                denoise_variance=a.denoise_variance, variance_map=a.variance_map):
            print("wrote", w)
    return 0


if __name__ == "__main__":
    sys.exit(main())
