"""Render(): the reference's entry point (raytracer.go:589) over the C ABI.

The only compute path is the HIP library csrc/librtamd.so (gfx950). There is
no CPU fallback: if the library or a HIP device is missing, every call raises.
PyTorch is used only for device memory and streams.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from . import scene as _scene

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "csrc", "librtamd.so")

_lib = None
# sigmas RenderContext.denoise and the CLI use when none are given (README "Denoising")
DENOISE_DEFAULTS = {"color": 0.6, "normal": 0.5, "depth": 1.0, "albedo": 0.25}
# the colour sigma, in standard deviations, of the variance-guided mode (RenderContext.denoise with `var`): the
# best of 1, 2, 4, 8 on the measured frame (BASELINE.md "Measured: variance and the variance-guided filter");
# SVGF's published 4 came second
DENOISE_VAR_COLOR = 8.0


class RenderError(RuntimeError):
    pass


def load_library(path=None):
    """Load librtamd.so and declare the include/rt_abi.h signatures.
    RT_AMD_LIB overrides the in-tree path (A/B builds of the same ABI)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("RT_AMD_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise RenderError("HIP renderer library not built: %s (run __graft_entry__.build())" % path)
    # torch bundles its own libamdhip64 (same soname as /opt/rocm's): load it
    # first so librtamd binds to that one runtime; loading the library first
    # would put two HIP runtimes in the process and the second finds no device.
    import torch  # noqa: F401
    l = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    l.rt_abi_version.argtypes = []
    l.rt_abi_version.restype = i
    l.rt_last_error.argtypes = []
    l.rt_last_error.restype = C.c_char_p
    l.rt_create.argtypes = [i, C.POINTER(vp)]
    l.rt_create.restype = i
    l.rt_destroy.argtypes = [vp]
    l.rt_destroy.restype = None
    l.rt_set_scene.argtypes = [vp, vp]
    l.rt_set_scene.restype = i
    l.rt_render_rows_async.argtypes = [vp, i, i, vp, vp]
    l.rt_render_rows_async.restype = i
    l.rt_render_tile_rows_async.argtypes = [vp, i, i, i, vp, vp]
    l.rt_render_tile_rows_async.restype = i
    l.rt_read_stats.argtypes = [vp, vp, i, vp]
    l.rt_read_stats.restype = i
    l.rt_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]
    l.rt_last_kernel_ms.restype = i
    l.rt_debug_run_surface.argtypes = [vp, i, i, vp, vp, vp, vp, vp]
    l.rt_debug_run_surface.restype = i
    l.rt_ssim_rgba8.argtypes = [vp, vp, vp, i, i, C.POINTER(C.c_double), vp]
    l.rt_ssim_rgba8.restype = i
    l.rt_set_specialize.argtypes = [vp, i]
    l.rt_set_specialize.restype = i
    l.rt_set_accel.argtypes = [vp, i]
    l.rt_set_accel.restype = i
    l.rt_set_schedule.argtypes = [vp, i]
    l.rt_set_schedule.restype = i
    l.rt_scene_info.argtypes = [vp, C.POINTER(i)]
    l.rt_scene_info.restype = i
    l.rt_specialized.argtypes = [vp, C.POINTER(i), C.POINTER(C.c_double)]
    l.rt_specialized.restype = i
    l.rt_spec_precompile.argtypes = [i, C.POINTER(i), i, C.POINTER(C.c_double)]
    l.rt_spec_precompile.restype = i
    l.rt_set_work_sharing.argtypes = [vp, i]
    l.rt_set_work_sharing.restype = i
    l.rt_set_tile_order.argtypes = [vp, i]
    l.rt_set_tile_order.restype = i
    l.rt_set_frames_in_flight.argtypes = [vp, i]
    l.rt_set_frames_in_flight.restype = i
    l.rt_tile_order_info.argtypes = [vp, C.POINTER(i), C.POINTER(C.c_double)]
    l.rt_tile_order_info.restype = i
    l.rt_render.argtypes = [vp, vp, vp]
    l.rt_render.restype = i
    l.rt_render_last_timing.argtypes = [vp]
    l.rt_render_last_timing.restype = i
    l.rt_render_ex.argtypes = [vp, vp, vp, vp]
    l.rt_render_ex.restype = i
    l.rt_debug_assemble.argtypes = [i, i, i, i, vp, vp]
    l.rt_debug_assemble.restype = i
    l.rt_debug_spec_compile.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
    l.rt_debug_spec_compile.restype = i
    l.rt_debug_getenv.argtypes = [C.c_char_p]
    l.rt_debug_getenv.restype = C.c_char_p
    l.rt_query_closest_async.argtypes = [vp, i, vp, vp, vp]
    l.rt_query_closest_async.restype = i
    l.rt_query_occluded_async.argtypes = [vp, i, vp, vp, vp]
    l.rt_query_occluded_async.restype = i
    l.rt_query_radiance_async.argtypes = [vp, i, vp, i, vp, vp]
    l.rt_query_radiance_async.restype = i
    l.rt_query_radiance_lanes.argtypes = [vp, i]
    l.rt_query_radiance_lanes.restype = i
    l.rt_query_camera_rays_async.argtypes = [vp, i, i, vp, vp]
    l.rt_query_camera_rays_async.restype = i
    l.rt_camera_rays_async.argtypes = [vp, vp, i, i, vp, vp]
    l.rt_camera_rays_async.restype = i
    l.rt_render_camera_async.argtypes = [vp, vp, i, i, vp, vp, vp]
    l.rt_render_camera_async.restype = i
    l.rt_render_camera_chunks.argtypes = [vp, vp, i, i]
    l.rt_render_camera_chunks.restype = i
    l.rt_render_camera_adaptive_async.argtypes = [vp, vp, vp, i, i, vp, vp, vp, vp]
    l.rt_render_camera_adaptive_async.restype = i
    l.rt_render_camera_adaptive_plan.argtypes = [vp, vp, vp, i, i, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    l.rt_render_camera_adaptive_plan.restype = i
    l.rt_render_camera_aov_async.argtypes = [vp, vp, i, i, vp, vp]
    l.rt_render_camera_aov_async.restype = i
    l.rt_denoise_atrous_async.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    l.rt_denoise_atrous_async.restype = i
    l.rt_render_camera_var_async.argtypes = [vp, vp, i, i, vp, vp, vp, vp]
    l.rt_render_camera_var_async.restype = i
    l.rt_render_camera_adaptive_var_async.argtypes = [vp, vp, vp, i, i, vp, vp, vp, vp, vp]
    l.rt_render_camera_adaptive_var_async.restype = i
    l.rt_denoise_atrous_var_async.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    l.rt_denoise_atrous_var_async.restype = i
    if l.rt_abi_version() != abi.RT_ABI_VERSION:
        raise RenderError("librtamd ABI version mismatch")
    _lib = l
    return l


def _check(rc, what):
    if rc != abi.RT_OK:
        msg = _lib.rt_last_error() if _lib is not None else b""
        raise RenderError("%s failed (%d): %s" % (what, rc, (msg or b"").decode(errors="replace")))


def _packed(scene_or_args):
    if isinstance(scene_or_args, abi.PackedScene):
        return scene_or_args
    return _scene.convert(scene_or_args)


class RenderContext:
    """One device context: scene resident in HBM, renders rows on a torch stream."""

    def __init__(self, device=None, specialize=False):
        import torch
        if not torch.cuda.is_available():
            raise RenderError("no HIP device visible: the renderer has no CPU path")
        self.torch = torch
        self.lib = load_library()
        self.device = torch.cuda.current_device() if device is None else int(device)
        with torch.cuda.device(self.device):
            h = C.c_void_p()
            _check(self.lib.rt_create(self.device, C.byref(h)), "rt_create")
        self.handle = h
        self.packed = None
        if specialize:
            self.set_specialize(True)

    def close(self):
        if self.handle:
            self.lib.rt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, scene_or_args):
        self.packed = _packed(scene_or_args)
        _check(self.lib.rt_set_scene(self.handle, self.packed.ref()), "rt_set_scene")
        return self.packed

    def set_specialize(self, enable=True):
        """Render with a kernel compiled for the scene's shape (hipRTC, ~1-2 s
        once per scene shape and process; bit-identical output). Raises
        RenderError if hipRTC fails."""
        _check(self.lib.rt_set_specialize(self.handle, int(bool(enable))), "rt_set_specialize")

    def set_accel(self, flags):
        """abi.RT_ACCEL_BVH | abi.RT_ACCEL_CULL (default both). 0 = the
        reference's brute-force search (every ray tests every object in FP64;
        identical pixels and counters). The BVH choice applies at the next
        set_scene; culling applies to specialised kernels."""
        _check(self.lib.rt_set_accel(self.handle, int(flags)), "rt_set_accel")

    def set_schedule(self, mode):
        """abi.RT_SCHED_AUTO (default: pixel quads for depth >= 7),
        RT_SCHED_PIXEL or RT_SCHED_QUADS -- how pixels are dealt to lanes;
        identical pixels and counters. Applies at the next set_scene."""
        _check(self.lib.rt_set_schedule(self.handle, int(mode)), "rt_set_schedule")

    def set_tile_order(self, enable=True):
        """Deal each launch's tiles most expensive first (default on; the
        estimate -- one centre sample per 8x8 tile -- runs at scene setup);
        identical pixels and counters either way. Applies at once."""
        _check(self.lib.rt_set_tile_order(self.handle, int(bool(enable))), "rt_set_tile_order")

    def set_frames_in_flight(self, n):
        """This context is one of n whose launches overlap (frames in flight,
        dist.DistributedRenderer with a list of contexts): the automatic
        schedule may then prefer serial samples at depth >= 7. Identical
        pixels and counters. Applies at once."""
        _check(self.lib.rt_set_frames_in_flight(self.handle, int(n)), "rt_set_frames_in_flight")

    def set_work_sharing(self, enable=True):
        """Work sharing at the tail of a launch (specialised kernel only;
        identical pixels and counters; applies at once). True / 1 the
        workgroup board (RT_SHARE_GROUP), 2 the device-wide one
        (RT_SHARE_DEVICE); the library default is RT_SHARE_AUTO: the device
        board for CSG scenes at depth >= 7 on strong-scaling shares or without
        frames in flight, else off."""
        # True / 1: the workgroup board; 2 (abi.RT_SHARE_DEVICE): device-wide
        mode = int(enable)
        _check(self.lib.rt_set_work_sharing(self.handle, mode), "rt_set_work_sharing")

    def tile_order_info(self):
        """(active, estimate_ms): whether the current scene's launches use a
        tile order, and the estimate's wall time at scene setup."""
        a, ms = C.c_int(), C.c_double()
        _check(self.lib.rt_tile_order_info(self.handle, C.byref(a), C.byref(ms)), "rt_tile_order_info")
        return bool(a.value), ms.value

    def scene_info(self):
        """rt_scene_info flags of the current scene (abi.RT_INFO_*): which
        kernel flavour renders it."""
        f = C.c_int()
        _check(self.lib.rt_scene_info(self.handle, C.byref(f)), "rt_scene_info")
        return f.value

    def specialized(self):
        """(active, compile_ms): whether the current scene runs a specialised
        kernel and what preparing it cost (0 on a cache hit)."""
        a, ms = C.c_int(), C.c_double()
        _check(self.lib.rt_specialized(self.handle, C.byref(a), C.byref(ms)), "rt_specialized")
        return bool(a.value), ms.value

    def render_rows_async(self, y0, y1, out, stream=None):
        """Enqueue rows [y0, y1) into the uint8 CUDA tensor `out` ([y1-y0, W, 4])."""
        torch = self.torch
        W = self.packed.width
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
        assert out.numel() == (y1 - y0) * W * 4, "output tensor shape does not match rows"
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        _check(self.lib.rt_render_rows_async(self.handle, int(y0), int(y1), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(s.cuda_stream)), "rt_render_rows_async")

    def render_tile_rows_async(self, trow0, stride, ntrows, out, stream=None):
        """Enqueue `ntrows` interleaved 8-row tile rows (image tile rows trow0 + j*stride)
        into the uint8 CUDA tensor `out` ([ntrows*8, W, 4])."""
        torch = self.torch
        W = self.packed.width
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
        assert out.numel() == ntrows * 8 * W * 4, "output tensor shape does not match tile rows"
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        _check(self.lib.rt_render_tile_rows_async(self.handle, int(trow0), int(stride), int(ntrows),
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)),
               "rt_render_tile_rows_async")

    def read_stats(self, reset=True, stream=None):
        s = self.torch.cuda.current_stream(self.device) if stream is None else stream
        st = abi.rt_stats()
        _check(self.lib.rt_read_stats(self.handle, C.c_void_p(s.cuda_stream), int(reset), C.byref(st)),
               "rt_read_stats")
        return st

    def last_kernel_ms(self):
        ms = C.c_double()
        _check(self.lib.rt_last_kernel_ms(self.handle, C.byref(ms)), "rt_last_kernel_ms")
        return ms.value

    def debug_run_surface(self, program, face, u, v):
        """Diagnostic: run one surface program on the device for arrays of inputs."""
        face = np.ascontiguousarray(face, dtype=np.int64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        v = np.ascontiguousarray(v, dtype=np.float64)
        n = len(face)
        out = np.zeros((n, 10), dtype=np.float64)
        err = np.zeros(n, dtype=np.int32)
        _check(self.lib.rt_debug_run_surface(self.handle, int(program), n, face.ctypes.data, u.ctypes.data,
                                             v.ctypes.data, out.ctypes.data, err.ctypes.data), "rt_debug_run_surface")
        return out, err

    def ssim(self, a, b):
        """prim.SSIM (internal/prim/ssim.go:27-182) of two RGBA8 frames on the
        device. a, b: uint8 [H, W, 4] (or [H, W, 3]) torch tensors or numpy
        arrays; host arrays are uploaded."""
        torch = self.torch
        dev = "cuda:%d" % self.device

        def prep(x):
            t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=np.uint8, copy=True))
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] not in (3, 4):
                raise ValueError("ssim: expected uint8 [H, W, 3|4] images")
            t = t.to(dev)
            if t.shape[2] == 3:
                t = torch.cat([t, torch.full_like(t[..., :1], 255)], dim=2)
            return t.contiguous()

        ta, tb = prep(a), prep(b)
        if ta.shape != tb.shape:
            raise ValueError("images are not the same size")  # ssim.go:29-31
        out = C.c_double()
        stream = torch.cuda.current_stream(self.device)
        _check(self.lib.rt_ssim_rgba8(self.handle, C.c_void_p(ta.data_ptr()), C.c_void_p(tb.data_ptr()),
                                      int(ta.shape[1]), int(ta.shape[0]), C.byref(out),
                                      C.c_void_p(stream.cuda_stream)), "rt_ssim_rgba8")
        return out.value

    def render(self, y0=0, y1=None):
        """Synchronous render of rows [y0, y1) -> numpy uint8 [rows, W, 4]."""
        torch = self.torch
        if y1 is None:
            y1 = self.packed.height
        out = torch.empty((y1 - y0, self.packed.width, 4), dtype=torch.uint8, device="cuda:%d" % self.device)
        self.render_rows_async(y0, y1, out)
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy()

    # ---- batched ray queries (include/rt_abi.h rt_query_*_async) ----
    def _query_args(self, rays, out, out_bytes, what):
        torch = self.torch
        for t, name in ((rays, "rays"), (out, "output")):
            assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous(), \
                "%s: %s must be a contiguous uint8 CUDA tensor" % (what, name)
            assert t.device.index == self.device, "%s: %s is on another device" % (what, name)
        rec = abi.RAY_DTYPE.itemsize
        assert rays.numel() % rec == 0, "%s: rays must hold whole %d-byte records" % (what, rec)
        n = rays.numel() // rec
        assert out.numel() == n * out_bytes, "%s: output tensor size does not match %d rays" % (what, n)
        return n

    def query_closest_async(self, rays, hits, stream=None):
        """Enqueue closest-hit queries: `rays` a uint8 CUDA tensor of n * 64
        bytes (abi.RAY_DTYPE records), `hits` one of n * 96 bytes
        (abi.HIT_DTYPE), against the current scene, ordered on `stream`."""
        n = self._query_args(rays, hits, abi.HIT_DTYPE.itemsize, "query_closest_async")
        s = self.torch.cuda.current_stream(self.device) if stream is None else stream
        _check(self.lib.rt_query_closest_async(self.handle, n, C.c_void_p(rays.data_ptr()),
                                               C.c_void_p(hits.data_ptr()), C.c_void_p(s.cuda_stream)),
               "rt_query_closest_async")

    def query_occluded_async(self, rays, out, stream=None):
        """Enqueue occlusion queries: out[i] = 1 when ray i meets any object
        other than its `exclude` at T < tmax. `out`: a uint8 CUDA tensor of n bytes."""
        n = self._query_args(rays, out, 1, "query_occluded_async")
        s = self.torch.cuda.current_stream(self.device) if stream is None else stream
        _check(self.lib.rt_query_occluded_async(self.handle, n, C.c_void_p(rays.data_ptr()),
                                                C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)),
               "rt_query_occluded_async")

    def _upload_rays(self, origins, dirs, tmax, exclude):
        o = np.asarray(origins, dtype=np.float64)
        d = np.asarray(dirs, dtype=np.float64)
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError("origins and dirs must both be [n, 3] arrays")
        n = o.shape[0]
        rec = np.zeros(n, dtype=abi.RAY_DTYPE)
        rec["origin"] = o
        rec["dir"] = d
        rec["tmax"] = np.inf if tmax is None else np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,))
        rec["exclude"] = -1 if exclude is None else np.broadcast_to(np.asarray(exclude, dtype=np.int32), (n,))
        dev = "cuda:%d" % self.device
        return n, self.torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)

    def closest_hits(self, origins, dirs, tmax=None, exclude=None):
        """Synchronous closest-hit queries for numpy [n, 3] float64 origins and
        directions (tmax, exclude: None, a scalar or [n]) -> abi.HIT_DTYPE array [n]."""
        torch = self.torch
        n, rays = self._upload_rays(origins, dirs, tmax, exclude)
        hits = torch.empty(n * abi.HIT_DTYPE.itemsize, dtype=torch.uint8, device=rays.device)
        self.query_closest_async(rays, hits)
        torch.cuda.synchronize(self.device)
        return hits.cpu().numpy().view(abi.HIT_DTYPE)

    def occluded(self, origins, dirs, tmax=None, exclude=None):
        """Synchronous occlusion queries (arguments as closest_hits) -> bool array [n]."""
        torch = self.torch
        n, rays = self._upload_rays(origins, dirs, tmax, exclude)
        out = torch.empty(n, dtype=torch.uint8, device=rays.device)
        self.query_occluded_async(rays, out)
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy().astype(bool)

    # ---- radiance queries (include/rt_abi.h rt_query_radiance_async) ----
    def query_radiance_async(self, rays, out, depth=0, stream=None):
        """Enqueue radiance queries: out[i] = traceRay(rays[i], depth) against
        the current scene (depth 0: the scene's). `rays` as for
        query_closest_async, `out` a uint8 CUDA tensor of n * 32 bytes
        (abi.RADIANCE_DTYPE). Radiance queries on one context share a
        workspace: keep them ordered with respect to each other."""
        n = self._query_args(rays, out, abi.RADIANCE_DTYPE.itemsize, "query_radiance_async")
        s = self.torch.cuda.current_stream(self.device) if stream is None else stream
        _check(self.lib.rt_query_radiance_async(self.handle, n, C.c_void_p(rays.data_ptr()), int(depth),
                                                C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream)),
               "rt_query_radiance_async")

    def radiance_lanes(self, depth=0):
        """Lanes of the persistent grid a radiance query at `depth` runs on at most."""
        n = self.lib.rt_query_radiance_lanes(self.handle, int(depth))
        if n < 0:
            _check(n, "rt_query_radiance_lanes")
        return n

    def radiance(self, origins, dirs, depth=None, tmax=None, exclude=None):
        """Synchronous radiance queries for numpy [n, 3] float64 origins and
        directions (depth None: the scene's; tmax, exclude as closest_hits)
        -> abi.RADIANCE_DTYPE array [n]."""
        torch = self.torch
        n, rays = self._upload_rays(origins, dirs, tmax, exclude)
        out = torch.empty(n * abi.RADIANCE_DTYPE.itemsize, dtype=torch.uint8, device=rays.device)
        self.query_radiance_async(rays, out, 0 if depth is None else depth)
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy().view(abi.RADIANCE_DTYPE)

    def camera_rays_async(self, y0, y1, out, stream=None):
        """Enqueue the reference camera's rays of rows [y0, y1): `out` a uint8
        CUDA tensor of (y1 - y0) * W * 4 records of 64 bytes (abi.RAY_DTYPE),
        in [row][x][sample] order."""
        torch = self.torch
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous(), \
            "camera_rays_async: out must be a contiguous uint8 CUDA tensor"
        assert out.device.index == self.device, "camera_rays_async: out is on another device"
        rows = max(0, int(y1) - int(y0))
        assert out.numel() == rows * self.packed.width * 4 * abi.RAY_DTYPE.itemsize, \
            "camera_rays_async: output tensor size does not match %d rows" % rows
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        _check(self.lib.rt_query_camera_rays_async(self.handle, int(y0), int(y1), C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(s.cuda_stream)), "rt_query_camera_rays_async")

    def camera_rays(self, y0=0, y1=None):
        """Synchronous camera rays of rows [y0, y1) -> numpy abi.RAY_DTYPE array [rows, W, 4]."""
        torch = self.torch
        if y1 is None:
            y1 = self.packed.height
        w = self.packed.width
        rows = max(0, y1 - y0)
        out = torch.empty(rows * w * 4 * abi.RAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:%d" % self.device)
        self.camera_rays_async(y0, y1, out)
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy().view(abi.RAY_DTYPE).reshape(rows, w, 4)

    # ---- camera renders (include/rt_abi.h rt_camera, rt_render_camera_async) ----
    @staticmethod
    def camera(model="pinhole", samples=0, size=None, depth=0, chunk_pixels=0, fov=0.0, extent=0.0, aperture=0.0,
               focus=0.0, eye=None, look_at=None, up=None):
        """An abi.rt_camera. No arguments: the scene's own camera at 4 samples
        (Render()). `model` a name of abi.CAMERA_MODELS or an RT_CAMERA_*
        value; `size` (width, height); giving any of eye / look_at / up poses
        the camera (defaults: the reference's eye (0, 0, -1) looking at the
        origin, up (0, 1, 0))."""
        cam = abi.rt_camera()
        cam.model = abi.CAMERA_MODELS[model] if isinstance(model, str) else int(model)
        cam.samples = int(samples)
        if size is not None:
            cam.width, cam.height = int(size[0]), int(size[1])
        cam.depth = int(depth)
        cam.chunk_pixels = int(chunk_pixels)
        cam.fov, cam.extent, cam.aperture, cam.focus = float(fov), float(extent), float(aperture), float(focus)
        if eye is not None or look_at is not None or up is not None:
            cam.flags = abi.RT_CAMERA_POSED
            cam.eye[:] = [float(v) for v in ((0.0, 0.0, -1.0) if eye is None else eye)]
            cam.look_at[:] = [float(v) for v in ((0.0, 0.0, 0.0) if look_at is None else look_at)]
            cam.up[:] = [float(v) for v in ((0.0, 1.0, 0.0) if up is None else up)]
        return cam

    def _camera_frame(self, cam):
        """(cam or the zero camera, W, H, samples) of a camera render."""
        cam = abi.rt_camera() if cam is None else cam
        w = int(cam.width) or self.packed.width
        h = int(cam.height) or self.packed.height
        return cam, w, h, int(cam.samples) or 4

    def _camera_out(self, t, nbytes, what, name):
        assert t.is_cuda and t.is_contiguous(), "%s: %s must be a contiguous CUDA tensor" % (what, name)
        assert t.device.index == self.device, "%s: %s is on another device" % (what, name)
        assert t.numel() * t.element_size() == nbytes, "%s: %s must hold %d bytes" % (what, name, nbytes)
        return C.c_void_p(t.data_ptr())

    def camera_rays_ex_async(self, cam, y0, y1, out, stream=None):
        """Enqueue the rays of camera `cam` (None: the zero camera) for rows
        [y0, y1) of its frame: `out` a uint8 CUDA tensor of (y1 - y0) * W *
        samples records of 64 bytes (abi.RAY_DTYPE), in [row][x][sample] order."""
        cam, w, _, S = self._camera_frame(cam)
        rows = max(0, int(y1) - int(y0))
        assert out.dtype == self.torch.uint8, "camera_rays_ex_async: out must be a uint8 tensor"
        ptr = self._camera_out(out, rows * w * S * abi.RAY_DTYPE.itemsize, "camera_rays_ex_async", "out")
        s = self.torch.cuda.current_stream(self.device) if stream is None else stream
        _check(self.lib.rt_camera_rays_async(self.handle, C.byref(cam), int(y0), int(y1), ptr,
                                             C.c_void_p(s.cuda_stream)), "rt_camera_rays_async")

    def camera_rays_ex(self, cam=None, y0=0, y1=None):
        """Synchronous rays of camera `cam` for rows [y0, y1) -> numpy
        abi.RAY_DTYPE array [rows, W, samples]."""
        torch = self.torch
        cam, w, h, S = self._camera_frame(cam)
        if y1 is None:
            y1 = h
        rows = max(0, y1 - y0)
        out = torch.empty(rows * w * S * abi.RAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:%d" % self.device)
        self.camera_rays_ex_async(cam, y0, y1, out)
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy().view(abi.RAY_DTYPE).reshape(rows, w, S)

    def render_camera_async(self, cam, y0, y1, rgba=None, mean=None, stream=None, var=None):
        """Enqueue the camera render of rows [y0, y1) of `cam`'s frame (None:
        the zero camera, Render()'s pixels) into either or both of `rgba`, a
        uint8 CUDA tensor [rows, W, 4], and `mean`, a float64 CUDA tensor
        [rows, W, 3] (the mean radiance before quantisation). `var`, a float64
        CUDA tensor [rows, W, 3], receives the variance of each pixel's mean
        (rt_render_camera_var_async; needs at least 2 samples). Camera renders
        and radiance queries on one context share a workspace: keep them
        ordered with respect to each other."""
        torch = self.torch
        cam, w, _, _ = self._camera_frame(cam)
        rows = max(0, int(y1) - int(y0))
        rp = mp = None
        if var is not None:
            assert var.dtype == torch.float64, "render_camera_async: var must be a float64 tensor"
            vp = self._camera_out(var, rows * w * 24, "render_camera_async", "var")
        if rgba is not None:
            assert rgba.dtype == torch.uint8, "render_camera_async: rgba must be a uint8 tensor"
            rp = self._camera_out(rgba, rows * w * 4, "render_camera_async", "rgba")
        if mean is not None:
            assert mean.dtype == torch.float64, "render_camera_async: mean must be a float64 tensor"
            mp = self._camera_out(mean, rows * w * 24, "render_camera_async", "mean")
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        if var is not None:
            _check(self.lib.rt_render_camera_var_async(self.handle, C.byref(cam), int(y0), int(y1), rp, mp, vp,
                                                       C.c_void_p(s.cuda_stream)), "rt_render_camera_var_async")
            return
        _check(self.lib.rt_render_camera_async(self.handle, C.byref(cam), int(y0), int(y1), rp, mp,
                                               C.c_void_p(s.cuda_stream)), "rt_render_camera_async")

    def render_camera(self, cam=None, y0=0, y1=None, mean=False, var=False):
        """Synchronous camera render of rows [y0, y1) -> numpy uint8 [rows, W,
        4]; with mean=True and / or var=True -> a tuple of that, the float64
        [rows, W, 3] mean radiance and the float64 [rows, W, 3] variance of
        that mean, in this order."""
        torch = self.torch
        cam, w, h, _ = self._camera_frame(cam)
        if y1 is None:
            y1 = h
        rows = max(0, y1 - y0)
        dev = "cuda:%d" % self.device
        rgba = torch.empty((rows, w, 4), dtype=torch.uint8, device=dev)
        m = torch.empty((rows, w, 3), dtype=torch.float64, device=dev) if mean else None
        v = torch.empty((rows, w, 3), dtype=torch.float64, device=dev) if var else None
        self.render_camera_async(cam, y0, y1, rgba, m, var=v)
        torch.cuda.synchronize(self.device)
        out = [t.cpu().numpy() for t in (rgba, m, v) if t is not None]
        return out[0] if len(out) == 1 else tuple(out)

    def render_camera_chunks(self, cam=None, y0=0, y1=None):
        """Launches of the radiance kernel render_camera_async makes for these arguments."""
        cam, _, h, _ = self._camera_frame(cam)
        n = self.lib.rt_render_camera_chunks(self.handle, C.byref(cam), int(y0), int(h if y1 is None else y1))
        if n < 0:
            _check(n, "rt_render_camera_chunks")
        return n

    # ---- adaptive camera renders (include/rt_abi.h rt_adaptive, rt_render_camera_adaptive_async) ----
    @staticmethod
    def adaptive(tolerance, min_samples=0):
        """An abi.rt_adaptive: pixels stop once the standard error of their
        mean is at most `tolerance` in every channel, after at least
        `min_samples` samples (0: min(4, the camera's samples))."""
        ad = abi.rt_adaptive()
        ad.tolerance = float(tolerance)
        ad.min_samples = int(min_samples)
        return ad

    def render_camera_adaptive_async(self, cam, ad, y0, y1, rgba=None, mean=None, samples=None, stream=None,
                                     var=None):
        """Enqueue the adaptive camera render of rows [y0, y1) of `cam`'s
        frame, whose samples are the cap, into any of `rgba` (uint8 [rows, W,
        4]), `mean` (float64 [rows, W, 3]) and `samples` (int32 [rows, W]: the
        samples each pixel took) and `var` (float64 [rows, W, 3]: the variance
        of each pixel's mean at the count it ends with;
        rt_render_camera_adaptive_var_async), all CUDA tensors. Ordering as
        render_camera_async."""
        torch = self.torch
        who = "render_camera_adaptive_async"
        cam, w, _, _ = self._camera_frame(cam)
        rows = max(0, int(y1) - int(y0))
        rp = mp = sp = None
        if rgba is not None:
            assert rgba.dtype == torch.uint8, who + ": rgba must be a uint8 tensor"
            rp = self._camera_out(rgba, rows * w * 4, who, "rgba")
        if mean is not None:
            assert mean.dtype == torch.float64, who + ": mean must be a float64 tensor"
            mp = self._camera_out(mean, rows * w * 24, who, "mean")
        if samples is not None:
            assert samples.dtype == torch.int32, who + ": samples must be an int32 tensor"
            sp = self._camera_out(samples, rows * w * 4, who, "samples")
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        if var is not None:
            assert var.dtype == torch.float64, who + ": var must be a float64 tensor"
            vp = self._camera_out(var, rows * w * 24, who, "var")
            _check(self.lib.rt_render_camera_adaptive_var_async(self.handle, C.byref(cam), C.byref(ad), int(y0),
                                                                int(y1), rp, mp, sp, vp, C.c_void_p(s.cuda_stream)),
                   "rt_render_camera_adaptive_var_async")
            return
        _check(self.lib.rt_render_camera_adaptive_async(self.handle, C.byref(cam), C.byref(ad), int(y0), int(y1), rp, mp,
                                                        sp, C.c_void_p(s.cuda_stream)),
               "rt_render_camera_adaptive_async")

    def render_camera_adaptive(self, cam, ad, y0=0, y1=None, mean=False, samples=False, var=False):
        """Synchronous adaptive camera render of rows [y0, y1) -> numpy uint8
        [rows, W, 4]; with mean=True, samples=True and / or var=True -> a
        tuple of that, the float64 [rows, W, 3] mean radiance, the int32
        [rows, W] sample counts and the float64 [rows, W, 3] variance of the
        mean, in this order."""
        torch = self.torch
        cam, w, h, _ = self._camera_frame(cam)
        if y1 is None:
            y1 = h
        rows = max(0, y1 - y0)
        dev = "cuda:%d" % self.device
        rgba = torch.empty((rows, w, 4), dtype=torch.uint8, device=dev)
        m = torch.empty((rows, w, 3), dtype=torch.float64, device=dev) if mean else None
        n = torch.empty((rows, w), dtype=torch.int32, device=dev) if samples else None
        v = torch.empty((rows, w, 3), dtype=torch.float64, device=dev) if var else None
        self.render_camera_adaptive_async(cam, ad, y0, y1, rgba, m, n, var=v)
        torch.cuda.synchronize(self.device)
        out = [t.cpu().numpy() for t in (rgba, m, n, v) if t is not None]
        return out[0] if len(out) == 1 else tuple(out)

    def render_camera_adaptive_plan(self, cam, ad, y0=0, y1=None):
        """(chunks, passes per chunk) render_camera_adaptive_async launches for these arguments."""
        cam, _, h, _ = self._camera_frame(cam)
        chunks, passes = C.c_int(0), C.c_int(0)
        _check(self.lib.rt_render_camera_adaptive_plan(self.handle, C.byref(cam), C.byref(ad), int(y0),
                                                       int(h if y1 is None else y1), C.byref(chunks), C.byref(passes)),
               "rt_render_camera_adaptive_plan")
        return chunks.value, passes.value

    # ---- feature buffers (include/rt_abi.h rt_aov_out, rt_render_camera_aov_async) ----
    def render_camera_aov_async(self, cam, y0, y1, depth=None, normal=None, albedo=None, coverage=None, ids=None,
                                stream=None):
        """Enqueue the feature buffers of rows [y0, y1) of `cam`'s frame (None:
        the zero camera) into any of `depth` [rows, W], `normal` [rows, W, 3],
        `albedo` [rows, W, 3], `coverage` [rows, W] (float64 CUDA tensors) and
        `ids` (int32 [rows, W, 4]: sample 0's object, face, kind, material).
        One launch, nothing allocated; needs no ordering with the context's
        other calls."""
        torch = self.torch
        who = "render_camera_aov_async"
        cam, w, _, _ = self._camera_frame(cam)
        n = max(0, int(y1) - int(y0)) * w
        out = abi.rt_aov_out()
        for name, t, per in (("depth", depth, 1), ("normal", normal, 3), ("albedo", albedo, 3),
                             ("coverage", coverage, 1)):
            if t is not None:
                assert t.dtype == torch.float64, "%s: %s must be a float64 tensor" % (who, name)
                setattr(out, name, self._camera_out(t, n * per * 8, who, name).value)
        if ids is not None:
            assert ids.dtype == torch.int32, who + ": ids must be an int32 tensor"
            out.ids = self._camera_out(ids, n * 16, who, "ids").value
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        _check(self.lib.rt_render_camera_aov_async(self.handle, C.byref(cam), int(y0), int(y1), C.byref(out),
                                                   C.c_void_p(s.cuda_stream)), "rt_render_camera_aov_async")

    def render_camera_aov(self, cam=None, y0=0, y1=None, which=abi.AOV_NAMES):
        """Synchronous feature buffers of rows [y0, y1) -> a dict of numpy
        arrays for the names in `which` (abi.AOV_NAMES): float64 depth and
        coverage [rows, W], normal and albedo [rows, W, 3], and ids, an
        abi.AOV_IDS_DTYPE array [rows, W]."""
        torch = self.torch
        cam, w, h, _ = self._camera_frame(cam)
        if y1 is None:
            y1 = h
        rows = max(0, y1 - y0)
        dev = "cuda:%d" % self.device
        shapes = {"depth": (rows, w), "normal": (rows, w, 3), "albedo": (rows, w, 3), "coverage": (rows, w),
                  "ids": (rows, w, 4)}
        bufs = {}
        for name in which:
            if name not in shapes:
                raise ValueError("unknown feature buffer %r (one of %s)" % (name, ", ".join(abi.AOV_NAMES)))
            bufs[name] = torch.empty(shapes[name], dtype=torch.int32 if name == "ids" else torch.float64, device=dev)
        self.render_camera_aov_async(cam, y0, y1, stream=None, **bufs)
        torch.cuda.synchronize(self.device)
        out = {k: t.cpu().numpy() for k, t in bufs.items()}
        if "ids" in out:
            out["ids"] = out["ids"].view(abi.AOV_IDS_DTYPE).reshape(rows, w)
        return out

    # ---- the guided a-trous denoiser (include/rt_abi.h rt_denoise, rt_denoise_atrous_async) ----
    @staticmethod
    def denoise_params(iterations=0, color=0.0, normal=0.0, depth=0.0, albedo=0.0):
        """An abi.rt_denoise: `iterations` 1..8 (0: 5) and the sigma of each
        term (0 or +inf: the term is off)."""
        dn = abi.rt_denoise()
        dn.iterations = int(iterations)
        dn.sigma_color, dn.sigma_normal = float(color), float(normal)
        dn.sigma_depth, dn.sigma_albedo = float(depth), float(albedo)
        return dn

    def denoise_async(self, params, color, out, tmp=None, normal=None, depth=None, albedo=None, rgba=None,
                      stream=None, var=None, var_out=None, var_tmp=None):
        """Enqueue the a-trous filter of the whole frame `color` (float64 CUDA
        tensor [H, W, 3], never written) into `out` (same shape), one launch
        per iteration. `tmp` (same shape) is needed for more than one
        iteration; the guides `normal` [H, W, 3], `depth` [H, W] and `albedo`
        [H, W, 3] are needed where their term is on; `rgba` (uint8 [H, W, 4])
        optionally receives the quantised result. Needs no scene.
        Giving `var` (float64 [H, W, 3], the variance of `color`, never
        written) selects the variance-guided filter
        (rt_denoise_atrous_var_async): params.sigma_color is then in standard
        deviations, and `var_out` and `var_tmp` (float64 [H, W]) are both
        needed; `var_out` receives the filtered frame's variance estimate."""
        torch = self.torch
        who = "denoise_async"
        assert color.dim() == 3 and color.shape[2] == 3, who + ": color must be [H, W, 3]"
        h, w = int(color.shape[0]), int(color.shape[1])
        assert var is not None or (var_out is None and var_tmp is None), who + ": var_out and var_tmp need var"
        assert var is None or (var_out is not None and var_tmp is not None), who + ": var needs var_out and var_tmp"
        ptrs = []
        for name, t, per in (("color", color, 3), ("normal", normal, 3), ("depth", depth, 1), ("albedo", albedo, 3),
                             ("out", out, 3), ("tmp", tmp, 3)):
            if t is None:
                ptrs.append(None)
                continue
            assert t.dtype == torch.float64, "%s: %s must be a float64 tensor" % (who, name)
            ptrs.append(self._camera_out(t, h * w * per * 8, who, name))
        rp = None
        if rgba is not None:
            assert rgba.dtype == torch.uint8, who + ": rgba must be a uint8 tensor"
            rp = self._camera_out(rgba, h * w * 4, who, "rgba")
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        if var is not None:
            vps = []
            for name, t, per in (("var", var, 3), ("var_out", var_out, 1), ("var_tmp", var_tmp, 1)):
                assert t.dtype == torch.float64, "%s: %s must be a float64 tensor" % (who, name)
                vps.append(self._camera_out(t, h * w * per * 8, who, name))
            _check(self.lib.rt_denoise_atrous_var_async(self.handle, C.byref(params), w, h, ptrs[0], vps[0], *ptrs[1:],
                                                        vps[1], vps[2], rp, C.c_void_p(s.cuda_stream)),
                   "rt_denoise_atrous_var_async")
            return
        _check(self.lib.rt_denoise_atrous_async(self.handle, C.byref(params), w, h, *ptrs, rp,
                                                C.c_void_p(s.cuda_stream)), "rt_denoise_atrous_async")

    def denoise(self, mean, normal=None, depth=None, albedo=None, params=None, rgba=False, var=None,
                variance_out=False):
        """Synchronous a-trous filter of a numpy float64 [H, W, 3] mean with
        the given guides (numpy arrays as render_camera_aov returns them) ->
        float64 [H, W, 3]; with rgba=True -> (that, uint8 [H, W, 4]). `params`
        None: denoise_params() with DENOISE_DEFAULTS for the guides given.
        Giving `var`, the float64 [H, W, 3] variance of `mean` as
        render_camera(var=True) returns it, selects the variance-guided
        filter: the colour sigma is then in standard deviations (`params`
        None: DENOISE_VAR_COLOR), and variance_out=True appends the filtered
        frame's float64 [H, W] variance estimate to the result."""
        torch = self.torch
        dev = "cuda:%d" % self.device
        if var is None and variance_out:
            raise ValueError("denoise: variance_out needs var")
        if var is not None and np.shape(var) != np.shape(mean):
            raise ValueError("denoise: var must have the shape of mean")
        if params is None:
            d = DENOISE_DEFAULTS
            params = self.denoise_params(0, d["color"] if var is None else DENOISE_VAR_COLOR,
                                         d["normal"] if normal is not None else 0.0,
                                         d["depth"] if depth is not None else 0.0,
                                         d["albedo"] if albedo is not None else 0.0)

        def up(a):
            return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)

        color = up(mean)
        out = torch.empty_like(color)
        k = int(params.iterations) or 5
        tmp = torch.empty_like(color) if k > 1 else None
        img = torch.empty(tuple(color.shape[:2]) + (4,), dtype=torch.uint8, device=dev) if rgba else None
        vo = vt = None
        if var is not None:
            vo = torch.empty(tuple(color.shape[:2]), dtype=torch.float64, device=dev)
            vt = torch.empty_like(vo)
        self.denoise_async(params, color, out, tmp, up(normal), up(depth), up(albedo), img, var=up(var), var_out=vo,
                           var_tmp=vt)
        torch.cuda.synchronize(self.device)
        res = [out.cpu().numpy()]
        if rgba:
            res.append(img.cpu().numpy())
        if variance_out:
            res.append(vo.cpu().numpy())
        return res[0] if len(res) == 1 else tuple(res)

    def image_from_radiance(self, out, samples):
        """Average `samples` consecutive radiance records per pixel and quantise
        as Render() does (raytracer.go:651-656, vec.go:104-107): `out` a uint8
        CUDA tensor of rows * W * samples records -> uint8 [rows, W, 4] CUDA
        tensor. The samples are added in order, ((s0 + s1) + s2) + ..., in
        float64, then scaled by 1.0 / samples."""
        torch = self.torch
        rec = abi.RADIANCE_DTYPE.itemsize
        w = self.packed.width
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous(), \
            "image_from_radiance: out must be a contiguous uint8 CUDA tensor"
        assert samples >= 1 and out.numel() % (rec * w * samples) == 0, \
            "image_from_radiance: out must hold rows * W * samples records"
        rows = out.numel() // (rec * w * samples)
        col = out.view(torch.float64).view(rows, w, samples, rec // 8)[..., :3]
        total = col[:, :, 0, :].clone()
        for k in range(1, samples):
            total = total + col[:, :, k, :]
        c = total * (1.0 / samples)
        # uint32(c * 65535) >> 8 as Go converts on amd64: through int64, truncated
        # to 32 bits; NaN and values outside (-2^63, 2^63) give 0
        v = c * 65535.0
        ok = (v > -9223372036854775808.0) & (v < 9223372036854775808.0)
        q = (torch.where(ok, v, torch.zeros_like(v)).to(torch.int64) & 0xffffffff) >> 8
        img = torch.empty((rows, w, 4), dtype=torch.uint8, device=out.device)
        img[..., :3] = (q & 0xff).to(torch.uint8)
        img[..., 3] = 255
        return img


def kernel_source_id():
    """Identifier of the device code and its launch configuration (sha256 of
    the kernel sources and of rt_kernel.hip -- occupancy bounds, hipRTC flags,
    schedule choice, tile order, grid sizing -- 16 hex digits): stored with
    committed PMC summaries so that a bench line only quotes counters recorded
    with the kernel and launches it times."""
    import hashlib
    h = hashlib.sha256()
    root = os.path.dirname(PKG_DIR)
    for rel in ("include/rt_abi.h", "go-raytracer_amd/csrc/rt_device.h", "go-raytracer_amd/csrc/rt_render.h",
                "go-raytracer_amd/csrc/rt_kernel.hip"):
        with open(os.path.join(root, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def spec_precompile(kinds, features=0, nlights=0):
    """Compile (no device needed) the specialised kernel for a scene whose
    objects have these primitive kinds, in order, RT_SPEC_* feature bits
    (abi.RT_SPEC_SURFACES / _DIRECTIONAL / _SPOT) and light count (1..8; the
    scene's own count, which rt_set_scene specialises on); returns the compile
    time (ms, 0 if already cached in this process)."""
    lib = load_library()
    features = int(features) | (int(nlights) << 8)
    arr = (C.c_int * len(kinds))(*[int(k) for k in kinds])
    ms = C.c_double()
    _check(lib.rt_spec_precompile(len(kinds), arr, int(features), C.byref(ms)), "rt_spec_precompile")
    return ms.value


def render_opts(devices=None, gather="auto", out_device=False, generic=False, spec_sync=False, bands=0):
    """abi.rt_render_opts for rt_render_ex. devices: None (the current
    device), an int N (devices 0..N-1) or a list of ordinals (repeats allowed:
    one GPU rendering several shares, each with its own contexts)."""
    o = abi.rt_render_opts()
    flags = 0
    if isinstance(devices, int):
        o.device_count = devices
    elif devices is not None:
        devices = [int(d) for d in devices]
        if not 1 <= len(devices) <= abi.RT_MAX_DEVICES:
            raise ValueError("1..%d devices" % abi.RT_MAX_DEVICES)
        o.device_count = len(devices)
        for k, d in enumerate(devices):
            o.devices[k] = d
        flags |= abi.RT_RENDER_DEVICE_LIST
    o.gather = {"auto": abi.RT_GATHER_AUTO, "host": abi.RT_GATHER_HOST, "peer": abi.RT_GATHER_PEER}[gather]
    flags |= (abi.RT_RENDER_OUT_DEVICE if out_device else 0) | (abi.RT_RENDER_GENERIC if generic else 0) | \
        (abi.RT_RENDER_SPEC_SYNC if spec_sync else 0)
    o.flags = flags
    o.bands = int(bands)
    return o


def render_frame(scene_or_args, devices=None, gather="auto", generic=False, spec_sync=False, bands=0, out=None):
    """One synchronous frame through rt_render_ex (include/rt_abi.h): the
    Render() seam over one or several GPUs of this process. Returns (image
    numpy uint8 [H, W, 4], abi.rt_stats, abi.rt_render_timing). `out`: a
    caller-owned host array to render into (reused across calls)."""
    lib = load_library()
    p = _packed(scene_or_args)
    if out is None:
        out = np.empty((p.height, p.width, 4), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size == p.height * p.width * 4
    o = render_opts(devices, gather, False, generic, spec_sync, bands)
    st = abi.rt_stats()
    _check(lib.rt_render_ex(p.ref(), C.byref(o), out.ctypes.data_as(C.c_void_p), C.byref(st)), "rt_render_ex")
    tm = abi.rt_render_timing()
    _check(lib.rt_render_last_timing(C.byref(tm)), "rt_render_last_timing")
    return out, st, tm


def debug_assemble(width, height, shares, bands=0):
    """The host side of rt_render_ex's multi-device assembly on host buffers
    (include/rt_abi.h rt_debug_assemble; no device): shares[d] = device d's
    packed tile rows. Returns the assembled frame."""
    lib = load_library()
    shares = [np.ascontiguousarray(s, dtype=np.uint8) for s in shares]
    ptrs = (C.c_void_p * len(shares))(*[s.ctypes.data for s in shares])
    out = np.zeros((height, width, 4), np.uint8)
    _check(lib.rt_debug_assemble(int(width), int(height), len(shares), int(bands), ptrs,
                                 out.ctypes.data_as(C.c_void_p)), "rt_debug_assemble")
    return out


def Render(scene_or_args, return_stats=False):
    """Render(scene) -> RGBA8 image as numpy [H, W, 4] (Go image.RGBA.Pix layout),
    raytracer.go:589-682. Runs on the current HIP device."""
    ctx = RenderContext()
    try:
        ctx.set_scene(scene_or_args)
        ctx.read_stats(reset=True)
        img = ctx.render()
        st = ctx.read_stats(reset=True)
    finally:
        ctx.close()
    return (img, st) if return_stats else img
