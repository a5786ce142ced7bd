"""ctypes mirror of include/rt_abi.h (the C ABI of the renderer).

Struct layouts must match include/rt_abi.h exactly; tests/test_abi.py checks
sizes and offsets against the compiled library's expectations.
"""
import ctypes as C

import numpy as np

RT_ABI_VERSION = 6  # include/rt_abi.h
RT_MAX_DEVICES = 16
RT_EXP_AMD64_FMA, RT_EXP_AMD64, RT_EXP_PORTABLE = 0, 1, 2  # rt_scene.exp_mode

RT_OK = 0
RT_E_INVALID = -1
RT_E_SINGULAR = -2
RT_E_DEVICE = -3
RT_E_NOMEM = -4

RT_SPHERE, RT_PLANE, RT_CUBE, RT_CYLINDER, RT_CONE, RT_CSG = 0, 1, 2, 3, 4, 5
RT_NUM_KINDS = 6
RT_MAX_FACES = 6
KIND_NAMES = ("sphere", "plane", "cube", "cylinder", "cone", "csg")
RT_CSG_UNION, RT_CSG_INTERSECT, RT_CSG_DIFFERENCE = -1, -2, -3
RT_CSG_MAX_LEAVES = 128
RT_VM_EXT_ASIN, RT_VM_EXT_ACOS, RT_VM_EXT_REAL = 32, 33, 34  # surface bytecode, contest extensions
RT_SPEC_SURFACES, RT_SPEC_DIRECTIONAL, RT_SPEC_SPOT = 1, 2, 4  # rt_spec_precompile feature bits
RT_ACCEL_BVH, RT_ACCEL_CULL = 1, 2  # rt_set_accel flags
RT_SCHED_AUTO, RT_SCHED_PIXEL, RT_SCHED_QUADS, RT_SCHED_PAIRS = 0, 1, 2, 3  # rt_set_schedule modes
RT_INFO_LDS, RT_INFO_BVH, RT_INFO_CSG, RT_INFO_STREAM, RT_INFO_WAVEFRONT, RT_INFO_ORDERED = 1, 2, 4, 8, 16, 32  # rt_scene_info
RT_INFO_SHARE_DEVICE = 64
RT_SHARE_OFF, RT_SHARE_GROUP, RT_SHARE_DEVICE, RT_SHARE_AUTO = 0, 1, 2, 3  # rt_set_work_sharing
RT_GATHER_AUTO, RT_GATHER_HOST, RT_GATHER_PEER = 0, 1, 2  # rt_render_opts.gather
RT_RENDER_DEVICE_LIST, RT_RENDER_OUT_DEVICE, RT_RENDER_GENERIC, RT_RENDER_SPEC_SYNC = 1, 2, 4, 8  # rt_render_opts.flags


def RT_SPEC_LIGHTS(n):
    """rt_spec_precompile feature bits for exactly n (1..8) lights (include/rt_abi.h)."""
    return int(n) << 8
RT_LIGHT_POINT, RT_LIGHT_DIRECTIONAL, RT_LIGHT_SPOT = 0, 1, 2


class rt_material(C.Structure):
    _fields_ = [
        ("color", C.c_double * 3),
        ("reflectivity", C.c_double),
        ("fuzziness", C.c_double),
        ("transparency", C.c_double),
        ("refractive_index", C.c_double),
        ("kd", C.c_double),
        ("ks", C.c_double),
        ("specular_exponent", C.c_double),
    ]


class rt_point_light(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("color", C.c_double * 3)]


class rt_light(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("reserved", C.c_int32),
        ("position", C.c_double * 3),
        ("direction", C.c_double * 3),
        ("color", C.c_double * 3),
        ("cutoff", C.c_double),
        ("exponent", C.c_double),
    ]


class rt_object(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("has_transform", C.c_int32),
        ("material", C.c_int32 * RT_MAX_FACES),
        ("transform", C.c_double * 16),
        ("plane_point", C.c_double * 3),
        ("plane_normal", C.c_double * 3),
        ("csg_first", C.c_int32),
        ("csg_count", C.c_int32),
        ("csg_code", C.c_int32),
        ("csg_code_len", C.c_int32),
    ]


class rt_scene(C.Structure):
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("depth", C.c_int32),
        ("num_lights", C.c_int32),
        ("fov", C.c_double),
        ("ambient", C.c_double * 3),
        ("bg_start", C.c_double * 3),
        ("bg_end", C.c_double * 3),
        ("lights", C.POINTER(rt_point_light)),
        ("objects", C.POINTER(rt_object)),
        ("materials", C.POINTER(rt_material)),
        ("num_objects", C.c_int32),
        ("num_materials", C.c_int32),
        ("program_code", C.POINTER(C.c_uint32)),
        ("program_consts", C.POINTER(C.c_uint64)),
        ("program_entry", C.POINTER(C.c_int32)),
        ("num_programs", C.c_int32),
        ("program_code_words", C.c_int32),
        ("program_const_count", C.c_int32),
        ("exp_mode", C.c_int32),  # RT_EXP_*
        ("ext_lights", C.POINTER(rt_light)),
        ("num_ext_lights", C.c_int32),
        ("reserved1", C.c_int32),
        ("csg_leaves", C.POINTER(rt_object)),
        ("csg_code", C.POINTER(C.c_int32)),
        ("num_csg_leaves", C.c_int32),
        ("csg_code_words", C.c_int32),
    ]


class rt_stats(C.Structure):
    _fields_ = [
        ("primary_rays", C.c_uint64),
        ("secondary_rays", C.c_uint64),
        ("shadow_rays", C.c_uint64),
        ("tests", C.c_uint64 * RT_NUM_KINDS),
        ("shadow_tests", C.c_uint64 * RT_NUM_KINDS),
        ("shaded_hits", C.c_uint64),
        ("surface_errors", C.c_uint64),
        ("kernel_ms", C.c_double),
        # ABI 6: rt_render_ex's devices, per-device GPU span, exposed gather time
        ("devices", C.c_int32),
        ("reserved2", C.c_int32),
        ("device_kernel_ms", C.c_double * RT_MAX_DEVICES),
        ("gather_ms", C.c_double),
    ]

    def as_dict(self):
        return {
            "primary_rays": int(self.primary_rays),
            "secondary_rays": int(self.secondary_rays),
            "shadow_rays": int(self.shadow_rays),
            "tests": [int(v) for v in self.tests],
            "shadow_tests": [int(v) for v in self.shadow_tests],
            "shaded_hits": int(self.shaded_hits),
            "surface_errors": int(self.surface_errors),
        }

    def total_rays(self):
        return int(self.primary_rays) + int(self.secondary_rays) + int(self.shadow_rays)


class rt_render_timing(C.Structure):
    """Parts of the calling thread's last rt_render call (ABI 5), one host
    timeline: setup + render_wait + copy_tail = total."""
    _fields_ = [
        ("total_ms", C.c_double),
        ("setup_ms", C.c_double),
        ("render_wait_ms", C.c_double),
        ("copy_tail_ms", C.c_double),
        ("gpu_ms", C.c_double),
        ("bands", C.c_int32),
        ("scene_reused", C.c_int32),
        ("specialized", C.c_int32),
        ("devices", C.c_int32),
        ("pending_compiles", C.c_int32),
        ("reserved", C.c_int32),
    ]

    def as_dict(self):
        return {k: (round(getattr(self, k), 4) if isinstance(getattr(self, k), float) else int(getattr(self, k)))
                for k, _ in self._fields_ if k != "reserved"}


class rt_render_opts(C.Structure):
    """rt_render_ex options (ABI 6): devices, gather mode, flags, bands."""
    _fields_ = [
        ("device_count", C.c_int32),
        ("device_mask", C.c_uint32),
        ("devices", C.c_int32 * RT_MAX_DEVICES),
        ("gather", C.c_int32),
        ("flags", C.c_int32),
        ("bands", C.c_int32),
        ("reserved", C.c_int32 * 5),
    ]


class rt_ray(C.Structure):
    """One query ray (rt_query_*_async): 64 bytes, arrays 16-byte aligned."""
    _fields_ = [
        ("origin", C.c_double * 3),
        ("dir", C.c_double * 3),  # used as given: t is in units of |dir|
        ("tmax", C.c_double),     # a result counts when T < tmax (+inf: no limit)
        ("exclude", C.c_int32),   # top-level object index left out, -1: none
        ("reserved", C.c_int32),
    ]


class rt_hit(C.Structure):
    """One closest-hit record: 96 bytes. A miss is object = -1 and zero elsewhere."""
    _fields_ = [
        ("t", C.c_double),
        ("point_obj", C.c_double * 3),
        ("point_world", C.c_double * 3),
        ("normal_world", C.c_double * 3),
        ("object", C.c_int32),
        ("face", C.c_int32),      # composites: (leaf << 4) | (flip << 3) | leaf_face
        ("kind", C.c_int32),      # of the surface (the leaf's for a composite)
        ("material", C.c_int32),  # >= 0 material index, < 0 closure program -(p+1)
    ]


class rt_radiance(C.Structure):
    """One radiance record (rt_query_radiance_async): 32 bytes."""
    _fields_ = [
        ("color", C.c_double * 3),  # what traceRay returns for the ray
        ("object", C.c_int32),      # top-level object the ray itself hit, -1: background
        ("rays", C.c_int32),        # rays traced for this query (1 + secondary rays)
    ]


RT_RADIANCE_MAX_DEPTH = 32

# camera renders (rt_camera_rays_async, rt_render_camera_async)
RT_CAMERA_PINHOLE, RT_CAMERA_ORTHO, RT_CAMERA_EQUIRECT, RT_CAMERA_THINLENS = 0, 1, 2, 3
RT_CAMERA_POSED = 1  # rt_camera.flags
RT_CAMERA_MAX_SAMPLES = 1024
CAMERA_MODELS = {"pinhole": RT_CAMERA_PINHOLE, "ortho": RT_CAMERA_ORTHO, "equirect": RT_CAMERA_EQUIRECT,
                 "thinlens": RT_CAMERA_THINLENS}


class rt_camera(C.Structure):
    """A camera render's camera. All zero = the scene's own camera at 4
    samples: Render()."""
    _fields_ = [
        ("model", C.c_int32),         # RT_CAMERA_*
        ("flags", C.c_int32),         # RT_CAMERA_POSED: eye / look_at / up are given
        ("samples", C.c_int32),       # per pixel, 1..RT_CAMERA_MAX_SAMPLES; 0: 4
        ("width", C.c_int32),         # both 0: the scene's; else both >= 2
        ("height", C.c_int32),
        ("depth", C.c_int32),         # 0: the scene's
        ("chunk_pixels", C.c_int32),  # 0: automatic; > 0: at most this many pixels per launch
        ("reserved", C.c_int32),
        ("fov", C.c_double),          # degrees; <= 0: the scene's
        ("extent", C.c_double),       # ortho: world width of the view
        ("aperture", C.c_double),     # thin lens: lens diameter
        ("focus", C.c_double),        # thin lens: focal-plane distance
        ("eye", C.c_double * 3),
        ("look_at", C.c_double * 3),
        ("up", C.c_double * 3),
    ]


class rt_adaptive(C.Structure):
    """An adaptive camera render's stopping rule (rt_render_camera_adaptive_async)."""
    _fields_ = [
        ("min_samples", C.c_int32),   # 0: min(4, samples); else 2 <= min_samples <= samples
        ("reserved", C.c_int32),      # must be 0
        ("tolerance", C.c_double),    # >= 0, not NaN; +inf: every pixel stops at min_samples
    ]


class rt_aov_out(C.Structure):
    """The feature buffers of rt_render_camera_aov_async: device pointers, any
    may be NULL, not all."""
    _fields_ = [
        ("depth", C.c_void_p),     # double, 1 per pixel
        ("normal", C.c_void_p),    # double, 3 per pixel
        ("albedo", C.c_void_p),    # double, 3 per pixel
        ("coverage", C.c_void_p),  # double, 1 per pixel
        ("ids", C.c_void_p),       # int32, 4 per pixel (AOV_IDS_DTYPE), 16-byte aligned
    ]


AOV_NAMES = ("depth", "normal", "albedo", "coverage", "ids")


class rt_denoise(C.Structure):
    """The a-trous filter's parameters (rt_denoise_atrous_async). A sigma > 0
    and finite turns its term on; 0 or +inf turns it off."""
    _fields_ = [
        ("iterations", C.c_int32),    # 1..8; 0: 5
        ("reserved", C.c_int32),      # must be 0
        ("sigma_color", C.c_double),
        ("sigma_normal", C.c_double),
        ("sigma_depth", C.c_double),
        ("sigma_albedo", C.c_double),
    ]


# the variance-guided filter (rt_denoise_atrous_var_async): added to kc2 * g under the reciprocal
RT_DENOISE_VAR_EPS = 1e-10

# numpy structured dtypes of the same layout as rt_ray / rt_hit / rt_radiance
RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("dir", "<f8", (3,)), ("tmax", "<f8"), ("exclude", "<i4"),
                      ("reserved", "<i4")])
HIT_DTYPE = np.dtype([("t", "<f8"), ("point_obj", "<f8", (3,)), ("point_world", "<f8", (3,)),
                      ("normal_world", "<f8", (3,)), ("object", "<i4"), ("face", "<i4"), ("kind", "<i4"),
                      ("material", "<i4")])
RADIANCE_DTYPE = np.dtype([("color", "<f8", (3,)), ("object", "<i4"), ("rays", "<i4")])
# one pixel of rt_aov_out.ids: sample 0's hit as rt_hit codes it (a miss: -1, 0, 0, 0)
AOV_IDS_DTYPE = np.dtype([("object", "<i4"), ("face", "<i4"), ("kind", "<i4"), ("material", "<i4")])


class PackedScene:
    """Owns the ctypes arrays an rt_scene points into (keeps them alive)."""

    def __init__(self, scene, lights, objects, materials, programs=None, ext_lights=None):
        self.scene = scene
        self._lights = lights
        self._ext_lights = ext_lights
        self._objects = objects
        self._materials = materials
        # (code, consts, entry ctypes arrays, [(SurfaceFn, EvalState stack)] per program)
        self.programs = programs

    @property
    def width(self):
        return int(self.scene.width)

    @property
    def height(self):
        return int(self.scene.height)

    def ref(self):
        return C.byref(self.scene)


# Algorithmic FP64 flops per Intersect call, by kind (SURVEY.md §8(d):
# +,-,*,/,sqrt = 1 each, compares 0; miss-path counts, i.e. a lower bound).
# sphere: 33 (ray->object) + 19 (a, halfB, c, discriminant) = 52
# plane : 33 + 5 (denom) + 7 (numerator) ... = 45 on the non-parallel path
# cube  : 6 planes = 270 (the reference re-transforms the ray per face)
# cylinder: 33 + ~51 = 84
# cone (extension): 33 + a, halfB, c (15) + discriminant (3) + base cap (~10) = 61
# csg (extension): counted as one test of the composite; lower bound = its
# bounding-sphere-culled leaf work is not modelled (0)
FLOPS_PER_TEST = (52, 45, 270, 84, 61, 0)
# Per shaded hit: surface props + ambient (21); per light: lighting (68).
FLOPS_PER_SHADE = 21
FLOPS_PER_LIGHT = 68


def algorithmic_flops(stats, num_lights):
    """Sum of count x flops over the work the render did (lower bound)."""
    f = 0
    for k in range(RT_NUM_KINDS):
        f += (int(stats.tests[k]) + int(stats.shadow_tests[k])) * FLOPS_PER_TEST[k]
    f += int(stats.shaded_hits) * (FLOPS_PER_SHADE + FLOPS_PER_LIGHT * num_lights)
    return f


def sum_stats(stats):
    """One rt_stats holding the field-wise sum of several (the counters of the
    contexts that rendered frames in flight); kernel_ms is the largest."""
    out = rt_stats()
    for st in stats:
        out.primary_rays += st.primary_rays
        out.secondary_rays += st.secondary_rays
        out.shadow_rays += st.shadow_rays
        for k in range(RT_NUM_KINDS):
            out.tests[k] += st.tests[k]
            out.shadow_tests[k] += st.shadow_tests[k]
        out.shaded_hits += st.shaded_hits
        out.surface_errors += st.surface_errors
        out.kernel_ms = max(out.kernel_ms, st.kernel_ms)
    return out
