/*
 * rt_abi.h -- C ABI of the MI355X-native renderer for the ICFP-2000 GML
 * raytracer (drop-in for the per-pixel Render() hot path of
 * timdestan/go-raytracer).
 *
 * What this replaces (reference file:line, relative to the reference repo):
 *   - raytracer.go:589-682   func Render(scene *Scene) image.Image
 *   - raytracer.go:724-830   ConvertRenderArgsToScene / convertGMLSceneObjects
 *                            (matrix inverse, normal matrices, plane D and
 *                            NormalWorld, cube face expansion) -- done inside
 *                            the library from the flattened object list below
 *   - raytracer.go:38-370    the SceneObject plug-in (Sphere/Plane/Cube/Cylinder
 *                            Intersect + ComputeSurfaceProps)
 *   - raytracer.go:372-562   computeLighting / inShadow / refract / fresnel /
 *                            closestHit / traceRay
 * The GML interpreter (internal/gml) stays on the host: it produces
 * gml.RenderArgs (evaluator.go:14-28); the host flattens RenderArgs.Scene in
 * the same BFS order as raytracer.go:776-828 and bakes each object's surface
 * into per-face constant materials (gml.Material, evaluator.go:136-150).
 *
 * Conventions: plain C, no exceptions cross this boundary; every entry point
 * returns RT_OK (0) or a negative RT_E* code, and rt_last_error() gives a
 * thread-local message. The output framebuffer has the exact layout of Go's
 * image.RGBA.Pix (row-major RGBA8, stride 4*width, alpha 255), so a cgo shim
 * can wrap it without copying.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#ifndef __HIPCC_RTC__ /* hipRTC (scene specialisation) provides size_t itself */
#include <stddef.h>
#endif
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 6
#define RT_MAX_DEVICES 16 /* devices one rt_render_ex call may use */
#define RT_EXP_AMD64_FMA 0
#define RT_EXP_AMD64 1
#define RT_EXP_PORTABLE 2

/* Status codes. */
#define RT_OK 0
#define RT_E_INVALID (-1)   /* bad argument / malformed scene             */
#define RT_E_SINGULAR (-2)  /* transform has det == 0 (prim/vec.go:343)   */
#define RT_E_DEVICE (-3)    /* HIP runtime error                          */
#define RT_E_NOMEM (-4)     /* device allocation failed                   */

/* Primitive kinds (the concrete SceneObject types, raytracer.go:43-277). */
#define RT_SPHERE 0
#define RT_PLANE 1
#define RT_CUBE 2
#define RT_CYLINDER 3
/* Contest extension (ICFP 2000 GML `cone`; not in the reference renderer, so
 * parity-unpinned): apex at the origin, x^2 + z^2 = y^2 for 0 <= y <= 1,
 * base disk at y = 1. Faces 0 side, 1 base. */
#define RT_CONE 4
/* Contest extension (GML `intersect` / `difference`; the reference renderer
 * rejects Difference, raytracer.go:825-826): one composite solid. Its leaves
 * are rt_scene.csg_leaves[csg_first .. csg_first + csg_count) (spheres, cubes,
 * cylinders, cones, planes as half-spaces n.p + D <= 0) combined by a postfix program
 * rt_scene.csg_code[csg_code .. csg_code + csg_code_len): v >= 0 pushes leaf v
 * (relative to csg_first), RT_CSG_UNION / _INTERSECT / _DIFFERENCE pop two.
 * The hit is the first interval end point t > 0 at which the composite's
 * membership changes (oracle/rt_oracle.c csg_intersect). */
#define RT_CSG 5
#define RT_NUM_KINDS 6
#define RT_CSG_UNION (-1)
#define RT_CSG_INTERSECT (-2)
#define RT_CSG_DIFFERENCE (-3)
#define RT_CSG_MAX_LEAVES 128

#define RT_MAX_FACES 6 /* prim.NUM_CUBE_SIDES, internal/prim/plane.go:27 */

/* gml.Material (internal/gml/evaluator.go:136-150), field for field. */
typedef struct rt_material {
    double color[3];
    double reflectivity;
    double fuzziness;
    double transparency;
    double refractive_index;
    double kd;
    double ks;
    double specular_exponent;
} rt_material;

/* gml.PointLight (internal/gml/evaluator.go:289-292). */
typedef struct rt_point_light {
    double position[3];
    double color[3];
} rt_point_light;

/* Lights of the contest extensions (GML `light`, `spotlight`; not in the
 * reference renderer, parity-unpinned). Point lights here behave exactly like
 * rt_point_light. Directional: direction = the way the light travels; the
 * shading vector is normalize(-direction) and shadow rays are unbounded.
 * Spot: at position, aimed at `direction` (a point), cutoff half-angle in
 * degrees, intensity colour * Pow(cos(angle), exponent) inside the cone and 0
 * outside (shadow rays are traced either way, one per light). No distance
 * attenuation, matching the reference's point lights. */
#define RT_LIGHT_POINT 0
#define RT_LIGHT_DIRECTIONAL 1
#define RT_LIGHT_SPOT 2
typedef struct rt_light {
    int32_t kind;
    int32_t reserved;
    double position[3];
    double direction[3]; /* directional: direction; spot: the point aimed at */
    double color[3];
    double cutoff;       /* spot: degrees */
    double exponent;     /* spot */
} rt_light;

/* One flattened scene object (a leaf of gml.RenderArgs.Scene after the BFS
 * union flattening of raytracer.go:776-828).
 *   transform      gml.<Kind>.TransformMat, row-major prim.Mat4
 *                  (object -> world); ignored when has_transform == 0 (nil
 *                  TransformMat => identity, raytracer.go:757-762).
 *   material[f]    index into rt_scene.materials for face f (the value
 *                  EvalSurfaceFn returns for that face; constant surfaces use
 *                  the same index for every face). Faces: sphere/plane 0;
 *                  cylinder 0 side, 1 top, 2 bottom (raytracer.go:263-267);
 *                  cube 0..5 = prim.CubeSide (internal/prim/plane.go:14-25).
 *   plane_point,
 *   plane_normal   RT_PLANE only: gml.Plane.Plane (evaluator.go:813-821 builds
 *                  point (0,0,0), normal (0,1,0)). */
/* Closure surfaces (GML surface functions that depend on face/u/v) run on the
 * device as straight-line register programs compiled by the host
 * (go-raytracer_amd/gml/surface_compiler.py). A face whose material index is
 * negative uses program (-material[f] - 1): it receives face (i64), u, v (f64)
 * as computed by the reference's ComputeSurfaceProps (raytracer.go:124-150,
 * 196-205, 339-359) and yields the 10 gml.Material fields, exactly what
 * EvalSurfaceFn (evaluator.go:672-727) returns for that hit. */
/* Surface-program bytecode: the contract a host compiles a GML surface
 * closure to (go-raytracer_amd/gml/surface_compiler.py is one compiler; a Go
 * or C host may emit the same words; tests/c/abi_render.c hand-assembles one).
 * Instruction = 2 x uint32: w0 = op | dst << 8 | a << 16 | b << 24, w1 = c.
 * 64 registers of 64 bits per lane (f64 bits, wrapping i64, or bool 0/1).
 * Entry: r10 = face (i64), r11 = u (f64), r12 = v (f64), as the reference's
 * ComputeSurfaceProps passes them. RET: r0..r9 = the gml.Material fields in
 * rt_material order (colour r g b, reflectivity, fuzziness, transparency,
 * refractive index, kd, ks, n), i.e. what EvalSurfaceFn returns
 * (evaluator.go:672-727; for `color kd ks n` results Reflectivity = ks and
 * fuzziness / transparency / refractive index are 0). Go semantics: one
 * rounding per f64 op, no fusion. The library validates every program at
 * rt_set_scene (opcodes, register / constant / table ranges, a reachable
 * RET within 8192 steps). */
#define RT_VM_NOP 0
#define RT_VM_CONST 1  /* r[d] = consts[c] (64-bit pattern) */
#define RT_VM_MOV 2    /* r[d] = r[a] */
#define RT_VM_ADDF 3   /* r[d] = r[a] + r[b] (f64); SUBF, MULF, DIVF likewise */
#define RT_VM_SUBF 4
#define RT_VM_MULF 5
#define RT_VM_DIVF 6
#define RT_VM_NEGF 7   /* r[d] = -r[a] */
#define RT_VM_ADDI 8   /* wrapping i64 */
#define RT_VM_SUBI 9
#define RT_VM_MULI 10
#define RT_VM_DIVI 11  /* truncating; x / 0 yields 0 (guard with ERR); MinInt64 / -1 wraps */
#define RT_VM_MODI 12  /* truncating remainder; x % 0 and x % -1 yield 0 */
#define RT_VM_NEGI 13
#define RT_VM_LTF 14   /* bool r[a] < r[b] (f64) */
#define RT_VM_EQF 15
#define RT_VM_LTI 16   /* i64 */
#define RT_VM_EQI 17
#define RT_VM_SEL 18   /* r[d] = r[a] ? r[b] : r[c & 63] */
#define RT_VM_FLOOR 19 /* i64 of floor(x) (amd64 float64 -> int64 conversion) */
#define RT_VM_FRAC 20  /* x - float64(int64(x)) */
#define RT_VM_SQRT 21
#define RT_VM_SIN 22   /* Go math.Sin(0.017453292519943295 * x), one product (evaluator.go:932 DegToRad): GML angles are degrees */
#define RT_VM_COS 23   /* Go math.Cos(0.017453292519943295 * x) */
#define RT_VM_CLAMPF 24 /* f64 clamped to [0, 1] */
#define RT_VM_CLAMPI 25 /* i64 clamped to [0, 1] */
#define RT_VM_TBL 26   /* r[d] = consts[c + 1 + clamp(r[a], 0, n - 1)], n = consts[c] (guard with ERR) */
#define RT_VM_AND 27   /* bool */
#define RT_VM_OR 28
#define RT_VM_NOT 29
#define RT_VM_ERR 30   /* the evaluation fails (counted in surface_errors) if r[a] != 0 */
#define RT_VM_RET 31
/* Contest extensions (GML `asin`, `acos`, `real`; not in the reference's
 * interpreter, oracle-pinned through the host interpreter). Angles come out
 * in degrees: one product with 57.29577951308232 (180 / Pi rounded once),
 * mirroring how SIN / COS apply Pi / 180. NaN for |x| > 1, as Go's math.Asin. */
#define RT_VM_EXT_ASIN 32 /* r[d] = 57.29577951308232 * Go math.Asin(r[a]) */
#define RT_VM_EXT_ACOS 33 /* r[d] = 57.29577951308232 * Go math.Acos(r[a]) */
#define RT_VM_EXT_REAL 34 /* r[d] = float64(int64 r[a]) (round to nearest even) */
#define RT_VM_INSN(op, d, a, b) ((uint32_t)(op) | ((uint32_t)(d) << 8) | ((uint32_t)(a) << 16) | ((uint32_t)(b) << 24))

typedef struct rt_object {
    int32_t kind;
    int32_t has_transform;
    int32_t material[RT_MAX_FACES];
    double transform[16];
    double plane_point[3];
    double plane_normal[3];
    /* RT_CSG only (see RT_CSG) */
    int32_t csg_first, csg_count, csg_code, csg_code_len;
} rt_object;

/* gml.RenderArgs (internal/gml/evaluator.go:14-28) with the scene already
 * flattened. depth <= 0 => 3 and fov <= 0 => 90 are applied by the library
 * exactly as raytracer.go:592-600 does. */
typedef struct rt_scene {
    int32_t width;
    int32_t height;
    int32_t depth;
    int32_t num_lights;
    double fov;          /* degrees */
    double ambient[3];
    double bg_start[3];  /* BgColorStart (zero when plain `render`) */
    double bg_end[3];    /* BgColorEnd */
    const rt_point_light *lights;
    const rt_object *objects;
    const rt_material *materials;
    int32_t num_objects;
    int32_t num_materials;
    /* surface programs (may be empty): instruction words of all programs,
     * each 2 x uint32 (w0 = op | dst<<8 | a<<16 | b<<24, w1 = c); entry word
     * offset per program; one shared constant pool of 64-bit patterns. */
    const uint32_t *program_code;
    const uint64_t *program_consts;
    const int32_t *program_entry;
    int32_t num_programs;
    int32_t program_code_words;
    int32_t program_const_count;
    /* ABI 3: which math.Exp / math.Log a fractional math.Pow exponent
     * (raytracer.go:395 specular n, spot exponents) runs -- Go dispatches them
     * per platform: RT_EXP_AMD64_FMA (0, default) exp_amd64.s with FMA, what
     * the reference runs on an x86-64 CPU with AVX2+FMA; RT_EXP_AMD64 (1) the
     * same without FMA; RT_EXP_PORTABLE (2) exp.go / log.go (platforms with
     * no assembly Exp). Integer exponents never reach Exp. */
    int32_t exp_mode;
    /* ABI 2: when num_ext_lights > 0 these are the scene's lights, in program
     * order, and lights / num_lights are ignored. */
    const rt_light *ext_lights;
    int32_t num_ext_lights;
    int32_t reserved1;
    /* ABI 2: CSG composites (RT_CSG objects) */
    const rt_object *csg_leaves;
    const int32_t *csg_code;
    int32_t num_csg_leaves;
    int32_t csg_code_words;
} rt_scene;

/* Work counters, identical in the CPU oracle and the GPU path.
 *   primary_rays     top-level traceRay calls (4 per pixel, raytracer.go:639)
 *   secondary_rays   recursive traceRay calls entered with depth > 0
 *                    (raytracer.go:528,554; depth 0 returns at :488-491)
 *   shadow_rays      inShadow calls: one per (shaded hit, light)
 *                    (raytracer.go:383)
 *   tests[k]         Intersect calls on kind k made by closestHit
 *   shadow_tests[k]  Intersect calls on kind k made by inShadow (early exit)
 *   shaded_hits      ComputeSurfaceProps + computeLighting evaluations
 *   surface_errors   closure-surface evaluations that raised an error */
typedef struct rt_stats {
    uint64_t primary_rays;
    uint64_t secondary_rays;
    uint64_t shadow_rays;
    uint64_t tests[RT_NUM_KINDS];
    uint64_t shadow_tests[RT_NUM_KINDS];
    uint64_t shaded_hits;
    uint64_t surface_errors; /* hits whose surface evaluation failed; the
                              * reference panics on the first one
                              * (raytracer.go:499-501) */
    double kernel_ms;    /* device time of the last render (GPU path; with
                          * several devices the slowest device's span)    */
    /* ABI 6: the devices of the last frame (rt_render / rt_render_ex; 1 for
     * rt_read_stats) and, per device in rt_render_opts order, the GPU span of
     * its share of the frame; gather_ms = host wall time from the moment every
     * device's share had rendered to the frame complete in the caller's
     * buffer (the gather and copy work the renders did not hide). */
    int32_t devices;
    int32_t reserved2;
    double device_kernel_ms[RT_MAX_DEVICES];
    double gather_ms;
} rt_stats;

/* Opaque per-device context: owns the converted scene on the device, the
 * work-queue counters and the stats buffer. Re-usable across renders (the
 * reference REPL renders many times per process, cmd/gml/main.go:104-115). */
typedef struct rt_context rt_context;

/* ABI version of the loaded library (RT_ABI_VERSION). */
int rt_abi_version(void);

/* Thread-local description of the last failure on this thread. */
const char *rt_last_error(void);

/* Create a context on HIP device `device` (the caller's current device when
 * device < 0). */
int rt_create(int device, rt_context **out);
void rt_destroy(rt_context *ctx);

/* Convert the flattened scene exactly as ConvertRenderArgsToScene
 * (raytracer.go:724-830) and upload it to the context's device. The scene is
 * read only during the call. Replaces any previous scene. */
int rt_set_scene(rt_context *ctx, const rt_scene *scene);

/* Enqueue the render of image rows [y0, y1) on `stream` (a hipStream_t; NULL
 * = the null stream) into device memory `d_rgba` (row y0 first, stride
 * 4*width bytes). Asynchronous; device pointers only. The per-row pixels are
 * identical to rows y0..y1-1 of a full-frame Render(): RNG state depends only
 * on (x, 20-row strip) (raytracer.go:627-634). Launches on one context run in
 * submission order: a launch on another stream than the previous launch
 * waits for that launch to end. */
int rt_render_rows_async(rt_context *ctx, int y0, int y1, void *d_rgba,
                         void *stream);

/* Interleaved variant for load-balanced multi-GPU sharding: render `ntrows`
 * 8-row tile rows, output tile row j being image rows
 * [(trow0 + j*trow_stride)*8, +8) clipped to the image, into d_rgba packed
 * contiguously (output row j*8 + r, stride 4*width; rows past the image are
 * left untouched). Same pixels as a full-frame render. */
int rt_render_tile_rows_async(rt_context *ctx, int trow0, int trow_stride, int ntrows,
                              void *d_rgba, void *stream);

/* Read (and optionally reset) the work counters accumulated on the device
 * since the last reset. Synchronises the given stream. If the render
 * watchdog stopped a wave (a kernel bug: a frame left unfinished) it returns
 * RT_E_DEVICE and resets the counters whatever `reset` says. */
int rt_read_stats(rt_context *ctx, void *stream, int reset, rt_stats *out);

/* Device time (ms) of the most recent rt_render_rows_async on this context,
 * measured with HIP events on the stream it was launched on. Synchronises. */
int rt_last_kernel_ms(rt_context *ctx, double *ms_out);

/* Scene specialisation (MI355X-specific, no reference counterpart). With
 * enable != 0 the context compiles, through hipRTC, a variant of the render
 * kernel with the current and every later scene's object count and primitive
 * kinds as compile-time constants, when the scene is small and linear (at most
 * 8 objects, no BVH, no CSG, scene resident in LDS); other scenes keep the
 * generic kernel. Output is bit-identical either way; the one-off compile
 * (seconds, cached per process) pays off for scenes rendered many times.
 * Returns RT_E_DEVICE with the compiler log if hipRTC is unavailable or fails.
 * Takes effect immediately for the current scene and in every rt_set_scene. */
int rt_set_specialize(rt_context *ctx, int enable);

/* Acceleration of the exact search (MI355X-specific; pixels and counters are
 * identical either way): RT_ACCEL_BVH builds a BVH over the bounded objects of
 * scenes with >= 12 of them (takes effect at the next rt_set_scene);
 * RT_ACCEL_CULL lets the kernel skip Intersect calls an FP32 bound proves to
 * miss (specialised kernels only; the generic kernel always culls). Default:
 * both. 0 runs the reference's brute-force search -- every ray tests every
 * object in FP64 -- e.g. to measure the FP64 roofline of the Intersect loop. */
#define RT_ACCEL_BVH 1
#define RT_ACCEL_CULL 2
int rt_set_accel(rt_context *ctx, int flags);

/* How pixels are dealt to the device lanes (MI355X-specific; pixels and
 * counters are identical in every mode). RT_SCHED_PIXEL: a lane renders a
 * pixel's 4 samples one after another (raytracer.go:645-651), 64 pixels per
 * dequeue. RT_SCHED_QUADS: a pixel's 4 samples run at once in 4 adjacent
 * lanes whose first lane adds them in sample order, 16 pixels per dequeue --
 * 4x shorter per-pixel latency, so deep branching glass trees do not leave a
 * few waves running long after the rest. RT_SCHED_AUTO (default): quads for
 * depth >= 7, and for launches that give each lane few pixels (a
 * strong-scaling share of a frame). Takes effect at the next launch (the
 * specialised kernel of the other schedule is compiled on first use). */
#define RT_SCHED_AUTO 0
#define RT_SCHED_PIXEL 1
#define RT_SCHED_QUADS 2
/* RT_SCHED_PAIRS: a pixel's samples 0-1 in one lane and 2-3 in the next, the
 * first lane adding all four in sample order -- half the quads' per-pixel
 * parallelism at half their idle-lane cost (specialised kernels,
 * rt_set_specialize; the generic kernels run quads for it). */
#define RT_SCHED_PAIRS 3
int rt_set_schedule(rt_context *ctx, int mode);

/* Frames in flight (MI355X-specific; pixels and counters are identical): a
 * host rendering a stream of frames keeps n >= 2 contexts with the same scene
 * and alternates its launches over them, one stream each, so one frame's
 * last waves share the chip with the next frame's first.
 * Telling each context n lets RT_SCHED_AUTO trade per-pixel latency for
 * fewer idle lanes where the overlap hides the longer tail (scenes in LDS
 * without CSG): serial samples instead of quads for launches of >= 32 pixels
 * per lane at depth >= 7, and with the specialised kernel pixel pairs for
 * branching scenes at 8-16 pixels per lane (depth < 7) or >= 16 (depth >= 7). Default 1. Takes effect at once. No reference
 * counterpart (Render is one synchronous frame, raytracer.go:589). */
int rt_set_frames_in_flight(rt_context *ctx, int n);

/* Tile order (MI355X-specific; pixels and counters are identical either
 * way). With enable != 0 (default) rt_set_scene also traces sample 0 of four
 * pixels per 8x8 tile of the frame at full depth and counts its rays (none of
 * them reach rt_read_stats); every launch then deals the costliest quarter of
 * its tiles first, in cost order, and the rest in tile order, so the deep
 * glass trees start early instead of keeping a few waves running after the
 * rest, while most tiles keep their neighbours' locality. Scenes staged in
 * LDS only: a scene read from HBM (a large BVH) loses more cache locality
 * than it gains. Applies to the current scene at once; rt_tile_order_info
 * reports whether an order is active and the estimate's wall time. */
int rt_set_tile_order(rt_context *ctx, int enable);
/* Work sharing at the tail of a launch (MI355X-specific; pixels and counters
 * are identical either way; default RT_SHARE_AUTO, below). With enable =
 * RT_SHARE_GROUP the context's
 * specialised kernel (rt_set_specialize) is compiled with a per-workgroup
 * board in LDS: once the work queue is drained, a lane still tracing a pixel
 * posts the samples it has not started and the pending refraction children
 * of its binary (reflect + refract, raytracer.go:512-556) frames, idle lanes
 * of any wave of the group trace them, and the owner joins their colours in
 * the reference's order. RT_SHARE_AUTO (the default, below) never picks this
 * workgroup board: its code costs every round of the kernel more than the
 * tail gains on the BASELINE configs. Applies to the current
 * scene at once. */
#define RT_SHARE_OFF 0
#define RT_SHARE_GROUP 1
/* RT_SHARE_DEVICE (ABI 5): the board is device-wide, in uncached HBM -- an
 * idle lane of any drained wave on the device (any workgroup, any XCD) takes
 * a posted refraction subtree; a few drained waves stay to help until no wave
 * of the launch is busy. Subtrees only (no sample posting).
 * RT_SHARE_AUTO (ABI 5, the default): RT_SHARE_DEVICE for scenes with CSG
 * composites at depth >= 7 on launches of fewer than 16 pixels per lane (a
 * strong-scaling share) or without frames in flight, else off. */
#define RT_SHARE_DEVICE 2
#define RT_SHARE_AUTO 3
int rt_set_work_sharing(rt_context *ctx, int enable);
/* Whether the current scene has a tile order, and the estimate's wall time
 * (ms) at scene setup. */
int rt_tile_order_info(rt_context *ctx, int *active, double *estimate_ms);

/* How the current scene is laid out for the device (bit flags), e.g. for
 * tests that must exercise one kernel flavour: RT_INFO_LDS the scene blob is
 * staged in LDS per workgroup; RT_INFO_BVH a BVH over the bounded objects;
 * RT_INFO_CSG CSG composites; RT_INFO_STREAM a large linear scene whose
 * object records are read from global memory in index order (per-wave LDS
 * chunks, or scalar loads in the brute-force kernel); RT_INFO_WAVEFRONT the
 * scene's kernel shares work across the lanes and waves of a workgroup at
 * the tail of a launch (rt_set_work_sharing); RT_INFO_ORDERED launches deal
 * tiles most expensive first (rt_set_tile_order). */
#define RT_INFO_LDS 1
#define RT_INFO_BVH 2
#define RT_INFO_CSG 4
#define RT_INFO_STREAM 8
#define RT_INFO_WAVEFRONT 16
#define RT_INFO_ORDERED 32
#define RT_INFO_SHARE_DEVICE 64 /* the work-sharing board is device-wide (RT_SHARE_DEVICE) */
int rt_scene_info(rt_context *ctx, int *flags);

/* Whether the current scene runs a specialised kernel, and the compile time
 * (ms) that preparing it cost (0 on a cache hit). Either pointer may be NULL. */
int rt_specialized(rt_context *ctx, int *active, double *compile_ms);

/* Compile (no device needed) and cache, for this process, the specialised
 * kernel for a scene of nobj (1..8) objects of the given kinds in object
 * order and the given RT_SPEC_* feature bits, e.g. to move the compile out of
 * a latency-critical rt_set_scene. */
#define RT_SPEC_SURFACES 1    /* the scene has closure (surface program) materials */
#define RT_SPEC_DIRECTIONAL 2 /* ... directional lights */
#define RT_SPEC_SPOT 4        /* ... spot lights */
#define RT_SPEC_LIGHTS(n) ((n) << 8) /* ... exactly n (1..8) lights, as every scene with 1..8
                                        lights is specialised (0: the generic light loop) */
int rt_spec_precompile(int nobj, const int *kinds, int features, double *compile_ms);

/* Diagnostic (tests, no device): compile the specialised variant named by
 * the library's internal key "lds:bvh:csg:nobj:kinds:kmask:feat:nlights:
 * pow_bits:nocull:schedule:share:far" (schedule 0 serial, 1 quads, 2 pairs;
 * share an RT_SHARE_* mode) exactly as a launch would ask for it. Every
 * compile runs in the helper process csrc/rt_spec_cc (RT_SPEC_INPROC=1: in
 * this process), so a compiler abort is a failed compile, not a dead caller. */
int rt_debug_spec_compile(const char *key, double *compile_ms);

/* Diagnostic (tests, no device): the value of environment variable `name` as
 * the library sees it -- its copy of the process environment taken when the
 * library was loaded (every RT_* knob, the compile helper's environment and
 * the in-process compiler's come from it; changes made after loading are not
 * seen) -- or NULL. The string lives as long as the process. */
const char *rt_debug_getenv(const char *name);

/* Diagnostic (tests): run surface program `program` of the context's scene on
 * n (face, u, v) inputs on the device; out10 receives n x 10 Material fields
 * (rt_material order), err n flags (1 = the reference would raise). */
int rt_debug_run_surface(rt_context *ctx, int program, int n, const long long *face,
                         const double *u, const double *v, double *out10, int *err);

/* ---- Batched ray queries against the scene last given to rt_set_scene ----
 * A separate kernel (csrc/rt_query.hip), one ray per lane, running the same
 * exact Intersect code as the renderer. Both records live in device memory,
 * in arrays aligned to 16 bytes. */
typedef struct rt_ray {        /* 64 bytes */
    double  origin[3];
    double  dir[3];            /* used as given, never normalised: t is in units of |dir| */
    double  tmax;              /* only an Intersect result with T < tmax counts; +inf: no limit */
    int32_t exclude;           /* top-level object index left out (raytracer.go:416), -1: none */
    int32_t reserved;          /* 0 */
} rt_ray;

typedef struct rt_hit {        /* 96 bytes */
    double  t;
    double  point_obj[3];      /* Hit.PointObj: object space of the surface (of the leaf, for a composite) */
    double  point_world[3];    /* HitEx.PointWorld */
    double  normal_world[3];   /* HitEx.NormalWorld, as the reference leaves it (a sphere's is not unit length) */
    int32_t object;            /* top-level index, -1: miss */
    int32_t face;              /* the oracle's code; composites: (leaf << 4) | (flip << 3) | leaf_face */
    int32_t kind;              /* RT_SPHERE.. of the surface (the leaf's kind for a composite) */
    int32_t material;          /* the face's objmat entry: >= 0 material index, < 0 closure program -(p+1) */
} rt_hit;

/* Closest mode: closestHit (raytracer.go:469-483) over the top-level objects
 * in index order for each of the n rays. Each object's own Intersect decides
 * whether there is a hit (its own t > 0 rules); `exclude` is skipped; a result
 * counts when T < tmax; the smallest T wins and exact ties go to the lowest
 * index. A miss writes object = -1 and zero in every other field, so records
 * compare as bytes. The answer does not depend on rt_set_accel.
 * RT_E_INVALID (with an rt_last_error text): NULL context, no scene set,
 * n < 0, or n > 0 with a NULL or not 16-byte aligned d_rays / d_hits. n == 0
 * returns RT_OK and launches nothing. The launch is ordered on `stream`; it
 * touches neither the frame counters (rt_read_stats) nor the tile order, the
 * specialisation state or pending compiles. As for renders, the scene must
 * not be replaced while a query is in flight. */
int rt_query_closest_async(rt_context *ctx, int n, const rt_ray *d_rays, rt_hit *d_hits, void *stream);

/* Occluded mode: d_occluded[i] = 1 when any object other than `exclude` has an
 * Intersect result with T < tmax for ray i, else 0 -- inShadow's loop
 * (raytracer.go:411-429) with the caller supplying the bound. Errors, ordering
 * and side effects as rt_query_closest_async (d_occluded needs no alignment). */
int rt_query_occluded_async(rt_context *ctx, int n, const rt_ray *d_rays, uint8_t *d_occluded, void *stream);

/* ---- Radiance queries: traceRay for arbitrary rays, and the camera's rays ----
 * A separate kernel (csrc/rt_trace.hip) with the renderer's exact tests and
 * shading, so a query returns the colour Render() sums for that ray, bit for
 * bit. */
typedef struct rt_radiance {   /* 32 bytes, arrays 16-byte aligned */
    double  color[3];          /* what traceRay returns for the ray (clamped per level as the reference does) */
    int32_t object;            /* top-level object the ray itself hit, -1: background */
    int32_t rays;              /* rays traced for this query: 1 + all secondary rays actually traced */
} rt_radiance;

#define RT_RADIANCE_MAX_DEPTH 32

/* d_out[i] = traceRay(d_rays[i], depth) (raytracer.go:487-562) against the
 * scene last set: lighting, shadows, the fuzz offset, reflection, refraction,
 * Fresnel, closure surfaces and CSG. depth == 0 means the scene's depth (3
 * when the scene gave depth <= 0). The direction is used as given, never
 * normalised (V = -dir, inShadow's t * |dir| < dist and fresnel's cosine
 * similarity then see the non-unit direction, as in the reference). tmax and
 * exclude apply to the ray's own closestHit only, with their meaning in
 * rt_query_closest_async; secondary and shadow rays follow the reference.
 * `rays` counts a ray when traceRay is entered with depth > 0, so depth 1
 * always answers rays == 1. The answer does not depend on rt_set_accel.
 * RT_E_INVALID (with an rt_last_error text): NULL context, no scene set,
 * n < 0, depth < 0 or > RT_RADIANCE_MAX_DEPTH (also a scene depth above it
 * with depth == 0), or n > 0 with a NULL or not 16-byte aligned d_rays /
 * d_out. n == 0 returns RT_OK and launches nothing. The launch is ordered on
 * `stream` and touches neither the frame counters (rt_read_stats) nor the tile
 * order, the specialisation state or pending compiles.
 * Unlike the other queries the call uses a per-context workspace: the frame
 * stacks of a persistent grid of rt_query_radiance_lanes() lanes (depth - 1
 * frames of 120 bytes per lane, at most 128 MiB per context: deeper calls run
 * on fewer lanes), allocated at the first call, grown when a call needs more
 * (which waits for the device) and freed by rt_destroy. Radiance queries on
 * one context must therefore be ordered with respect to each other -- one
 * stream, or events between streams -- as renders on a context already are. */
int rt_query_radiance_async(rt_context *ctx, int n, const rt_ray *d_rays, int depth,
                            rt_radiance *d_out, void *stream);

/* Lanes of the persistent grid a radiance query at `depth` (0: the scene's)
 * runs on at most -- 512 per compute unit, fewer where the workspace bound
 * says so; a batch of n rays uses min(that, n rounded up to 256). A batch
 * larger than this makes lanes take several rays. Negative: RT_E_INVALID. */
int rt_query_radiance_lanes(rt_context *ctx, int depth);

/* The reference camera's rays (raytracer.go:605-652) for rows [y0, y1) of the
 * scene's frame: 4 * width * (y1 - y0) records in [row][x][sample] order with
 * tmax = +inf, exclude = -1, reserved = 0 -- the exact jitter draws of
 * Render() (PCG seeded per column and 20-row strip, 8 draws per row, the
 * draws of a strip's rows before y0 consumed), so averaging their radiance at
 * the scene's depth and quantising reproduces Render()'s pixels.
 * RT_E_INVALID: NULL context, no scene set, rows outside 0 <= y0 < y1 <=
 * height, NULL or not 16-byte aligned d_rays. Ordered on `stream`; no side
 * effects on the context. */
int rt_query_camera_rays_async(rt_context *ctx, int y0, int y1, rt_ray *d_rays, void *stream);

/* ---- Camera renders: any sample count and camera model, fused on the device ----
 * The radiance kernel forms the camera's rays itself (no ray array), writes
 * one rt_radiance record per sample into a bounded context-owned buffer, and a
 * resolve kernel averages and quantises them (csrc/rt_camera.hip). All zero =
 * the scene's own camera at 4 samples: Render()'s pixels, byte for byte.
 *
 * Everything is FP64, one rounding per operation, in the order written here.
 * Draws: pixel (x, y) uses Render()'s stream PCG(0xDEAD ^ x, 0xBEEF ^ ymin),
 * ymin = 20 * (y / 20) (raytracer.go:627-634). With S samples and D draws per
 * sample (4 for the thin lens, else 2) a row consumes S * D draws; sample s of
 * row y reads draws (y - ymin) * S * D + s * D + 0 .. D-1 -- what the
 * reference would draw if numSamples were S.
 * Screen: dx = draw0 - 0.5, dy = draw1 - 0.5, su = (x + dx) / (W - 1),
 * sv = (y + dy) / (H - 1); with vw the view width and
 * vh = vw * (float(H) / float(W)): u = su * vw - vw / 2, v = sv * vh - vh / 2
 * (raytracer.go:603, 644-647).
 * Camera space is the reference's: eye e = (0, 0, -1), screen plane z = 0,
 * x right, y up, looking along +z.
 *   RT_CAMERA_PINHOLE   vw = 2 / Tan(fov * Pi / 180 / 2) (raytracer.go:601-602;
 *                       fov <= 0: the scene's vw); o = (u, -v, 0),
 *                       d = normalize(o - e)
 *   RT_CAMERA_ORTHO     vw = extent; o = (u, -v, 0), d = (0, 0, 1)
 *   RT_CAMERA_EQUIRECT  theta = (su - 0.5) * 360, phi = (0.5 - sv) * 180;
 *                       o = e, d = (Sin theta * Cos phi, Sin phi,
 *                       Cos theta * Cos phi), Sin / Cos being Go's math.Sin /
 *                       math.Cos of 0.017453292519943295 * angle (RT_VM_SIN)
 *   RT_CAMERA_THINLENS  the pinhole's o and d; P = e + d * (focus / d.z);
 *                       rho = (aperture / 2) * sqrt(draw2), alpha = 360 * draw3;
 *                       L = e + (rho * Cos alpha, rho * Sin alpha, 0); the ray
 *                       is (L, normalize(P - L))
 * Pose (RT_CAMERA_POSED; without it camera space is world space):
 * f = normalize(look_at - eye), r = normalize(cross(up, f)), w = cross(f, r);
 * a camera-space point p maps to eye + p.x * r + p.y * w + (p.z + 1) * f, a
 * direction to d.x * r + d.y * w + d.z * f (not renormalised), terms added
 * left to right.
 * Pixel: mean = ((c0 + c1) + c2 + ...) * (1.0 / S) in sample order, each byte
 * uint8(uint32(mean * 65535) >> 8) as Go converts on amd64 (vec.go:104-107). */
#define RT_CAMERA_PINHOLE  0   /* the reference's camera model (raytracer.go:601-652) */
#define RT_CAMERA_ORTHO    1
#define RT_CAMERA_EQUIRECT 2   /* 360 x 180 degree panorama */
#define RT_CAMERA_THINLENS 3   /* pinhole with a finite aperture: depth of field */
#define RT_CAMERA_POSED    1   /* flags: eye / look_at / up are given */
#define RT_CAMERA_MAX_SAMPLES 1024

typedef struct rt_camera {      /* all zero = the scene's own camera, 4 samples: Render() */
    int32_t model, flags;
    int32_t samples;            /* per pixel, 1..RT_CAMERA_MAX_SAMPLES; 0: 4 */
    int32_t width, height;      /* both 0: the scene's; else both >= 2 */
    int32_t depth;              /* 0: the scene's; else 1..RT_RADIANCE_MAX_DEPTH */
    int32_t chunk_pixels;       /* 0: automatic (below); > 0: at most this many pixels per launch */
    int32_t reserved;
    double  fov;                /* degrees; <= 0: the scene's (pinhole, thin lens) */
    double  extent;             /* ortho: world width of the view, > 0 */
    double  aperture, focus;    /* thin lens: lens diameter >= 0, focal-plane distance > 0 */
    double  eye[3], look_at[3], up[3];   /* RT_CAMERA_POSED only */
} rt_camera;

/* The camera's rays for rows [y0, y1) of its frame (W x H: the camera's size,
 * else the scene's): samples * W * (y1 - y0) records in [row][x][sample]
 * order with tmax = +inf, exclude = -1, reserved = 0. cam == NULL means all
 * zeros, for which these are exactly the records of
 * rt_query_camera_rays_async. RT_E_INVALID (with an rt_last_error text): NULL
 * context, no scene set, unknown model or flag bits, samples / width / height
 * / depth / chunk_pixels out of range (a frame of more than 2^31 - 1 pixels
 * included), rows outside 0 <= y0 < y1 <= H, a fov whose Tan is not a positive
 * finite number, extent (ortho), focus or aperture (thin lens) out of range
 * or not finite, a posed camera with eye == look_at or up parallel to the view
 * direction (or not finite), NULL or not 16-byte aligned d_rays. Ordered on
 * `stream`; no side effects on the context. */
int rt_camera_rays_async(rt_context *ctx, const rt_camera *cam, int y0, int y1, rt_ray *d_rays, void *stream);

/* Render rows [y0, y1) of the camera's frame into either or both of d_rgba
 * (row y0 first, stride 4 * W, alpha 255) and d_mean (3 doubles per pixel,
 * 8-byte aligned: the mean before quantisation); not both NULL. Device
 * pointers only. Errors as rt_camera_rays_async, for the output pointers:
 * both NULL, d_mean not 8-byte aligned, d_rgba not 4-byte aligned (pixels are
 * stored as 32-bit words).
 * The band's pixels, in [row][x] order, are cut into chunks of
 * max(1, 2097152 / samples) consecutive pixels (chunk_pixels if that is
 * smaller; chunks need not align to rows). Per chunk the call enqueues on
 * `stream`: the ticket counter's reset, one launch of the radiance kernel in
 * which ticket t is sample t % samples of the chunk's pixel t / samples, and
 * one resolve launch (a thread per pixel). The host never waits between
 * chunks. The sample records live in a context-owned buffer of at most 64 MiB,
 * allocated at the first call, grown when a call needs more (which waits for
 * the device) and freed by rt_destroy.
 * The call touches neither the frame counters (rt_read_stats) nor the tile
 * order, the specialisation state or pending compiles, and the pixels do not
 * depend on rt_set_accel. It uses the radiance queries' workspace and ticket
 * and its own sample buffer: camera renders and radiance queries on one
 * context must be ordered with respect to each other -- one stream, or events
 * between streams. */
int rt_render_camera_async(rt_context *ctx, const rt_camera *cam, int y0, int y1,
                           void *d_rgba, double *d_mean, void *stream);

/* Chunks (radiance-kernel launches) rt_render_camera_async makes for these
 * arguments; negative: the RT_E_INVALID it would return (buffers aside). */
int rt_render_camera_chunks(rt_context *ctx, const rt_camera *cam, int y0, int y1);

/* Adaptive camera renders: per-pixel sample counts chosen on the device.
 * Everything is FP64, one rounding per operation, no contraction, in the order
 * written here.
 * Cap and draws: S = cam->samples (0: 4) is the cap and also the draw stride:
 * sample s of pixel (x, y) is exactly sample s of rt_render_camera_async with
 * the same camera -- same draws, same ray. A pixel that ends with n = S
 * samples is that render's pixel, bit for bit.
 * Schedule: n_0 = min_samples (0: min(4, S)), n_(k+1) = min(2 * n_k, S) until
 * n_K = S. Pass 0 traces samples [0, n_0) of every pixel, pass k samples
 * [n_(k-1), n_k) of every pixel still active: all active pixels of a pass hold
 * the same n.
 * State of a pixel: Sum_c and Q_c start as c_0 and c_0 * c_0; then for
 * s = 1, 2, ... in sample order Sum_c = Sum_c + c_s and
 * Q_c = Q_c + (c_s * c_s), per channel c. Sum is the fixed render's ordered sum.
 * Stopping rule after a pass that leaves n samples:
 *   inv = 1.0 / (double)n;  m_c = Sum_c * inv;  v_c = Q_c - Sum_c * m_c;
 *   e_c = v_c / (double)(n * (n - 1))   (the squared standard error of the mean)
 * the pixel is converged iff e_c <= tol2 for all three channels, with
 * tol2 = tolerance * tolerance formed once on the host (false for NaN; a
 * negative v_c passes).
 * A pixel becomes final when it is converged or n = S: its mean is m_c, its
 * bytes uint8(uint32(m_c * 65535) >> 8) with alpha 255 as above, its sample
 * count n. Other pixels stay active for the next pass. */
typedef struct rt_adaptive {
    int32_t min_samples;        /* 0: min(4, samples); else 2 <= min_samples <= samples */
    int32_t reserved;           /* must be 0 */
    double  tolerance;          /* >= 0, not NaN; +inf: every pixel stops at min_samples */
} rt_adaptive;

/* Render rows [y0, y1) of the camera's frame adaptively into any of d_rgba and
 * d_mean (laid out as for rt_render_camera_async) and d_samples (one int32 per
 * pixel, [row][x], 4-byte aligned: the pixel's sample count); not all three
 * NULL. Device pointers only. RT_E_INVALID (with an rt_last_error text) for
 * everything rt_render_camera_async rejects, and: NULL ad, reserved != 0, a
 * cap below 2 samples, min_samples outside [2, samples], a negative or NaN
 * tolerance, all outputs NULL, a misaligned output. Nothing is launched then
 * and the context stays usable.
 * Chunks: max(1, min(524288, 2097152 / B)) consecutive pixels, B the largest
 * batch n_k - n_(k-1) of the schedule (chunk_pixels if that is smaller). Per
 * chunk the call enqueues on `stream`: one reset of the chunk's pass counts
 * and tickets, then per pass one launch of the radiance kernel -- ticket t is
 * sample n_(k-1) + t % b of the pass's active pixel t / b, b = n_k - n_(k-1),
 * and the launch reads its number of active pixels from device memory -- and
 * one launch that continues the pixels' sums, applies the rule, writes the
 * final pixels and lists the others for the next pass. The host never waits
 * and never learns how many pixels are active. The order of a list may differ
 * from run to run; no output depends on it.
 * Memory, context-owned, grown when a call needs more (which waits for the
 * device), freed by rt_destroy: the camera renders' sample buffer (at most
 * 64 MiB) and at most 28 MiB of pixel state and lists.
 * Side effects and ordering: as rt_render_camera_async (none on renders,
 * counters, specialisation and tile order; to be ordered with the other
 * camera renders and the radiance queries of the context). */
int rt_render_camera_adaptive_async(rt_context *ctx, const rt_camera *cam, const rt_adaptive *ad, int y0, int y1,
                                    void *d_rgba, double *d_mean, int32_t *d_samples, void *stream);

/* The launches rt_render_camera_adaptive_async makes for these arguments:
 * *chunks chunks of *passes passes each (either may be NULL). RT_OK, or the
 * RT_E_INVALID the render would return (buffers aside). */
int rt_render_camera_adaptive_plan(rt_context *ctx, const rt_camera *cam, const rt_adaptive *ad, int y0, int y1,
                                   int *chunks, int *passes);

/* ---- Variance of a camera render: the squared standard error of each pixel's
 * mean, per channel ---- (csrc/rt_camera.hip). FP64, one rounding per
 * operation, no contraction, in the order written here; the state and the
 * expressions are those of "Adaptive camera renders" above, unchanged.
 * Sum_c and Q_c accumulate in sample order over the pixel's n samples (Sum_c
 * and Q_c start as c_0 and c_0 * c_0; then Sum_c = Sum_c + c_s and
 * Q_c = Q_c + (c_s * c_s)): n = S for the fixed render, and the count the
 * pixel ends with for the adaptive render. Then
 *   inv = 1.0 / (double)n;  m_c = Sum_c * inv;  v_c = Q_c - Sum_c * m_c;
 *   e_c = v_c / (double)(n * (n - 1));  var_c = e_c < 0.0 ? 0.0 : e_c
 * so a negative estimate becomes 0 and a NaN stays NaN. m_c is bit for bit the
 * mean the calls without a variance write.
 * d_var holds 3 doubles per pixel, 8-byte aligned, laid out like d_mean. With
 * d_var == NULL the two calls below are rt_render_camera_async and
 * rt_render_camera_adaptive_async: the same checks, chunks, launches (the
 * same kernels), memory, ordering and side effects. With a d_var the fixed
 * render's resolve launch is a sibling kernel that also keeps Q_c, and the
 * adaptive render's per-pass launch writes var_c where it writes m_c; d_rgba
 * and d_mean receive what those calls write. RT_E_INVALID in addition to those
 * calls' cases: all outputs NULL (d_var included), d_var not 8-byte aligned,
 * d_var given with samples == 1 (there is no estimate from one sample). */
int rt_render_camera_var_async(rt_context *ctx, const rt_camera *cam, int y0, int y1,
                               void *d_rgba, double *d_mean, double *d_var, void *stream);
int rt_render_camera_adaptive_var_async(rt_context *ctx, const rt_camera *cam, const rt_adaptive *ad, int y0, int y1,
                                        void *d_rgba, double *d_mean, int32_t *d_samples,
                                        double *d_var, void *stream);

/* ---- Feature buffers: per-pixel depth, normal, albedo, coverage and ids of a
 * camera render, and an edge-avoiding a-trous filter guided by them ----
 * (csrc/rt_aov.hip). Everything is FP64, one rounding per operation, no
 * contraction, in the order written here.
 *
 * Rows [y0, y1) of the camera's frame are written in [row][x] order, row y0
 * first. S = cam->samples (0: 4). Sample s of pixel (x, y) is exactly sample s
 * of rt_render_camera_async with the same camera -- same draws, same ray. For
 * each sample, closestHit runs as rt_query_closest_async defines it, with
 * tmax = +inf and exclude = -1. A sample that hits yields
 *   t   the hit's t;
 *   n^  nw / sqrt(nw.x * nw.x + nw.y * nw.y + nw.z * nw.z), component by
 *       component with IEEE division, nw being rt_hit.normal_world (the
 *       composite's flip included);
 *   a   the surface's material colour: materials[material].color for
 *       material >= 0; for a closure surface the colour of its program run on
 *       the (face, u, v) the radiance kernel forms, a failing evaluation giving
 *       (0, 0, 0) (the all-zero material). The colour is not clamped.
 * Accumulators zt, N, A (0.0) and the integer hit count h (0): the hitting
 * samples are added in sample order (zt = zt + t, N = N + n^, A = A + a per
 * component, h = h + 1); misses add nothing. With inv = 1.0 / (double)S:
 *   coverage = (double)h * inv,  normal = N * inv,  albedo = A * inv,
 *   depth = h > 0 ? zt / (double)h : +inf
 * so normal and albedo carry the coverage. ids is sample 0's object, face,
 * kind, material as rt_hit codes them; a miss gives -1, 0, 0, 0. */
typedef struct rt_aov_out {      /* device pointers; any may be NULL, not all */
    double  *depth;              /* 1 per pixel, 8-byte aligned */
    double  *normal;             /* 3 per pixel */
    double  *albedo;             /* 3 per pixel */
    double  *coverage;           /* 1 per pixel */
    int32_t *ids;                /* 4 per pixel, 16-byte aligned: object, face, kind, material */
} rt_aov_out;

/* One launch, one lane per pixel of the band, ordered on `stream`.
 * cam->depth and cam->chunk_pixels are validated as for camera renders and
 * otherwise unused. RT_E_INVALID (with an rt_last_error text) for everything
 * rt_render_camera_async rejects, and: NULL out, all five pointers NULL, a
 * misaligned pointer. Nothing is launched then and the context stays usable.
 * The call touches no counters, tile order, specialisation state or workspace
 * and allocates nothing: there is no sample buffer and there are no chunks, so
 * it needs no ordering with the other calls on the context. The answer does
 * not depend on rt_set_accel. */
int rt_render_camera_aov_async(rt_context *ctx, const rt_camera *cam, int y0, int y1,
                               const rt_aov_out *out, void *stream);

/* Edge-avoiding a-trous filter on a float64 mean. All buffers are whole frames
 * of width x height pixels in [row][x] order, laid out as
 * rt_render_camera_async (d_mean -> d_color) and rt_render_camera_aov_async
 * (normal, depth, albedo) write them; d_out and d_tmp hold 3 doubles per pixel.
 * Taps h = (1/16, 1/4, 3/8, 1/4, 1/16), so h[j] * h[i] is exact. K = iterations
 * (0: 5). For iteration i = 0 .. K-1: step = 1 << i; the input is I_i, with
 * I_0 = d_color; the output goes to d_out when K - 1 - i is even, else to
 * d_tmp, so I_K lands in d_out. Constants, formed once on the host:
 * ic_i = 1.0 / (s * s) with s = sigma_color * 0.5^i; in, iz, ia =
 * 1.0 / (sigma * sigma) of the normal, depth and albedo terms.
 *   kern(x) = x < 1.0 ? (1.0 - x) * (1.0 - x) : 0.0       (0 for NaN)
 *   dist2(a, b) = (d0 * d0 + d1 * d1) + d2 * d2, d the componentwise a - b
 * Pixel p = (x, y): sum = 0, wsum = 0; for dy = -2..2 (outer), dx = -2..2
 * (inner): q = (x + dx * step, y + dy * step), skipped when outside the frame;
 * w = h[dy + 2] * h[dx + 2]; then for each term that is on, in this order,
 *   colour  w = w * kern(dist2(I_i[p], I_i[q]) * ic_i)
 *   normal  w = w * kern(dist2(n[p], n[q]) * in)
 *   depth   w = w * kern((z[p] == z[q] ? 0.0 : (z[p] - z[q]) * (z[p] - z[q])) * iz)
 *           (two background pixels, both +inf, agree)
 *   albedo  w = w * kern(dist2(a[p], a[q]) * ia)
 * and the tap contributes only if w > 0.0: sum.c = sum.c + w * I_i[q].c per
 * channel, then wsum = wsum + w. The result is sum.c / wsum (IEEE division)
 * when wsum > 0.0, else I_i[p] unchanged. d_rgba (optional, 4-byte aligned)
 * receives I_K quantised as the camera renders quantise their mean. */
typedef struct rt_denoise {
    int32_t iterations;          /* 1..8; 0: 5 */
    int32_t reserved;            /* must be 0 */
    double  sigma_color, sigma_normal, sigma_depth, sigma_albedo;
                                 /* > 0 and finite: the term is on; 0 or +inf: off; negative or NaN: invalid */
} rt_denoise;

/* One launch per iteration on `stream` (a thread per pixel); the host does not
 * wait. No scene is needed, nothing is allocated and d_color is never written.
 * RT_E_INVALID (with an rt_last_error text): NULL context or dn, reserved != 0,
 * iterations outside [0, 8], a negative or NaN sigma, width or height < 1 (or
 * more than 2^31 - 1 pixels), NULL d_color or d_out, NULL d_tmp with more than
 * one iteration, a NULL guide whose term is on, a float64 buffer not 8-byte
 * aligned, overlapping byte ranges of d_color, d_out and d_tmp. Nothing is
 * launched then. */
int rt_denoise_atrous_async(rt_context *ctx, const rt_denoise *dn, int width, int height,
                            const double *d_color, const double *d_normal, const double *d_depth,
                            const double *d_albedo, double *d_out, double *d_tmp, void *d_rgba, void *stream);

/* ---- Variance-guided a-trous filter ---- (csrc/rt_aov.hip). The filter above
 * with its colour term scaled by the locally prefiltered standard deviation of
 * the pixel, and a scalar variance carried through the iterations (as SVGF
 * does). rt_denoise is reused unchanged; in this call sigma_color is in
 * standard deviations. FP64, one rounding per operation, in this order.
 * Taps, kern, dist2, the normal, depth and albedo terms, the d_out / d_tmp
 * ping-pong, the buffer sizes, K and the rule that turns a term on or off are
 * exactly those of rt_denoise_atrous_async. d_var (3 doubles per pixel, as
 * rt_render_camera_var_async writes it) is the variance of d_color.
 * The scalar variance S_i has one double per pixel and lives in d_var_out when
 * K - i is even, else in d_var_tmp (both are always needed); S_K ends in
 * d_var_out, the filtered frame's variance estimate. One reduce launch writes
 *   S_0[p] = (var[p].0 + var[p].1) + var[p].2
 * kc2 = sigma_color * sigma_color is formed on the host; sigma does not halve
 * per iteration.
 * Iteration i at pixel p = (x, y), with the colour term on: g = N / D with
 * N = 0, D = 0 and, for dy = -1..1 (outer), dx = -1..1 (inner) at unit spacing
 * whatever the step, q = (x + dx, y + dy) skipped when outside the frame,
 * k = (1/4, 1/2, 1/4):
 *   N = N + (k[dy + 1] * k[dx + 1]) * S_i[q];  D = D + k[dy + 1] * k[dx + 1]
 * then icv = 1.0 / (kc2 * g + RT_DENOISE_VAR_EPS), and the colour term of tap
 * q is  w = w * kern(dist2(I_i[p], I_i[q]) * icv); the guides follow in the
 * old order. A tap with w > 0.0 contributes to sum and wsum as before and also
 *   vs = vs + (w * w) * S_i[q]          (vs starts at 0)
 * I_(i+1)[p] is formed as before, and
 *   S_(i+1)[p] = wsum > 0.0 ? vs / (wsum * wsum) : S_i[p]
 * With the colour term off no g is formed and the variance still propagates.
 * A NaN g shuts every tap: the pixel and its variance pass through. g = +inf
 * opens the colour term fully (icv = 0). */
#define RT_DENOISE_VAR_EPS 1e-10

/* One reduce launch, then one launch per iteration on `stream`; the host never
 * waits, nothing is allocated, and d_color and d_var are never written.
 * RT_E_INVALID as for rt_denoise_atrous_async, and: NULL or not 8-byte aligned
 * d_var, d_var_out or d_var_tmp; any overlap among the byte ranges of d_color,
 * d_var, d_out, d_tmp (3 doubles per pixel each), d_var_out and d_var_tmp (1
 * double per pixel each). d_tmp may still be NULL when there is one
 * iteration. Nothing is launched then. */
int rt_denoise_atrous_var_async(rt_context *ctx, const rt_denoise *dn, int width, int height,
                                const double *d_color, const double *d_var,
                                const double *d_normal, const double *d_depth, const double *d_albedo,
                                double *d_out, double *d_tmp, double *d_var_out, double *d_var_tmp,
                                void *d_rgba, void *stream);

/* SSIM of two RGBA8 frames in device memory (width x height, stride 4W), the
 * reference's parity metric prim.SSIM (internal/prim/ssim.go:27-182; used by
 * raytracer_test.go:42 with threshold 0.99). Synchronous on `stream`.
 * RT_E_INVALID "images are too small" below 11x11; NaN at exactly 11 wide or
 * high (no window visited, as in the reference). */
int rt_ssim_rgba8(rt_context *ctx, const uint8_t *d_a, const uint8_t *d_b, int width, int height,
                  double *out_ssim, void *stream);

/* Synchronous whole-frame Render() into host memory (width*height*4 bytes,
 * caller-owned, e.g. Go's image.RGBA.Pix): the replacement of
 * func Render(*Scene) image.Image (raytracer.go:589-682), called from the
 * EvalState.Render hook (evaluator.go:48). Same as rt_render_ex(scene, NULL,
 * rgba_out, stats): the caller's current HIP device. */
int rt_render(const rt_scene *scene, uint8_t *rgba_out, rt_stats *stats);

/* ABI 6: Render() over one or several GPUs of this process.
 *
 * Devices (first match): device_mask != 0 -> the devices whose bit is set, in
 * ascending order; else device_count > 0 with RT_RENDER_DEVICE_LIST in flags
 * -> devices[0 .. device_count) (an ordinal may repeat: the same GPU then
 * renders several shares at once, each with its own contexts, which exercises
 * the multi-device path on one GPU); else device_count > 0 -> devices
 * 0 .. device_count-1; else the caller's current device. opts may be NULL.
 *
 * Partition: the frame's 8-row tile rows are dealt
 * round-robin, tile row t to device t mod N, so every device gets the same
 * mix of sky, floor and glass; pixels and counters are those of a one-device
 * frame (RNG state depends only on (x, 20-row strip), raytracer.go:627-634).
 * Each device renders its share into its own HBM, densely packed, as row
 * bands alternating over two contexts and streams.
 *
 * Gather (the `gather` field):
 *   RT_GATHER_HOST  each device DMAs each finished band of its share straight
 *                   to the band's final rows of a pinned frame, over its own
 *                   PCIe link, and the host copies finished bands on to
 *                   rgba_out while later bands render (N links in parallel);
 *   RT_GATHER_PEER  every share is copied to the first device over xGMI
 *                   (hipMemcpyPeerAsync, peer access enabled where the
 *                   devices allow it) and de-interleaved there into one
 *                   frame, which one DMA brings to the host -- or, with
 *                   RT_RENDER_OUT_DEVICE, which IS rgba_out;
 *   RT_GATHER_AUTO  (0) HOST for host output, PEER with RT_RENDER_OUT_DEVICE.
 * flags: RT_RENDER_OUT_DEVICE -- rgba_out is device memory of the first
 * device (H x 4W bytes); RT_RENDER_GENERIC -- the ahead-of-time kernel only
 * (no hipRTC); RT_RENDER_SPEC_SYNC -- a new scene shape waits for its
 * specialised kernel instead of rendering with the generic one meanwhile.
 * bands: row bands per device (0: one per ~2 M pixels of the share, <= 4;
 * RT_RENDER_BANDS in the environment overrides the automatic count). Bands
 * decrease in size (weights n, n-1, ..., 1; RT_RENDER_BAND_SHAPE=0: equal), so
 * the exposed copy after the last band is the smallest band's. Environment
 * knobs are read from the library's load-time copy of the environment.
 *
 * Kept per device between calls: two contexts with the last scene (an
 * unchanged scene -- byte-equal arrays -- is not converted, uploaded or
 * estimated again; a changed one is converted once and cloned to every
 * context), the share buffer, streams and events; one pinned frame. Scene
 * specialisation: a call never waits for hipRTC unless RT_RENDER_SPEC_SYNC --
 * a new shape renders with the generic kernel (same pixels and counters)
 * while its specialised kernel compiles on a background thread, and later
 * calls switch to it (rt_render_timing.specialized / .pending_compiles);
 * a failed compile is logged once and the generic kernel stays;
 * RT_RENDER_SPECIALIZE=0 in the environment keeps the generic kernel.
 * stats may be NULL: the counters summed over every device and context;
 * kernel_ms = the slowest device's GPU span; devices, device_kernel_ms[],
 * gather_ms as documented at rt_stats. Synchronous; calls are serialised. */
#define RT_GATHER_AUTO 0
#define RT_GATHER_HOST 1
#define RT_GATHER_PEER 2
#define RT_RENDER_DEVICE_LIST 1
#define RT_RENDER_OUT_DEVICE 2
#define RT_RENDER_GENERIC 4
#define RT_RENDER_SPEC_SYNC 8
typedef struct rt_render_opts {
    int32_t device_count;
    uint32_t device_mask;
    int32_t devices[RT_MAX_DEVICES];
    int32_t gather;     /* RT_GATHER_* */
    int32_t flags;      /* RT_RENDER_* */
    int32_t bands;      /* row bands per device, 0 = automatic */
    int32_t reserved[5];
} rt_render_opts;
int rt_render_ex(const rt_scene *scene, const rt_render_opts *opts, uint8_t *rgba_out, rt_stats *stats);

/* Diagnostic (tests, no device): the host side of the multi-device assembly
 * rt_render_ex runs, on host buffers. shares[d] holds device d's share as
 * rt_render_ex renders it (its tile rows d, d+N, ... of an N-device frame,
 * packed, stride 4*width, the last tile row clipped to the image); the frame
 * is assembled into out with exactly the copy plan -- bands, strided DMA
 * segments, row clipping -- the device path uses, for `bands` bands per
 * device (0 = automatic). */
int rt_debug_assemble(int width, int height, int ndev, int bands, const uint8_t *const *shares, uint8_t *out);

/* ABI 5: the parts of the calling thread's last rt_render call, on one host
 * timeline (setup + render_wait + copy_tail = total):
 *   setup_ms        scene compare (and, if it changed, conversion, upload,
 *                   specialisation, tile-cost estimate) and the launches
 *   render_wait_ms  until the frame's last band has rendered (the earlier
 *                   bands' host copies run inside it)
 *   copy_tail_ms    the last band's DMA and host copy, and the counters
 *   gpu_ms          GPU span of the frame (first band's start to last end)
 * bands: row bands the frame was rendered in (over all devices);
 * scene_reused: the scene was unchanged; specialized: every launch of the
 * call ran a specialised kernel. ABI 6: devices of the call; pending_compiles:
 * specialised kernels still compiling in the background when the call ended
 * (the call itself rendered with the generic kernel where they were missing). */
typedef struct rt_render_timing {
    double total_ms;
    double setup_ms;
    double render_wait_ms;
    double copy_tail_ms;
    double gpu_ms;
    int32_t bands;
    int32_t scene_reused;
    int32_t specialized;
    int32_t devices;
    int32_t pending_compiles;
    int32_t reserved;
} rt_render_timing;
int rt_render_last_timing(rt_render_timing *out);

#ifdef __cplusplus
}
#endif

#endif /* RT_ABI_H */
