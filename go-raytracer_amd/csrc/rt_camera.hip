// rt_camera.hip -- camera renders (include/rt_abi.h rt_camera,
// rt_camera_rays_async, rt_render_camera_async, rt_render_camera_chunks,
// rt_render_camera_adaptive_async, rt_render_camera_adaptive_plan, and the
// two renders with a variance output, rt_render_camera_var_async and
// rt_render_camera_adaptive_var_async).
//
// The radiance kernel of rt_trace.hip with a ray source of its own, plus a
// resolve step. rt_trace_kernel<.., GEN = true> hands out tickets exactly as a
// radiance query does, but ticket t is sample t % S of pixel first + t / S of
// the camera's frame, and the lane that takes it forms the ray itself
// (cam_ticket_ray -> cam_ray) instead of loading Q.rays[t]. Everything after
// the refill is the query's code, and the record still goes to Q.out[t]: here
// the context's sample buffer. cam_resolve_kernel, one thread per pixel, then
// adds the pixel's S records in sample order, scales and quantises.
//
// Sample-granular tickets and a separate resolve, not a per-lane accumulator
// over a pixel's samples: nothing new stays live across the kernel's loop
// (pixel, sample, draws and the camera-space ray die inside the refill; the
// camera is a kernel argument, read through scalar loads where it is needed),
// and the kernel's CSG and VM instantiations have no registers to spare.
//
// Bounded memory: a band is cut into chunks of consecutive pixels whose
// samples fit the buffer (CAM_BUF_RECORDS records, 64 MiB). Per chunk, on the
// caller's stream: zero the ticket, one GEN launch, one resolve launch. The
// stream orders a chunk's resolve after its trace and the next chunk's trace
// after that resolve, so one buffer and one ticket serve every chunk and the
// host never waits. Within a launch the ticket counter is still the only state
// waves share: a wave's loop ends when its lanes hold no ray and every ticket
// has been handed out, each ray tree is bounded by the depth, and no wave
// waits for another -- nothing can hang, as for the radiance queries.
//
// Adaptive renders (rt_render_camera_adaptive_async): per-pixel sample counts
// chosen on the device. Passes double the samples of the pixels still active;
// per chunk and pass one launch of rt_trace_kernel<.., GEN, ADP> -- ticket t is
// sample s0 + t % b of the pass's list entry t / b, and the number of entries
// is read from device memory (cam_ticket_limit), so the host enqueues every
// pass without knowing how many pixels are active -- and one cam_adapt_kernel
// launch, which continues the pixels' sums, applies the stopping rule, writes
// the final pixels and lists the others for the next pass. The ADP flag keeps
// this refill out of the fixed render's instantiations, whose registers have
// no room for it (DESIGN.md "Adaptive camera renders"). An empty pass drains
// at the first refill; nothing can hang, by the argument above.
//
// Variance (rt_render_camera_var_async, rt_render_camera_adaptive_var_async):
// the squared standard error of each pixel's mean from the sums the adaptive
// rule already keeps (cam_var). The fixed render resolves through
// cam_resolve_var_kernel, a sibling of cam_resolve_kernel that also carries
// the sum of squares, only when the caller gives a d_var; the adapt kernel
// writes it where it writes the mean. Nothing else of a render changes.
//
// PCG position: sample s of row y starts ((y mod 20) * S + s) * D draws into
// its column's strip stream (D draws per sample), at most 81 916 < 2^17. The
// lane jumps there by binary decomposition: the LCG's 2^k-step maps (A, C),
// k = 0..16, are compile-time constants, and the lane applies the maps of the
// set bits of its offset (pcg_jump, as the render kernel does with its
// host-built table).
//
// Shared pieces used here, each defined once elsewhere: ray_store and flavour
// (rt_query.hip); wave_take, the wave-aggregated atomicAdd of the adaptive list
// append, and ray_out_check (rt_trace.hip: wave_take has to precede the
// radiance kernel, whose ticket refill is its other caller); grow and
// need_scene (rt_kernel.hip, beside the context). pack_rgba8 below serves both
// the resolve and the adapt kernel.
// Included by rt_kernel.hip after rt_trace.hip.

namespace {

constexpr int CAM_BUF_RECORDS = 2097152;  // rt_radiance records of the sample buffer, at most (64 MiB)
constexpr int CAM_JUMP_BITS = 17;         // offsets below 2^17: 19 * 1024 * 4 + 1023 * 4 = 81 916

struct CamJumpPow {
  uint64_t v[CAM_JUMP_BITS][4];  // [k]: ahi alo chi clo of 2^k LCG steps
};

constexpr CamJumpPow cam_jump_pow() {
  typedef unsigned __int128 u128;
  const u128 mul = ((u128)2549297995355413924ULL << 64) | 4865540595714422341ULL;  // pcg.go
  const u128 inc = ((u128)6364136223846793005ULL << 64) | 1442695040888963407ULL;
  CamJumpPow t = {};
  u128 A = mul, Cc = inc;
  for (int k = 0; k < CAM_JUMP_BITS; k++) {
    t.v[k][0] = (uint64_t)(A >> 64);
    t.v[k][1] = (uint64_t)A;
    t.v[k][2] = (uint64_t)(Cc >> 64);
    t.v[k][3] = (uint64_t)Cc;
    Cc = Cc * A + Cc;  // twice the steps: x -> A (A x + C) + C
    A = A * A;
  }
  return t;
}

__constant__ const CamJumpPow k_cam_jump = cam_jump_pow();

// The camera of a launch, derived on the host (cam_setup): wave-uniform.
struct CamArgs {
  int model, posed;
  int S, D;       // samples per pixel, draws per sample
  int W, H;       // the camera's frame
  int first;      // frame pixel (y * W + x) of ticket 0 / of the rays kernel's first row
  int nbits;      // bit length of the largest draw offset: 19 * S * D + (S - 1) * D
  double W1, H1;  // float(W - 1), float(H - 1)
  double vw, vh;
  double half_ap, focus;               // thin lens: aperture / 2, focal-plane distance
  double eye[3], r[3], w[3], f[3];     // posed: the eye and the basis (right, up, forward)
  // a pass of an adaptive render (the ADP instantiations; a fixed render reads none of these):
  // ticket t is sample s0 + t % b of pixel first + (list ? list[t / b] : t / b)
  int s0, b;
  const int* list;            // a pass of an adaptive render: its active pixels, relative to `first`
  const unsigned int* count;  // ... and how many there are (device memory, written by the pass before)
};

template <>
struct TraceArgsT<true> : TraceArgs {
  CamArgs cam;
};

// Sample s of frame pixel `pixel`: the ray of include/rt_abi.h "Camera
// renders", operation for operation. The one ray-forming function: the GEN
// refill of rt_trace_kernel and cam_rays_kernel both call it.
__device__ __forceinline__ void cam_ray(const CamArgs& A, int pixel, int s, d3& ro, d3& rd) {
  const int y = pixel / A.W, x = pixel - y * A.W;
  const int ry = y % 20;
  Pcg rng{0xDEADULL ^ (uint64_t)x, 0xBEEFULL ^ (uint64_t)(y - ry)};  // raytracer.go:632-634
  const unsigned int off = ((unsigned int)ry * (unsigned int)A.S + (unsigned int)s) * (unsigned int)A.D;
  for (int k = 0; k < A.nbits; k++) {  // (wave-uniform k: the table through scalar loads)
    const uint64_t* j = k_cam_jump.v[k];
    if ((off >> k) & 1u) rng = pcg_jump(rng, j[0], j[1], j[2], j[3]);
  }
  const double dx = pcg_float64(rng) - 0.5;
  const double dy = pcg_float64(rng) - 0.5;
  const double su = ((double)x + dx) / A.W1;
  const double sv = ((double)y + dy) / A.H1;
  const d3 e = mk(0.0, 0.0, -1.0);  // raytracer.go:605-609
  d3 o, d;
  if (A.model == RT_CAMERA_EQUIRECT) {
    const double th = (su - 0.5) * 360.0, ph = (0.5 - sv) * 180.0;
    const double st = rt::go_sin(0.017453292519943295 * th), ct = rt::go_cos(0.017453292519943295 * th);
    const double sp = rt::go_sin(0.017453292519943295 * ph), cp = rt::go_cos(0.017453292519943295 * ph);
    o = e;
    d = mk(st * cp, sp, ct * cp);
  } else {
    const double u = su * A.vw - A.vw / 2.0;
    const double v = sv * A.vh - A.vh / 2.0;
    o = mk(u, -v, 0.0);
    if (A.model == RT_CAMERA_ORTHO) {
      d = mk(0.0, 0.0, 1.0);
    } else {
      d = norm(sub(o, e));
      if (A.model == RT_CAMERA_THINLENS) {
        const double d2 = pcg_float64(rng), d3_ = pcg_float64(rng);
        const d3 P = add(e, scale(d, A.focus / d.z));
        const double rho = A.half_ap * __builtin_sqrt(d2), al = 360.0 * d3_;
        const double ca = rt::go_cos(0.017453292519943295 * al), sa = rt::go_sin(0.017453292519943295 * al);
        const d3 L = add(e, mk(rho * ca, rho * sa, 0.0));
        o = L;
        d = norm(sub(P, L));
      }
    }
  }
  if (A.posed) {
    const double pz = o.z + 1.0;
    ro = mk(A.eye[0] + o.x * A.r[0] + o.y * A.w[0] + pz * A.f[0], A.eye[1] + o.x * A.r[1] + o.y * A.w[1] + pz * A.f[1],
            A.eye[2] + o.x * A.r[2] + o.y * A.w[2] + pz * A.f[2]);
    rd = mk(d.x * A.r[0] + d.y * A.w[0] + d.z * A.f[0], d.x * A.r[1] + d.y * A.w[1] + d.z * A.f[1],
            d.x * A.r[2] + d.y * A.w[2] + d.z * A.f[2]);
  } else {
    ro = o;
    rd = d;
  }
}

// Ticket t of a GEN launch (t < n <= CAM_BUF_RECORDS)
__device__ __forceinline__ void cam_ticket_ray(const CamArgs& A, unsigned int t, BoolC<false>, d3& ro, d3& rd) {
  const unsigned int p = t / (unsigned int)A.S;
  cam_ray(A, A.first + (int)p, (int)(t - p * (unsigned int)A.S), ro, rd);
}

// ... of a pass of an adaptive render (the ADP instantiations). One
// wave-uniform branch on the list pointer: pass 0 has no list.
__device__ __forceinline__ void cam_ticket_ray(const CamArgs& A, unsigned int t, BoolC<true>, d3& ro, d3& rd) {
  const unsigned int p = t / (unsigned int)A.b;
  int pixel = (int)p;
  if (A.list) pixel = A.list[p];
  cam_ray(A, A.first + pixel, A.s0 + (int)(t - p * (unsigned int)A.b), ro, rd);
}

// Tickets of an ADP launch of at most n = pixels * b: min(*count, pixels) * b
// when the launch has a count, read once per wave. The clamp keeps a ticket
// inside the chunk's sample buffer and list whatever the count holds.
__device__ __forceinline__ unsigned int cam_ticket_limit(const CamArgs& A, unsigned int n) {
  if (!A.count) return n;
  const unsigned long long m = (unsigned long long)*A.count * (unsigned int)A.b;
  return m < (unsigned long long)n ? (unsigned int)m : n;
}

// rt_camera_rays_async: one thread per (pixel, sample) of the band
__global__ __launch_bounds__(WG) void cam_rays_kernel(CamArgs A, long long n, rt_ray* out) {
  const long long tid = (long long)blockIdx.x * WG + threadIdx.x;
  if (tid >= n) return;
  const long long p = tid / A.S;
  d3 o, d;
  cam_ray(A, A.first + (int)p, (int)(tid - p * A.S), o, d);
  ray_store(out + tid, o, d);
}

// A pixel's mean colour quantised as Render() does: 16 bits, the high byte kept
__device__ __forceinline__ uint32_t pack_rgba8(const d3& c) {
  const uint32_t r8 = go_f64_to_u32(c.x * 65535.0) >> 8;
  const uint32_t g8 = go_f64_to_u32(c.y * 65535.0) >> 8;
  const uint32_t b8 = go_f64_to_u32(c.z * 65535.0) >> 8;
  return (r8 & 0xffu) | ((g8 & 0xffu) << 8) | ((b8 & 0xffu) << 16) | 0xff000000u;
}

// One thread per pixel of a chunk: the pixel's S records (two 16-byte loads
// each) added in sample order, scaled by 1 / S, quantised as Render() does.
// `px0`: the chunk's first pixel relative to the band (the outputs' origin).
__global__ __launch_bounds__(WG) void cam_resolve_kernel(const rt_radiance* __restrict__ rec, int npix, int S,
                                                          double inv, long long px0, uint32_t* rgba, double* mean) {
  const int p = (int)(blockIdx.x * WG + threadIdx.x);
  if (p >= npix) return;
  const Q16* rp = reinterpret_cast<const Q16*>(rec + (size_t)p * S);
  Q16 a = rp[0], b = rp[1];
  d3 sum = mk(a.a, a.b, b.a);
  for (int s = 1; s < S; s++) {
    a = rp[2 * s];
    b = rp[2 * s + 1];
    sum = add(sum, mk(a.a, a.b, b.a));
  }
  const d3 c = scale(sum, inv);
  const long long q = px0 + p;
  if (mean) {
    mean[q * 3 + 0] = c.x;
    mean[q * 3 + 1] = c.y;
    mean[q * 3 + 2] = c.z;
  }
  if (rgba) rgba[q] = pack_rgba8(c);
}

// A channel's squared standard error of the mean from its sum, sum of squares
// and mean (include/rt_abi.h "Variance of a camera render"): the adaptive
// rule's e_c, a negative estimate clamped to 0, a NaN kept.
__device__ __forceinline__ double cam_var(double sum, double sq, double m, double den) {
  const double e = (sq - sum * m) / den;
  return e < 0.0 ? 0.0 : e;
}

// cam_resolve_kernel with the second moment (rt_render_camera_var_async with a
// d_var): Sum as there, Q beside it in the adaptive state's order, and the
// variance of the mean written next to the mean. A sibling, not a template
// parameter, so the kernel above stays the code object it was.
__global__ __launch_bounds__(WG) void cam_resolve_var_kernel(const rt_radiance* __restrict__ rec, int npix, int S,
                                                              double inv, long long px0, uint32_t* rgba, double* mean,
                                                              double* var) {
  const int p = (int)(blockIdx.x * WG + threadIdx.x);
  if (p >= npix) return;
  const Q16* rp = reinterpret_cast<const Q16*>(rec + (size_t)p * S);
  Q16 a = rp[0], b = rp[1];
  d3 sum = mk(a.a, a.b, b.a);
  d3 sq = mul(sum, sum);
  for (int s = 1; s < S; s++) {
    a = rp[2 * s];
    b = rp[2 * s + 1];
    const d3 c = mk(a.a, a.b, b.a);
    sum = add(sum, c);
    sq = add(sq, mul(c, c));
  }
  const d3 c = scale(sum, inv);
  const double den = (double)(S * (S - 1));
  const long long q = px0 + p;
  if (mean) {
    mean[q * 3 + 0] = c.x;
    mean[q * 3 + 1] = c.y;
    mean[q * 3 + 2] = c.z;
  }
  var[q * 3 + 0] = cam_var(sum.x, sq.x, c.x, den);
  var[q * 3 + 1] = cam_var(sum.y, sq.y, c.y, den);
  var[q * 3 + 2] = cam_var(sum.z, sq.z, c.z, den);
  if (rgba) rgba[q] = pack_rgba8(c);
}

// One pass of an adaptive render (include/rt_abi.h "Adaptive camera renders").
struct AdaptArgs {
  const rt_radiance* rec;      // the pass's records: entry j's b samples at rec[j * b ..]
  int npix;                    // pixels of the chunk
  int b, n, S;                 // the pass's batch, samples per active pixel after it, the cap
  double tol2;
  const int* list;             // the pass's active pixels (NULL: pass 0, entry j is pixel j)
  const unsigned int* count;   // ... and their number (NULL: npix)
  int* next;                   // the next pass's list and count (unused when n == S)
  unsigned int* next_count;
  double* state;               // [6][npix]: sum r g b, sum of squares r g b
  long long px0;               // the chunk's first pixel relative to the band
  uint32_t* rgba;
  double* mean;
  int32_t* samples;
  double* var;                 // the variance of the final pixels' means (NULL: not wanted)
};

// One thread per active list entry: the entry's b records added to the pixel's
// running sums in sample order, then the stopping rule. A pixel that is
// converged, or holds S samples, is written out; any other goes to the next
// pass's list (one atomic per wave, rank by popcount; the order of a list does
// not matter to any output).
__global__ __launch_bounds__(WG) void cam_adapt_kernel(AdaptArgs A) {
  const unsigned int j = blockIdx.x * WG + threadIdx.x;
  unsigned int lim = (unsigned int)A.npix;
  if (A.count) {
    const unsigned int cnt = *A.count;
    if (cnt < lim) lim = cnt;
  }
  bool valid = j < lim;
  unsigned int p = j;
  if (valid && A.list) {
    p = (unsigned int)A.list[j];
    valid = p < (unsigned int)A.npix;  // (always, for a list this kernel wrote)
  }
  bool again = false;
  if (valid) {
    const Q16* rp = reinterpret_cast<const Q16*>(A.rec + (size_t)j * A.b);
    double* st = A.state + p;
    const size_t np = (size_t)A.npix;
    d3 sum, sq;
    int s = 0;
    if (A.list) {
      sum = mk(st[0], st[np], st[2 * np]);
      sq = mk(st[3 * np], st[4 * np], st[5 * np]);
    } else {
      const Q16 a = rp[0], b = rp[1];
      sum = mk(a.a, a.b, b.a);
      sq = mul(sum, sum);
      s = 1;
    }
    for (; s < A.b; s++) {
      const Q16 a = rp[2 * s], b = rp[2 * s + 1];
      const d3 c = mk(a.a, a.b, b.a);
      sum = add(sum, c);
      sq = add(sq, mul(c, c));
    }
    const double inv = 1.0 / (double)A.n;
    const d3 m = scale(sum, inv);
    const d3 v = sub(sq, mul(sum, m));
    const double den = (double)(A.n * (A.n - 1));
    const bool conv = v.x / den <= A.tol2 && v.y / den <= A.tol2 && v.z / den <= A.tol2;
    if (conv || A.n >= A.S) {
      const long long q = A.px0 + p;
      if (A.mean) {
        A.mean[q * 3 + 0] = m.x;
        A.mean[q * 3 + 1] = m.y;
        A.mean[q * 3 + 2] = m.z;
      }
      if (A.var) {
        A.var[q * 3 + 0] = cam_var(sum.x, sq.x, m.x, den);
        A.var[q * 3 + 1] = cam_var(sum.y, sq.y, m.y, den);
        A.var[q * 3 + 2] = cam_var(sum.z, sq.z, m.z, den);
      }
      if (A.rgba) A.rgba[q] = pack_rgba8(m);
      if (A.samples) A.samples[q] = A.n;
    } else {
      st[0] = sum.x;
      st[np] = sum.y;
      st[2 * np] = sum.z;
      st[3 * np] = sq.x;
      st[4 * np] = sq.y;
      st[5 * np] = sq.z;
      again = true;
    }
  }
  const uint64_t am = wave_ballot(again);
  if (am) {
    unsigned int base;
    const unsigned int at = wave_take(A.next_count, am, (int)(threadIdx.x & 63), base);
    if (again && at < (unsigned int)A.npix) A.next[at] = (int)p;
  }
}

// [BVH | CSG << 1 | VM << 2], as k_trace_kernels
const void* const k_camera_kernels[8] = {
    (const void*)rt_trace_kernel<false, false, false, true>, (const void*)rt_trace_kernel<true, false, false, true>,
    (const void*)rt_trace_kernel<false, true, false, true>,  (const void*)rt_trace_kernel<true, true, false, true>,
    (const void*)rt_trace_kernel<false, false, true, true>,  (const void*)rt_trace_kernel<true, false, true, true>,
    (const void*)rt_trace_kernel<false, true, true, true>,   (const void*)rt_trace_kernel<true, true, true, true>};

// ... with the adaptive refill: the passes of rt_render_camera_adaptive_async
const void* const k_adaptive_kernels[8] = {
    (const void*)rt_trace_kernel<false, false, false, true, true>, (const void*)rt_trace_kernel<true, false, false, true, true>,
    (const void*)rt_trace_kernel<false, true, false, true, true>,  (const void*)rt_trace_kernel<true, true, false, true, true>,
    (const void*)rt_trace_kernel<false, false, true, true, true>,  (const void*)rt_trace_kernel<true, false, true, true, true>,
    (const void*)rt_trace_kernel<false, true, true, true, true>,   (const void*)rt_trace_kernel<true, true, true, true, true>};

struct CamPlan {
  CamArgs A;
  int depth;         // of the trace
  long long pixels;  // of the band
  int chunk;         // pixels per chunk
  int chunks;
};

bool cam_finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// Validate `cam` (NULL: all zeros) and the rows against the context's scene
// and derive the launch's camera, in the order include/rt_abi.h states.
int cam_setup(rt_context* c, const rt_camera* cam, int y0, int y1, const char* who, CamPlan& P) {
  const std::string w = std::string(who) + ": ";
  if (int rc = need_scene(c, who); rc != RT_OK) return rc;
  rt_camera z;
  std::memset(&z, 0, sizeof z);
  if (cam) z = *cam;
  const DevScene& s = c->sc;
  CamArgs& A = P.A;
  std::memset(&A, 0, sizeof A);
  if (z.model < RT_CAMERA_PINHOLE || z.model > RT_CAMERA_THINLENS) return fail(RT_E_INVALID, w + "unknown camera model");
  if (z.flags & ~RT_CAMERA_POSED) return fail(RT_E_INVALID, w + "unknown flag bits");
  if (z.samples < 0 || z.samples > RT_CAMERA_MAX_SAMPLES)
    return fail(RT_E_INVALID, w + "samples outside [0, RT_CAMERA_MAX_SAMPLES]");
  if (!((z.width == 0 && z.height == 0) || (z.width >= 2 && z.height >= 2)))
    return fail(RT_E_INVALID, w + "width and height must both be 0 or both be >= 2");
  A.model = z.model;
  A.posed = (z.flags & RT_CAMERA_POSED) ? 1 : 0;
  A.S = z.samples == 0 ? 4 : z.samples;
  A.D = z.model == RT_CAMERA_THINLENS ? 4 : 2;
  A.W = z.width ? z.width : s.width;
  A.H = z.height ? z.height : s.height;
  if ((long long)A.W * A.H > 2147483647LL) return fail(RT_E_INVALID, w + "the frame has more than 2^31 - 1 pixels");
  if (z.depth < 0) return fail(RT_E_INVALID, w + "depth outside [0, RT_RADIANCE_MAX_DEPTH]");
  if (int rc = trace_depth(c, who, z.depth, &P.depth); rc != RT_OK) return rc;
  if (z.chunk_pixels < 0) return fail(RT_E_INVALID, w + "chunk_pixels < 0");
  if (y0 < 0 || y1 > A.H || y0 >= y1) return fail(RT_E_INVALID, w + "rows must satisfy 0 <= y0 < y1 <= height");
  const unsigned int maxoff = (19u * (unsigned int)A.S + (unsigned int)(A.S - 1)) * (unsigned int)A.D;
  while (A.nbits < CAM_JUMP_BITS && (maxoff >> A.nbits) != 0) A.nbits++;
  A.W1 = (double)(A.W - 1);
  A.H1 = (double)(A.H - 1);
  // the view width
  if (z.model == RT_CAMERA_ORTHO) {
    if (!(z.extent > 0.0) || !std::isfinite(z.extent)) return fail(RT_E_INVALID, w + "extent must be > 0 and finite");
    A.vw = z.extent;
  } else if (z.model != RT_CAMERA_EQUIRECT && z.fov > 0.0) {
    const double fovr = z.fov * M_PI / 180.0;  // raytracer.go:601-602, as rt_set_scene
    double tn;
    if (!go_tan(fovr / 2.0, tn) || !(tn > 0.0) || !std::isfinite(2.0 / tn))
      return fail(RT_E_INVALID, w + "fov: its Tan is not a positive finite number");
    A.vw = 2.0 / tn;
  } else {
    if (z.model != RT_CAMERA_EQUIRECT && z.fov != z.fov) return fail(RT_E_INVALID, w + "fov is NaN");
    A.vw = s.vw;
  }
  A.vh = A.vw * ((double)A.H / (double)A.W);  // raytracer.go:603
  if (z.model == RT_CAMERA_THINLENS) {
    if (!(z.aperture >= 0.0) || !std::isfinite(z.aperture))
      return fail(RT_E_INVALID, w + "aperture must be >= 0 and finite");
    if (!(z.focus > 0.0) || !std::isfinite(z.focus)) return fail(RT_E_INVALID, w + "focus must be > 0 and finite");
    A.half_ap = z.aperture / 2.0;
    A.focus = z.focus;
  }
  if (A.posed) {
    if (!cam_finite3(z.eye) || !cam_finite3(z.look_at) || !cam_finite3(z.up))
      return fail(RT_E_INVALID, w + "eye, look_at and up must be finite");
    const double g[3] = {z.look_at[0] - z.eye[0], z.look_at[1] - z.eye[1], z.look_at[2] - z.eye[2]};
    const double gl = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    if (!(gl > 0.0) || !std::isfinite(gl)) return fail(RT_E_INVALID, w + "eye == look_at (or too far apart)");
    const double f[3] = {g[0] / gl, g[1] / gl, g[2] / gl};
    const double* u = z.up;
    const double x[3] = {u[1] * f[2] - u[2] * f[1], u[2] * f[0] - u[0] * f[2], u[0] * f[1] - u[1] * f[0]};
    const double xl = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    if (!(xl > 0.0) || !std::isfinite(xl)) return fail(RT_E_INVALID, w + "up is parallel to the view direction");
    const double r[3] = {x[0] / xl, x[1] / xl, x[2] / xl};
    const double wv[3] = {f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]};
    for (int k = 0; k < 3; k++) {
      A.eye[k] = z.eye[k];
      A.r[k] = r[k];
      A.w[k] = wv[k];
      A.f[k] = f[k];
    }
  }
  A.first = y0 * A.W;
  P.pixels = (long long)A.W * (y1 - y0);
  P.chunk = std::max(1, CAM_BUF_RECORDS / A.S);
  if (z.chunk_pixels > 0) P.chunk = std::min(P.chunk, z.chunk_pixels);
  const long long nch = (P.pixels + P.chunk - 1) / P.chunk;
  if (nch > 2147483647LL) return fail(RT_E_INVALID, w + "chunk_pixels cuts the band into more than 2^31 - 1 chunks");
  P.chunks = (int)nch;
  return RT_OK;
}

// The pixel outputs both renders share
int cam_out_check(const void* d_rgba, const double* d_mean, const char* who) {
  if (((uintptr_t)d_rgba & 3) != 0) return fail(RT_E_INVALID, std::string(who) + ": d_rgba must be 4-byte aligned");
  if (((uintptr_t)d_mean & 7) != 0) return fail(RT_E_INVALID, std::string(who) + ": d_mean must be 8-byte aligned");
  return RT_OK;
}

// d_var of the two renders that write a variance: NULL is "not wanted"
int cam_var_check(const double* d_var, int S, const char* who) {
  if (!d_var) return RT_OK;
  if (((uintptr_t)d_var & 7) != 0) return fail(RT_E_INVALID, std::string(who) + ": d_var must be 8-byte aligned");
  if (S < 2) return fail(RT_E_INVALID, std::string(who) + ": d_var needs at least 2 samples");
  return RT_OK;
}

// Adaptive renders: the pass schedule and the chunking that goes with it.
constexpr int CAM_ADAPT_MAX_PASSES = 12;     // min_samples 2 -> cap 1024: 10 passes
constexpr int CAM_ADAPT_MAX_CHUNK = 524288;  // pixels of a chunk, at most: bounds the state and the lists (28 MiB)
constexpr size_t CAM_ADAPT_CTL = 256;        // bytes: counts[passes] then tickets[passes], 32-bit each

struct AdaptPlan {
  double tol2;
  int passes;
  int n[CAM_ADAPT_MAX_PASSES];  // samples of an active pixel after pass k
  int B;                        // the largest batch
};

// Validate `ad` against the camera of `P` and rework P's chunks for the
// schedule's largest batch, in the order include/rt_abi.h states.
int adapt_setup(const rt_adaptive* ad, const rt_camera* cam, const char* who, CamPlan& P, AdaptPlan& D) {
  const std::string w = std::string(who) + ": ";
  const int S = P.A.S;
  if (!ad) return fail(RT_E_INVALID, w + "NULL rt_adaptive");
  if (ad->reserved != 0) return fail(RT_E_INVALID, w + "rt_adaptive.reserved must be 0");
  if (S < 2) return fail(RT_E_INVALID, w + "an adaptive render needs a cap of at least 2 samples");
  const int n0 = ad->min_samples == 0 ? std::min(4, S) : ad->min_samples;
  if (n0 < 2 || n0 > S) return fail(RT_E_INVALID, w + "min_samples must satisfy 2 <= min_samples <= samples");
  if (!(ad->tolerance >= 0.0)) return fail(RT_E_INVALID, w + "tolerance must be >= 0 and not NaN");
  D.tol2 = ad->tolerance * ad->tolerance;
  D.passes = 0;
  D.B = n0;
  for (int n = n0;; n = std::min(2 * n, S)) {
    if (D.passes > 0) D.B = std::max(D.B, n - D.n[D.passes - 1]);
    D.n[D.passes++] = n;
    if (n == S) break;
  }
  P.chunk = std::max(1, std::min(CAM_ADAPT_MAX_CHUNK, CAM_BUF_RECORDS / D.B));
  if (cam && cam->chunk_pixels > 0) P.chunk = std::min(P.chunk, cam->chunk_pixels);
  const long long nch = (P.pixels + P.chunk - 1) / P.chunk;
  if (nch > 2147483647LL) return fail(RT_E_INVALID, w + "chunk_pixels cuts the band into more than 2^31 - 1 chunks");
  P.chunks = (int)nch;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_camera_rays_async(rt_context* c, const rt_camera* cam, int y0, int y1, rt_ray* d_rays, void* stream) {
  const char* who = "rt_camera_rays_async";
  CamPlan P;
  if (int rc = cam_setup(c, cam, y0, y1, who, P); rc != RT_OK) return rc;
  if (int rc = ray_out_check(d_rays, who); rc != RT_OK) return rc;
  DeviceGuard guard(c->device);
  long long n = P.pixels * P.A.S;
  const long long blocks = (n + WG - 1) / WG;
  if (blocks > 2147483647LL) return fail(RT_E_INVALID, std::string(who) + ": too many rays for one launch");
  void* args[] = {(void*)&P.A, (void*)&n, (void*)&d_rays};
  HIP_TRY(hipLaunchKernel((const void*)cam_rays_kernel, dim3((unsigned)blocks), dim3(WG), args, 0, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int rt_render_camera_chunks(rt_context* c, const rt_camera* cam, int y0, int y1) {
  CamPlan P;
  if (int rc = cam_setup(c, cam, y0, y1, "rt_render_camera_chunks", P); rc != RT_OK) return rc;
  return P.chunks;
}

}  // extern "C"

namespace {

// rt_render_camera_async (`var_call` false: d_var is NULL) and rt_render_camera_var_async
int cam_render(rt_context* c, const rt_camera* cam, int y0, int y1, void* d_rgba, double* d_mean, double* d_var,
               void* stream, const char* who, bool var_call) {
  CamPlan P;
  if (int rc = cam_setup(c, cam, y0, y1, who, P); rc != RT_OK) return rc;
  if (!d_rgba && !d_mean && !d_var)
    return fail(RT_E_INVALID, std::string(who) + (var_call ? ": d_rgba, d_mean and d_var are all NULL"
                                                           : ": d_rgba and d_mean are both NULL"));
  if (int rc = cam_out_check(d_rgba, d_mean, who); rc != RT_OK) return rc;
  if (int rc = cam_var_check(d_var, P.A.S, who); rc != RT_OK) return rc;
  const DevScene& s = c->sc;
  DeviceGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  int S = P.A.S;
  // the sample buffer: grown when a call needs more (calls on a context are ordered)
  const size_t need = (size_t)std::min<long long>(P.pixels, P.chunk) * S * sizeof(rt_radiance);
  if (int rc = grow(c->cam_buf, c->cam_buf_bytes, need); rc != RT_OK) return rc;
  const void* kfn = k_camera_kernels[flavour(s)];
  const char* blob = s.blob;
  const rt_radiance* rec = c->cam_buf;
  uint32_t* rgba = (uint32_t*)d_rgba;
  double inv = 1.0 / (double)S;
  for (long long px0 = 0; px0 < P.pixels; px0 += P.chunk) {
    int npix = (int)std::min<long long>(P.chunk, P.pixels - px0);
    TraceArgsT<true> Q;
    std::memset(&Q, 0, sizeof Q);
    int wgs = 0;
    if (int rc = trace_prepare(c, npix * S, P.depth, nullptr, c->cam_buf, st, Q, wgs); rc != RT_OK) return rc;
    Q.cam = P.A;
    Q.cam.first = P.A.first + (int)px0;
    void* targs[] = {(void*)&blob, (void*)&Q};
    HIP_TRY(hipLaunchKernel(kfn, dim3((unsigned)wgs), dim3(WG), targs, 0, st));
    void* rargs[] = {(void*)&rec,  (void*)&npix,   (void*)&S,    (void*)&inv, (void*)&px0,
                     (void*)&rgba, (void*)&d_mean, (void*)&d_var};  // (the plain kernel takes the first seven)
    HIP_TRY(hipLaunchKernel(d_var ? (const void*)cam_resolve_var_kernel : (const void*)cam_resolve_kernel,
                            dim3((unsigned)((npix + WG - 1) / WG)), dim3(WG), rargs, 0, st));
  }
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_render_camera_async(rt_context* c, const rt_camera* cam, int y0, int y1, void* d_rgba, double* d_mean,
                           void* stream) {
  return cam_render(c, cam, y0, y1, d_rgba, d_mean, nullptr, stream, "rt_render_camera_async", false);
}

int rt_render_camera_var_async(rt_context* c, const rt_camera* cam, int y0, int y1, void* d_rgba, double* d_mean,
                               double* d_var, void* stream) {
  return cam_render(c, cam, y0, y1, d_rgba, d_mean, d_var, stream, "rt_render_camera_var_async", true);
}

int rt_render_camera_adaptive_plan(rt_context* c, const rt_camera* cam, const rt_adaptive* ad, int y0, int y1,
                                   int* chunks, int* passes) {
  const char* who = "rt_render_camera_adaptive_plan";
  CamPlan P;
  AdaptPlan D;
  if (int rc = cam_setup(c, cam, y0, y1, who, P); rc != RT_OK) return rc;
  if (int rc = adapt_setup(ad, cam, who, P, D); rc != RT_OK) return rc;
  if (chunks) *chunks = P.chunks;
  if (passes) *passes = D.passes;
  return RT_OK;
}

}  // extern "C"

namespace {

// rt_render_camera_adaptive_async (`var_call` false: d_var is NULL) and rt_render_camera_adaptive_var_async
int cam_render_adaptive(rt_context* c, const rt_camera* cam, const rt_adaptive* ad, int y0, int y1, void* d_rgba,
                        double* d_mean, int32_t* d_samples, double* d_var, void* stream, const char* who,
                        bool var_call) {
  CamPlan P;
  AdaptPlan D;
  if (int rc = cam_setup(c, cam, y0, y1, who, P); rc != RT_OK) return rc;
  if (int rc = adapt_setup(ad, cam, who, P, D); rc != RT_OK) return rc;
  if (!d_rgba && !d_mean && !d_samples && !d_var)
    return fail(RT_E_INVALID, std::string(who) + (var_call ? ": d_rgba, d_mean, d_samples and d_var are all NULL"
                                                           : ": d_rgba, d_mean and d_samples are all NULL"));
  if (int rc = cam_out_check(d_rgba, d_mean, who); rc != RT_OK) return rc;
  if (((uintptr_t)d_samples & 3) != 0)
    return fail(RT_E_INVALID, std::string(who) + ": d_samples must be 4-byte aligned");
  if (int rc = cam_var_check(d_var, P.A.S, who); rc != RT_OK) return rc;
  const DevScene& s = c->sc;
  DeviceGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  // the sample buffer (shared with the fixed renders), then the state: both grown when a call needs more
  const size_t cpix = (size_t)std::min<long long>(P.pixels, P.chunk);  // pixels of the largest chunk
  const size_t need = cpix * D.B * sizeof(rt_radiance);
  if (int rc = grow(c->cam_buf, c->cam_buf_bytes, need); rc != RT_OK) return rc;
  // [counts and tickets][state: 6 doubles per pixel][two lists]
  const size_t aneed = CAM_ADAPT_CTL + cpix * (6 * sizeof(double) + 2 * sizeof(int));
  if (int rc = grow(c->cam_adapt, c->cam_adapt_bytes, aneed); rc != RT_OK) return rc;
  unsigned int* counts = reinterpret_cast<unsigned int*>(c->cam_adapt);
  unsigned int* tickets = counts + CAM_ADAPT_MAX_PASSES;
  double* state = reinterpret_cast<double*>(c->cam_adapt + CAM_ADAPT_CTL);
  int* lists[2] = {reinterpret_cast<int*>(state + 6 * cpix), reinterpret_cast<int*>(state + 6 * cpix) + cpix};
  // the frame stack for the largest launch of the call, and the argument record every launch starts from
  TraceArgsT<true> Q0;
  std::memset(&Q0, 0, sizeof Q0);
  int wgs_max = 0;
  if (int rc = trace_prepare(c, (int)cpix * D.B, P.depth, nullptr, c->cam_buf, st, Q0, wgs_max); rc != RT_OK) return rc;
  Q0.cam = P.A;
  const int grid = trace_grid_wgs(c, P.depth);
  const void* kfn = k_adaptive_kernels[flavour(s)];
  const char* blob = s.blob;
  for (long long px0 = 0; px0 < P.pixels; px0 += P.chunk) {
    const int npix = (int)std::min<long long>(P.chunk, P.pixels - px0);
    HIP_TRY(hipMemsetAsync(c->cam_adapt, 0, CAM_ADAPT_CTL, st));
    for (int k = 0; k < D.passes; k++) {
      const int s0 = k == 0 ? 0 : D.n[k - 1], b = D.n[k] - s0;
      // pass k reads list k & 1 and counts[k] (pass 0: every pixel), and fills list (k + 1) & 1 and counts[k + 1]
      const int* list = k == 0 ? nullptr : lists[k & 1];
      const unsigned int* count = k == 0 ? nullptr : counts + k;
      TraceArgsT<true> Q = Q0;
      Q.n = npix * b;
      Q.ticket = tickets + k;
      Q.cam.first = P.A.first + (int)px0;
      Q.cam.s0 = s0;
      Q.cam.b = b;
      Q.cam.list = list;
      Q.cam.count = count;
      const int wgs = std::min(grid, (Q.n + WG - 1) / WG);
      void* targs[] = {(void*)&blob, (void*)&Q};
      HIP_TRY(hipLaunchKernel(kfn, dim3((unsigned)wgs), dim3(WG), targs, 0, st));
      AdaptArgs R;
      std::memset(&R, 0, sizeof R);
      R.rec = c->cam_buf;
      R.npix = npix;
      R.b = b;
      R.n = D.n[k];
      R.S = P.A.S;
      R.tol2 = D.tol2;
      R.list = list;
      R.count = count;
      R.next = lists[(k + 1) & 1];
      R.next_count = counts + k + 1;
      R.state = state;
      R.px0 = px0;
      R.rgba = (uint32_t*)d_rgba;
      R.mean = d_mean;
      R.samples = d_samples;
      R.var = d_var;
      void* rargs[] = {(void*)&R};
      HIP_TRY(hipLaunchKernel((const void*)cam_adapt_kernel, dim3((unsigned)((npix + WG - 1) / WG)), dim3(WG), rargs, 0,
                              st));
    }
  }
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_render_camera_adaptive_async(rt_context* c, const rt_camera* cam, const rt_adaptive* ad, int y0, int y1,
                                    void* d_rgba, double* d_mean, int32_t* d_samples, void* stream) {
  return cam_render_adaptive(c, cam, ad, y0, y1, d_rgba, d_mean, d_samples, nullptr, stream,
                             "rt_render_camera_adaptive_async", false);
}

int rt_render_camera_adaptive_var_async(rt_context* c, const rt_camera* cam, const rt_adaptive* ad, int y0, int y1,
                                        void* d_rgba, double* d_mean, int32_t* d_samples, double* d_var,
                                        void* stream) {
  return cam_render_adaptive(c, cam, ad, y0, y1, d_rgba, d_mean, d_samples, d_var, stream,
                             "rt_render_camera_adaptive_var_async", true);
}

}  // extern "C"
