// rt_aov.hip -- feature buffers of a camera render and the guided a-trous
// denoiser (include/rt_abi.h "Feature buffers": rt_render_camera_aov_async,
// rt_denoise_atrous_async; "Variance-guided a-trous filter":
// rt_denoise_atrous_var_async).
//
// rt_aov_kernel<BVH, CSG, VM>: one lane per pixel of the band, 256-thread
// workgroups, lanes past the band's last pixel gone before any ballot (as in
// rt_query_kernel). A lane loops over the camera's S samples (wave-uniform):
// the sample's ray (cam_ray, rt_camera.hip: the ray the camera render traces),
// the shared search in closest mode (SceneSearch, rt_query.hip), surface_props,
// the material colour -- a closure surface's through run_vm on the (face, u,
// v) the radiance kernel forms (rt_trace.hip; keep the two in step) -- and
// eight accumulators plus the hit count held in registers across the loop.
// Only the first ray of each sample's tree is traced: no lighting, no
// children, no frame stack, no sample buffer, no chunks, and nothing the
// context owns. No shared state but the wave's BVH stack, no atomics and no
// waiting: the kernel cannot hang.
//
// dn_atrous_kernel: one thread per pixel and iteration of the filter, plain
// cached global loads, wave-uniform 5 x 5 tap loop with the weights in
// constant memory; launched once per iteration on the caller's stream, the
// host never waits. dn_atrous_tile_kernel<STEP>: the iterations with step 1
// and 2 read their taps from an LDS tile with a halo instead (same bits).
// dn_atrous_var_kernel, dn_atrous_var_tile_kernel<STEP>: the same pair for the
// variance-guided filter, which also reads and writes a scalar variance per
// pixel; dn_var_reduce_kernel forms its first value. All of them write only
// their own pixel and wait for nothing.
// Included by rt_kernel.hip after rt_camera.hip (cam_ray, CamArgs, cam_setup,
// pack_rgba8).

namespace {

struct AovArgs : SceneRef {
  int off_mats, off_code, off_consts, off_entry;
  int npix;  // pixels of the band
  CamArgs cam;
  double inv;  // 1.0 / (double)S
  double* depth;
  double* normal;
  double* albedo;
  double* coverage;
  int32_t* ids;
};

template <bool BVH, bool CSG, bool VM>
__global__ __launch_bounds__(WG) void rt_aov_kernel(const char* __restrict__ blob, AovArgs Q) {
  __shared__ uint64_t s_mask[BVH ? WAVES_PER_WG * BVH_STACK : 1];
  __shared__ int s_ref[BVH ? WAVES_PER_WG * BVH_STACK : 1];
  const int gid = (int)(blockIdx.x * WG + threadIdx.x);
  if (gid >= Q.npix) return;  // lanes past npix: inactive from here on, in no ballot

  auto search = scene_search<BVH, CSG>(blob, Q, s_mask, s_ref);
  const double* v_mats = reinterpret_cast<const double*>(blob + Q.off_mats);
  const int pixel = Q.cam.first + gid;

  double zt = 0.0;
  d3 N = mk(0.0, 0.0, 0.0), A = mk(0.0, 0.0, 0.0);
  int h = 0;
  Q16i id = {-1, 0, 0, 0};  // sample 0's object, face, kind, material
  for (int s = 0; s < Q.cam.S; s++) {
    Ray ray;
    cam_ray(Q.cam, pixel, s, ray.o, ray.d);
    bool found;
    double hit_t;
    int hit_i, hit_f;
    search(ray, true, __builtin_inf(), -1, BoolC<false>(), BoolC<false>(), 1.0, 0.0, found, hit_t, hit_i, hit_f);
    if (!found) continue;
    int si, sf, k, mat;
    d3 p, pw, nw;
    surface_props<CSG>(blob, Q, ray, hit_i, hit_f, hit_t, si, sf, k, p, pw, nw, mat);
    d3 a = mk(0.0, 0.0, 0.0);
    if (mat >= 0) {
      const double* M = v_mats + (size_t)mat * MAT;
      a = mk(M[0], M[1], M[2]);
    } else {
      if constexpr (VM) {
        // Closure surface: (face, u, v) and the VM call of rt_trace.hip
        // (raytracer.go:124-150, 196-205, 249, 339-359)
        double vr[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        double u, v;
        bool bad = false;
        const long long face = (k == RT_PLANE) ? 0 : sf;
        if (k == RT_SPHERE) {
          bad = __builtin_fabs(p.y) > 1;
          v = (p.y + 1.0) / 2.0;
          u = go_acos(p.z / __builtin_sqrt(1.0 - p.y * p.y)) / 6.283185307179586;
        } else if ((k == RT_CYLINDER || k == RT_CONE) && sf == 0) {
          u = (go_atan2(p.x, p.z) + 3.141592653589793) / 6.283185307179586;
          v = p.y;
        } else {
          u = p.x;
          v = p.z;
        }
        bad = run_vm<true>(reinterpret_cast<const uint32_t*>(blob + Q.off_code),
                           reinterpret_cast<const uint64_t*>(blob + Q.off_consts),
                           reinterpret_cast<const int*>(blob + Q.off_entry)[-mat - 1], face, u, v, vr) ||
              bad;
        if (!bad) a = mk(vr[0], vr[1], vr[2]);  // a failing evaluation: the all-zero material
      }
    }
    const d3 nh = norm(nw);
    zt = zt + hit_t;
    N = add(N, nh);
    A = add(A, a);
    h++;
    if (s == 0) {
      const Q16i i0 = {hit_i, hit_f, k, mat};
      id = i0;
    }
  }

  const double inv = Q.inv;
  if (Q.depth) Q.depth[gid] = h > 0 ? zt / (double)h : __builtin_inf();
  if (Q.normal) {
    double* o = Q.normal + (size_t)gid * 3;
    o[0] = N.x * inv;
    o[1] = N.y * inv;
    o[2] = N.z * inv;
  }
  if (Q.albedo) {
    double* o = Q.albedo + (size_t)gid * 3;
    o[0] = A.x * inv;
    o[1] = A.y * inv;
    o[2] = A.z * inv;
  }
  if (Q.coverage) Q.coverage[gid] = (double)h * inv;
  if (Q.ids) reinterpret_cast<Q16i*>(Q.ids)[gid] = id;
}

// [BVH | CSG << 1 | VM << 2], as k_trace_kernels
const void* const k_aov_kernels[8] = {
    (const void*)rt_aov_kernel<false, false, false>, (const void*)rt_aov_kernel<true, false, false>,
    (const void*)rt_aov_kernel<false, true, false>,  (const void*)rt_aov_kernel<true, true, false>,
    (const void*)rt_aov_kernel<false, false, true>,  (const void*)rt_aov_kernel<true, false, true>,
    (const void*)rt_aov_kernel<false, true, true>,   (const void*)rt_aov_kernel<true, true, true>};

// ---- the a-trous filter ----

enum { DN_COLOR = 1, DN_NORMAL = 2, DN_DEPTH = 4, DN_ALBEDO = 8 };

struct DnArgs {
  int W, H, step, on;     // on: DN_* bits of the terms that are on
  double ic, in, iz, ia;  // 1 / sigma^2 of the colour (this iteration's), normal, depth and albedo terms
  const double* src;      // I_i
  const double* normal;
  const double* depth;
  const double* albedo;
  double* dst;     // I_(i+1)
  uint32_t* rgba;  // the last iteration's, or NULL
};

// h[j] * h[i] of the taps h = (1/16, 1/4, 3/8, 1/4, 1/16): exact
struct DnTaps {
  double w[25];
};
constexpr DnTaps dn_taps() {
  const double h[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
  DnTaps t = {};
  for (int j = 0; j < 5; j++)
    for (int i = 0; i < 5; i++) t.w[j * 5 + i] = h[j] * h[i];
  return t;
}
__constant__ const DnTaps k_dn_taps = dn_taps();

__device__ __forceinline__ double dn_kern(double x) {
  if (x < 1.0) {  // (false for NaN)
    const double m = 1.0 - x;
    return m * m;
  }
  return 0.0;
}

__device__ __forceinline__ double dn_dist2(const d3& a, const d3& b) {
  const double d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z;
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

__device__ __forceinline__ d3 dn_load3(const double* b, long long q) { return mk(b[q * 3], b[q * 3 + 1], b[q * 3 + 2]); }

__global__ __launch_bounds__(WG) void dn_atrous_kernel(DnArgs A) {
  const long long p = (long long)blockIdx.x * WG + threadIdx.x;
  if (p >= (long long)A.W * A.H) return;
  const int y = (int)(p / A.W), x = (int)(p - (long long)y * A.W);
  const d3 cp = dn_load3(A.src, p);
  d3 np = mk(0, 0, 0), ap = mk(0, 0, 0);
  double zp = 0.0;
  if (A.on & DN_NORMAL) np = dn_load3(A.normal, p);
  if (A.on & DN_DEPTH) zp = A.depth[p];
  if (A.on & DN_ALBEDO) ap = dn_load3(A.albedo, p);
  d3 sum = mk(0.0, 0.0, 0.0);
  double wsum = 0.0;
  for (int dy = -2; dy <= 2; dy++) {
    const long long qy = (long long)y + (long long)dy * A.step;
    for (int dx = -2; dx <= 2; dx++) {
      const long long qx = (long long)x + (long long)dx * A.step;
      if (qx < 0 || qx >= A.W || qy < 0 || qy >= A.H) continue;
      const long long q = qy * A.W + qx;
      double w = k_dn_taps.w[(dy + 2) * 5 + (dx + 2)];
      const d3 cq = dn_load3(A.src, q);
      if (A.on & DN_COLOR) w = w * dn_kern(dn_dist2(cp, cq) * A.ic);
      if (A.on & DN_NORMAL) w = w * dn_kern(dn_dist2(np, dn_load3(A.normal, q)) * A.in);
      if (A.on & DN_DEPTH) {
        const double zq = A.depth[q];
        const double dz = zp - zq;
        w = w * dn_kern((zp == zq ? 0.0 : dz * dz) * A.iz);
      }
      if (A.on & DN_ALBEDO) w = w * dn_kern(dn_dist2(ap, dn_load3(A.albedo, q)) * A.ia);
      if (w > 0.0) {
        sum = mk(sum.x + w * cq.x, sum.y + w * cq.y, sum.z + w * cq.z);
        wsum = wsum + w;
      }
    }
  }
  d3 r = cp;
  if (wsum > 0.0) r = mk(sum.x / wsum, sum.y / wsum, sum.z / wsum);
  A.dst[p * 3] = r.x;
  A.dst[p * 3 + 1] = r.y;
  A.dst[p * 3 + 2] = r.z;
  if (A.rgba) A.rgba[p] = pack_rgba8(r);
}

// The same iteration for STEP 1 and 2 from an LDS tile with a halo: a
// workgroup covers DN_BX x DN_BY pixels and first copies their 5 x 5 x STEP
// neighbourhood, (DN_BX + 4 STEP) x (DN_BY + 4 STEP) pixels of the colour and
// of the guides that are on, into LDS (one array per component: consecutive
// lanes read consecutive doubles). The taps then read LDS in dn_atrous_kernel's
// order with its arithmetic, so the two kernels give the same bits. One
// barrier, before any thread leaves.
constexpr int DN_BX = 32, DN_BY = 8;
static_assert(DN_BX * DN_BY == WG, "one thread per pixel of the tile");

template <int STEP>
__global__ __launch_bounds__(WG) void dn_atrous_tile_kernel(DnArgs A) {
  constexpr int TW = DN_BX + 4 * STEP, TH = DN_BY + 4 * STEP, TN = TW * TH;
  __shared__ double s_c[3][TN], s_n[3][TN], s_a[3][TN], s_z[TN];
  const int bx0 = (int)blockIdx.x * DN_BX, by0 = (int)blockIdx.y * DN_BY;
  for (int t = (int)threadIdx.x; t < TN; t += WG) {
    const int ty = t / TW, tx = t - ty * TW;
    const int gx = bx0 - 2 * STEP + tx, gy = by0 - 2 * STEP + ty;
    if (gx < 0 || gx >= A.W || gy < 0 || gy >= A.H) continue;  // (never read: the taps skip it too)
    const long long q = (long long)gy * A.W + gx;
    const d3 c = dn_load3(A.src, q);
    s_c[0][t] = c.x;
    s_c[1][t] = c.y;
    s_c[2][t] = c.z;
    if (A.on & DN_NORMAL) {
      const d3 n = dn_load3(A.normal, q);
      s_n[0][t] = n.x;
      s_n[1][t] = n.y;
      s_n[2][t] = n.z;
    }
    if (A.on & DN_DEPTH) s_z[t] = A.depth[q];
    if (A.on & DN_ALBEDO) {
      const d3 a = dn_load3(A.albedo, q);
      s_a[0][t] = a.x;
      s_a[1][t] = a.y;
      s_a[2][t] = a.z;
    }
  }
  __syncthreads();
  const int lx = (int)threadIdx.x % DN_BX, ly = (int)threadIdx.x / DN_BX;
  const int x = bx0 + lx, y = by0 + ly;
  if (x >= A.W || y >= A.H) return;
  const int tc = (ly + 2 * STEP) * TW + lx + 2 * STEP;
  const d3 cp = mk(s_c[0][tc], s_c[1][tc], s_c[2][tc]);
  d3 np = mk(0, 0, 0), ap = mk(0, 0, 0);
  double zp = 0.0;
  if (A.on & DN_NORMAL) np = mk(s_n[0][tc], s_n[1][tc], s_n[2][tc]);
  if (A.on & DN_DEPTH) zp = s_z[tc];
  if (A.on & DN_ALBEDO) ap = mk(s_a[0][tc], s_a[1][tc], s_a[2][tc]);
  d3 sum = mk(0.0, 0.0, 0.0);
  double wsum = 0.0;
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + dy * STEP;
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + dx * STEP;
      if (qx < 0 || qx >= A.W || qy < 0 || qy >= A.H) continue;
      const int t = tc + dy * STEP * TW + dx * STEP;
      double w = k_dn_taps.w[(dy + 2) * 5 + (dx + 2)];
      const d3 cq = mk(s_c[0][t], s_c[1][t], s_c[2][t]);
      if (A.on & DN_COLOR) w = w * dn_kern(dn_dist2(cp, cq) * A.ic);
      if (A.on & DN_NORMAL) w = w * dn_kern(dn_dist2(np, mk(s_n[0][t], s_n[1][t], s_n[2][t])) * A.in);
      if (A.on & DN_DEPTH) {
        const double zq = s_z[t];
        const double dz = zp - zq;
        w = w * dn_kern((zp == zq ? 0.0 : dz * dz) * A.iz);
      }
      if (A.on & DN_ALBEDO) w = w * dn_kern(dn_dist2(ap, mk(s_a[0][t], s_a[1][t], s_a[2][t])) * A.ia);
      if (w > 0.0) {
        sum = mk(sum.x + w * cq.x, sum.y + w * cq.y, sum.z + w * cq.z);
        wsum = wsum + w;
      }
    }
  }
  d3 r = cp;
  if (wsum > 0.0) r = mk(sum.x / wsum, sum.y / wsum, sum.z / wsum);
  const long long p = (long long)y * A.W + x;
  A.dst[p * 3] = r.x;
  A.dst[p * 3 + 1] = r.y;
  A.dst[p * 3 + 2] = r.z;
  if (A.rgba) A.rgba[p] = pack_rgba8(r);
}

// ---- the variance-guided filter (include/rt_abi.h "Variance-guided a-trous filter") ----
// The kernels above with the colour term scaled by the locally prefiltered
// variance and a scalar variance S_i propagated beside the colour: siblings of
// dn_atrous_kernel and dn_atrous_tile_kernel, which stay the code objects they
// were.

struct DnVarArgs : DnArgs {
  double kc2;          // sigma_color^2 (in standard deviations)
  const double* vsrc;  // S_i, one double per pixel
  double* vdst;        // S_(i+1)
};

// S_0: the channels' variances added
__global__ __launch_bounds__(WG) void dn_var_reduce_kernel(const double* __restrict__ var, double* __restrict__ dst,
                                                            long long n) {
  const long long p = (long long)blockIdx.x * WG + threadIdx.x;
  if (p >= n) return;
  dst[p] = (var[p * 3] + var[p * 3 + 1]) + var[p * 3 + 2];
}

// k[j] * k[i] of the prefilter's taps k = (1/4, 1/2, 1/4): exact
__device__ __forceinline__ double dn_pre_tap(int dy, int dx) { return (dy == 0 ? 0.5 : 0.25) * (dx == 0 ? 0.5 : 0.25); }

__global__ __launch_bounds__(WG) void dn_atrous_var_kernel(DnVarArgs A) {
  const long long p = (long long)blockIdx.x * WG + threadIdx.x;
  if (p >= (long long)A.W * A.H) return;
  const int y = (int)(p / A.W), x = (int)(p - (long long)y * A.W);
  const d3 cp = dn_load3(A.src, p);
  d3 np = mk(0, 0, 0), ap = mk(0, 0, 0);
  double zp = 0.0, icv = 0.0;
  if (A.on & DN_NORMAL) np = dn_load3(A.normal, p);
  if (A.on & DN_DEPTH) zp = A.depth[p];
  if (A.on & DN_ALBEDO) ap = dn_load3(A.albedo, p);
  if (A.on & DN_COLOR) {
    double N = 0.0, D = 0.0;
    for (int dy = -1; dy <= 1; dy++) {
      const int qy = y + dy;
      for (int dx = -1; dx <= 1; dx++) {
        const int qx = x + dx;
        if (qx < 0 || qx >= A.W || qy < 0 || qy >= A.H) continue;
        const double k = dn_pre_tap(dy, dx);
        N = N + k * A.vsrc[(long long)qy * A.W + qx];
        D = D + k;
      }
    }
    const double g = N / D;
    icv = 1.0 / (A.kc2 * g + RT_DENOISE_VAR_EPS);
  }
  d3 sum = mk(0.0, 0.0, 0.0);
  double wsum = 0.0, vs = 0.0;
  for (int dy = -2; dy <= 2; dy++) {
    const long long qy = (long long)y + (long long)dy * A.step;
    for (int dx = -2; dx <= 2; dx++) {
      const long long qx = (long long)x + (long long)dx * A.step;
      if (qx < 0 || qx >= A.W || qy < 0 || qy >= A.H) continue;
      const long long q = qy * A.W + qx;
      double w = k_dn_taps.w[(dy + 2) * 5 + (dx + 2)];
      const d3 cq = dn_load3(A.src, q);
      if (A.on & DN_COLOR) w = w * dn_kern(dn_dist2(cp, cq) * icv);
      if (A.on & DN_NORMAL) w = w * dn_kern(dn_dist2(np, dn_load3(A.normal, q)) * A.in);
      if (A.on & DN_DEPTH) {
        const double zq = A.depth[q];
        const double dz = zp - zq;
        w = w * dn_kern((zp == zq ? 0.0 : dz * dz) * A.iz);
      }
      if (A.on & DN_ALBEDO) w = w * dn_kern(dn_dist2(ap, dn_load3(A.albedo, q)) * A.ia);
      if (w > 0.0) {
        sum = mk(sum.x + w * cq.x, sum.y + w * cq.y, sum.z + w * cq.z);
        wsum = wsum + w;
        vs = vs + (w * w) * A.vsrc[q];
      }
    }
  }
  d3 r = cp;
  double sv = A.vsrc[p];
  if (wsum > 0.0) {
    r = mk(sum.x / wsum, sum.y / wsum, sum.z / wsum);
    sv = vs / (wsum * wsum);
  }
  A.dst[p * 3] = r.x;
  A.dst[p * 3 + 1] = r.y;
  A.dst[p * 3 + 2] = r.z;
  A.vdst[p] = sv;
  if (A.rgba) A.rgba[p] = pack_rgba8(r);
}

// ... for STEP 1 and 2 from the LDS tile of dn_atrous_tile_kernel plus one
// array, S_i, whose halo (2 STEP >= 2 pixels) covers the prefilter's 3 x 3.
// <2>: 11 arrays of 640 doubles, 56 320 bytes.
template <int STEP>
__global__ __launch_bounds__(WG) void dn_atrous_var_tile_kernel(DnVarArgs A) {
  constexpr int TW = DN_BX + 4 * STEP, TH = DN_BY + 4 * STEP, TN = TW * TH;
  __shared__ double s_c[3][TN], s_n[3][TN], s_a[3][TN], s_z[TN], s_v[TN];
  const int bx0 = (int)blockIdx.x * DN_BX, by0 = (int)blockIdx.y * DN_BY;
  for (int t = (int)threadIdx.x; t < TN; t += WG) {
    const int ty = t / TW, tx = t - ty * TW;
    const int gx = bx0 - 2 * STEP + tx, gy = by0 - 2 * STEP + ty;
    if (gx < 0 || gx >= A.W || gy < 0 || gy >= A.H) continue;  // (never read: the taps skip it too)
    const long long q = (long long)gy * A.W + gx;
    const d3 c = dn_load3(A.src, q);
    s_c[0][t] = c.x;
    s_c[1][t] = c.y;
    s_c[2][t] = c.z;
    s_v[t] = A.vsrc[q];
    if (A.on & DN_NORMAL) {
      const d3 n = dn_load3(A.normal, q);
      s_n[0][t] = n.x;
      s_n[1][t] = n.y;
      s_n[2][t] = n.z;
    }
    if (A.on & DN_DEPTH) s_z[t] = A.depth[q];
    if (A.on & DN_ALBEDO) {
      const d3 a = dn_load3(A.albedo, q);
      s_a[0][t] = a.x;
      s_a[1][t] = a.y;
      s_a[2][t] = a.z;
    }
  }
  __syncthreads();
  const int lx = (int)threadIdx.x % DN_BX, ly = (int)threadIdx.x / DN_BX;
  const int x = bx0 + lx, y = by0 + ly;
  if (x >= A.W || y >= A.H) return;
  const int tc = (ly + 2 * STEP) * TW + lx + 2 * STEP;
  const d3 cp = mk(s_c[0][tc], s_c[1][tc], s_c[2][tc]);
  d3 np = mk(0, 0, 0), ap = mk(0, 0, 0);
  double zp = 0.0, icv = 0.0;
  if (A.on & DN_NORMAL) np = mk(s_n[0][tc], s_n[1][tc], s_n[2][tc]);
  if (A.on & DN_DEPTH) zp = s_z[tc];
  if (A.on & DN_ALBEDO) ap = mk(s_a[0][tc], s_a[1][tc], s_a[2][tc]);
  if (A.on & DN_COLOR) {
    double N = 0.0, D = 0.0;
    for (int dy = -1; dy <= 1; dy++) {
      const int qy = y + dy;
      for (int dx = -1; dx <= 1; dx++) {
        const int qx = x + dx;
        if (qx < 0 || qx >= A.W || qy < 0 || qy >= A.H) continue;
        const double k = dn_pre_tap(dy, dx);
        N = N + k * s_v[tc + dy * TW + dx];
        D = D + k;
      }
    }
    const double g = N / D;
    icv = 1.0 / (A.kc2 * g + RT_DENOISE_VAR_EPS);
  }
  d3 sum = mk(0.0, 0.0, 0.0);
  double wsum = 0.0, vs = 0.0;
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + dy * STEP;
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + dx * STEP;
      if (qx < 0 || qx >= A.W || qy < 0 || qy >= A.H) continue;
      const int t = tc + dy * STEP * TW + dx * STEP;
      double w = k_dn_taps.w[(dy + 2) * 5 + (dx + 2)];
      const d3 cq = mk(s_c[0][t], s_c[1][t], s_c[2][t]);
      if (A.on & DN_COLOR) w = w * dn_kern(dn_dist2(cp, cq) * icv);
      if (A.on & DN_NORMAL) w = w * dn_kern(dn_dist2(np, mk(s_n[0][t], s_n[1][t], s_n[2][t])) * A.in);
      if (A.on & DN_DEPTH) {
        const double zq = s_z[t];
        const double dz = zp - zq;
        w = w * dn_kern((zp == zq ? 0.0 : dz * dz) * A.iz);
      }
      if (A.on & DN_ALBEDO) w = w * dn_kern(dn_dist2(ap, mk(s_a[0][t], s_a[1][t], s_a[2][t])) * A.ia);
      if (w > 0.0) {
        sum = mk(sum.x + w * cq.x, sum.y + w * cq.y, sum.z + w * cq.z);
        wsum = wsum + w;
        vs = vs + (w * w) * s_v[t];
      }
    }
  }
  d3 r = cp;
  double sv = s_v[tc];
  if (wsum > 0.0) {
    r = mk(sum.x / wsum, sum.y / wsum, sum.z / wsum);
    sv = vs / (wsum * wsum);
  }
  const long long p = (long long)y * A.W + x;
  A.dst[p * 3] = r.x;
  A.dst[p * 3 + 1] = r.y;
  A.dst[p * 3 + 2] = r.z;
  A.vdst[p] = sv;
  if (A.rgba) A.rgba[p] = pack_rgba8(r);
}

// A sigma of rt_denoise: > 0 and finite: on; 0 or +inf: off; else invalid
bool dn_sigma(double s, bool& on) {
  on = s > 0.0 && std::isfinite(s);
  return s >= 0.0;  // (false for NaN)
}

bool dn_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

// ... of buffers of different sizes
bool dn_overlap2(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// What rt_denoise_atrous_async and rt_denoise_atrous_var_async check alike, in
// the header's order; fills K and the part of `A` that no iteration changes.
int dn_setup(rt_context* c, const rt_denoise* dn, int width, int height, const double* d_color, const double* d_normal,
             const double* d_depth, const double* d_albedo, double* d_out, double* d_tmp, void* d_rgba,
             const std::string& w, int& K, DnArgs& A) {
  if (!c) return fail(RT_E_INVALID, w + "NULL context");
  if (!dn) return fail(RT_E_INVALID, w + "NULL rt_denoise");
  if (dn->reserved != 0) return fail(RT_E_INVALID, w + "rt_denoise.reserved must be 0");
  if (dn->iterations < 0 || dn->iterations > 8) return fail(RT_E_INVALID, w + "iterations outside [0, 8]");
  K = dn->iterations == 0 ? 5 : dn->iterations;
  bool onc, onn, onz, ona;
  if (!dn_sigma(dn->sigma_color, onc) || !dn_sigma(dn->sigma_normal, onn) || !dn_sigma(dn->sigma_depth, onz) ||
      !dn_sigma(dn->sigma_albedo, ona))
    return fail(RT_E_INVALID, w + "a sigma is negative or NaN");
  if (width < 1 || height < 1 || (long long)width * height > 2147483647LL)
    return fail(RT_E_INVALID, w + "width and height must be >= 1 and the frame at most 2^31 - 1 pixels");
  if (!d_color || !d_out) return fail(RT_E_INVALID, w + "NULL d_color or d_out");
  if (!d_tmp && K > 1) return fail(RT_E_INVALID, w + "d_tmp may be NULL only when there is one iteration");
  if ((onn && !d_normal) || (onz && !d_depth) || (ona && !d_albedo))
    return fail(RT_E_INVALID, w + "a guide may be NULL only when its term is off");
  if ((((uintptr_t)d_color | (uintptr_t)d_normal | (uintptr_t)d_depth | (uintptr_t)d_albedo | (uintptr_t)d_out |
        (uintptr_t)d_tmp) & 7) != 0)
    return fail(RT_E_INVALID, w + "the float64 buffers must be 8-byte aligned");
  if (((uintptr_t)d_rgba & 3) != 0) return fail(RT_E_INVALID, w + "d_rgba must be 4-byte aligned");
  const size_t bytes = (size_t)width * height * 3 * sizeof(double);
  if (dn_overlap(d_color, d_out, bytes) || (d_tmp && (dn_overlap(d_color, d_tmp, bytes) || dn_overlap(d_out, d_tmp, bytes))))
    return fail(RT_E_INVALID, w + "d_color, d_out and d_tmp must not overlap");
  std::memset(&A, 0, sizeof A);
  A.W = width;
  A.H = height;
  A.on = (onc ? DN_COLOR : 0) | (onn ? DN_NORMAL : 0) | (onz ? DN_DEPTH : 0) | (ona ? DN_ALBEDO : 0);
  if (onn) A.in = 1.0 / (dn->sigma_normal * dn->sigma_normal);
  if (onz) A.iz = 1.0 / (dn->sigma_depth * dn->sigma_depth);
  if (ona) A.ia = 1.0 / (dn->sigma_albedo * dn->sigma_albedo);
  A.normal = d_normal;
  A.depth = d_depth;
  A.albedo = d_albedo;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_render_camera_aov_async(rt_context* c, const rt_camera* cam, int y0, int y1, const rt_aov_out* out,
                               void* stream) {
  const char* who = "rt_render_camera_aov_async";
  CamPlan P;
  if (int rc = cam_setup(c, cam, y0, y1, who, P); rc != RT_OK) return rc;
  const std::string w = std::string(who) + ": ";
  if (!out) return fail(RT_E_INVALID, w + "NULL rt_aov_out");
  if (!out->depth && !out->normal && !out->albedo && !out->coverage && !out->ids)
    return fail(RT_E_INVALID, w + "all five output pointers are NULL");
  if ((((uintptr_t)out->depth | (uintptr_t)out->normal | (uintptr_t)out->albedo | (uintptr_t)out->coverage) & 7) != 0)
    return fail(RT_E_INVALID, w + "depth, normal, albedo and coverage must be 8-byte aligned");
  if (((uintptr_t)out->ids & 15) != 0) return fail(RT_E_INVALID, w + "ids must be 16-byte aligned");
  const DevScene& s = c->sc;
  DeviceGuard guard(c->device);
  AovArgs Q;
  std::memset(&Q, 0, sizeof Q);
  scene_ref(c, Q);
  Q.off_mats = s.off_mats;
  Q.off_code = s.off_code;
  Q.off_consts = s.off_consts;
  Q.off_entry = s.off_entry;
  Q.npix = (int)P.pixels;  // (a frame has at most 2^31 - 1 pixels: cam_setup)
  Q.cam = P.A;
  Q.inv = 1.0 / (double)P.A.S;
  Q.depth = out->depth;
  Q.normal = out->normal;
  Q.albedo = out->albedo;
  Q.coverage = out->coverage;
  Q.ids = out->ids;
  const char* blob = s.blob;
  void* args[] = {(void*)&blob, (void*)&Q};
  HIP_TRY(hipLaunchKernel(k_aov_kernels[flavour(s)], dim3((unsigned)((P.pixels + WG - 1) / WG)), dim3(WG), args, 0,
                          (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int rt_denoise_atrous_async(rt_context* c, const rt_denoise* dn, int width, int height, const double* d_color,
                            const double* d_normal, const double* d_depth, const double* d_albedo, double* d_out,
                            double* d_tmp, void* d_rgba, void* stream) {
  int K;
  DnArgs A;
  if (int rc = dn_setup(c, dn, width, height, d_color, d_normal, d_depth, d_albedo, d_out, d_tmp, d_rgba,
                        "rt_denoise_atrous_async: ", K, A);
      rc != RT_OK)
    return rc;
  const bool onc = (A.on & DN_COLOR) != 0;
  DeviceGuard guard(c->device);
  const long long blocks = ((long long)width * height + WG - 1) / WG;
  const double* src = d_color;
  double half = 1.0;  // 0.5^i
  for (int i = 0; i < K; i++) {
    A.step = 1 << i;
    if (onc) {
      const double sg = dn->sigma_color * half;
      A.ic = 1.0 / (sg * sg);
    }
    A.src = src;
    A.dst = ((K - 1 - i) % 2 == 0) ? d_out : d_tmp;
    A.rgba = i == K - 1 ? (uint32_t*)d_rgba : nullptr;
    void* args[] = {(void*)&A};
    // steps 1 and 2 from an LDS tile (measured faster: DESIGN.md "Feature buffers and the a-trous filter");
    // wider steps, and frames too tall for a grid's y extent, through global loads
    const unsigned gx = (unsigned)((width + DN_BX - 1) / DN_BX), gy = (unsigned)((height + DN_BY - 1) / DN_BY);
    if (i < 2 && gy <= 65535u)
      HIP_TRY(hipLaunchKernel(i == 0 ? (const void*)dn_atrous_tile_kernel<1> : (const void*)dn_atrous_tile_kernel<2>,
                              dim3(gx, gy), dim3(WG), args, 0, (hipStream_t)stream));
    else
      HIP_TRY(hipLaunchKernel((const void*)dn_atrous_kernel, dim3((unsigned)blocks), dim3(WG), args, 0,
                              (hipStream_t)stream));
    src = A.dst;
    half = half * 0.5;
  }
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int rt_denoise_atrous_var_async(rt_context* c, const rt_denoise* dn, int width, int height, const double* d_color,
                                const double* d_var, const double* d_normal, const double* d_depth,
                                const double* d_albedo, double* d_out, double* d_tmp, double* d_var_out,
                                double* d_var_tmp, void* d_rgba, void* stream) {
  const std::string w = "rt_denoise_atrous_var_async: ";
  int K;
  DnVarArgs A;
  if (int rc = dn_setup(c, dn, width, height, d_color, d_normal, d_depth, d_albedo, d_out, d_tmp, d_rgba, w, K, A);
      rc != RT_OK)
    return rc;
  if (!d_var || !d_var_out || !d_var_tmp) return fail(RT_E_INVALID, w + "NULL d_var, d_var_out or d_var_tmp");
  if ((((uintptr_t)d_var | (uintptr_t)d_var_out | (uintptr_t)d_var_tmp) & 7) != 0)
    return fail(RT_E_INVALID, w + "d_var, d_var_out and d_var_tmp must be 8-byte aligned");
  const long long npix = (long long)width * height;
  const size_t b1 = (size_t)npix * sizeof(double), b3 = 3 * b1;
  const void* buf[6] = {d_color, d_var, d_out, d_tmp, d_var_out, d_var_tmp};
  const size_t len[6] = {b3, b3, b3, b3, b1, b1};
  for (int i = 0; i < 6; i++)
    for (int j = i + 1; j < 6; j++)
      if (buf[i] && buf[j] && dn_overlap2(buf[i], len[i], buf[j], len[j]))
        return fail(RT_E_INVALID, w + "d_color, d_var, d_out, d_tmp, d_var_out and d_var_tmp must not overlap");
  DeviceGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  A.kc2 = dn->sigma_color * dn->sigma_color;
  A.vsrc = nullptr;
  A.vdst = nullptr;
  const long long blocks = (npix + WG - 1) / WG;
  // S_i lives in d_var_out when K - i is even, else in d_var_tmp: S_K ends in d_var_out
  double* s0 = K % 2 == 0 ? d_var_out : d_var_tmp;
  {
    long long n = npix;
    void* args[] = {(void*)&d_var, (void*)&s0, (void*)&n};
    HIP_TRY(hipLaunchKernel((const void*)dn_var_reduce_kernel, dim3((unsigned)blocks), dim3(WG), args, 0, st));
  }
  const double* src = d_color;
  for (int i = 0; i < K; i++) {
    A.step = 1 << i;
    A.src = src;
    A.dst = ((K - 1 - i) % 2 == 0) ? d_out : d_tmp;
    A.vsrc = ((K - i) % 2 == 0) ? d_var_out : d_var_tmp;
    A.vdst = ((K - 1 - i) % 2 == 0) ? d_var_out : d_var_tmp;
    A.rgba = i == K - 1 ? (uint32_t*)d_rgba : nullptr;
    void* args[] = {(void*)&A};
    // the split of rt_denoise_atrous_async, for its reason
    const unsigned gx = (unsigned)((width + DN_BX - 1) / DN_BX), gy = (unsigned)((height + DN_BY - 1) / DN_BY);
    if (i < 2 && gy <= 65535u)
      HIP_TRY(hipLaunchKernel(i == 0 ? (const void*)dn_atrous_var_tile_kernel<1> : (const void*)dn_atrous_var_tile_kernel<2>,
                              dim3(gx, gy), dim3(WG), args, 0, st));
    else
      HIP_TRY(hipLaunchKernel((const void*)dn_atrous_var_kernel, dim3((unsigned)blocks), dim3(WG), args, 0, st));
    src = A.dst;
  }
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // extern "C"
