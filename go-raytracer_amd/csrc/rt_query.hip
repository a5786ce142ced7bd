// rt_query.hip -- batched ray queries against the scene of rt_set_scene
// (include/rt_abi.h rt_query_closest_async / rt_query_occluded_async).
//
// A kernel of its own beside rt_render_kernel, which it does not touch: one
// ray per lane, 256-thread workgroups, no persistent queue. It replaces, for
// arbitrary world-space rays,
//   raytracer.go:469-483  closestHit (index order, strict <, first index wins)
//   raytracer.go:411-429  inShadow's loop (any object but `exclude` with T < bound)
//   raytracer.go:106-122, 182-194, 242-260, 339-370  ComputeSurfaceProps
// with the exact tests of rt_render.h called unchanged (object_hit, csg_hit),
// so a query returns the values a render works with, bit for bit.
//
// The object loop is wave-uniform as in the megakernel's TRACE pass: the
// object's index, kind and record are read with scalar loads from the device
// blob (no scene copy in LDS), the ray is per lane. The BVH flavour walks the
// planes-and-composites list first and then the wave-shared stack (the only
// LDS: WAVES_PER_WG * BVH_STACK * 12 bytes).
//
// Ray directions are used as given (t is in units of |dir|), while the FP32
// culls of rt_render.h are written for unit directions (may_hit_s projects
// onto d). The culls here therefore get the direction scaled to unit length
// and bounds scaled by |dir|: bound = (float)((lim - t0) * |dir|) * 1.0001f +
// 1e-4f, the megakernel's form, where lim is the lane's best t so far or its
// tmax. A lane whose direction length or origin is not a usable FP32 number
// (zero, denormal, huge, NaN) passes every cull. csg_hit's own leaf and group
// culls take the ray's direction directly: a wave whose active lanes all hold
// unit directions (|d|^2 within 1e-9 of 1, as every normalised FP64 vector)
// calls it; any other wave takes csg_search_nocull below, the same search
// over every leaf's interval (the culls only skip leaves that change nothing,
// so both give the same bits).
//
// Shared with the radiance kernel (rt_trace.hip) and the camera renders
// (rt_camera.hip), each defined here once: scene_ref (fills the scene's part of
// an argument record: SceneRef's fields), SceneSearch (the search above,
// closest and any-hit), ray_load / ray_store (the 64-byte ray record) and
// flavour (the index into a kernel table). surface_props (ComputeSurfaceProps
// of a winner) is called by the query kernel only: the radiance kernel keeps
// the same lines written out, because the call costs it 40 VGPRs and a wave
// per SIMD in one instantiation (DESIGN.md "Shared pieces of the query,
// radiance and camera kernels"). The query kernel's mode is a template flag:
// closest and occluded are instantiations of their own.
// Included by rt_kernel.hip (shares rt_context, DevScene and the error plumbing).

namespace {

// What a kernel needs to find the scene of a context (wave-uniform), filled by
// scene_ref: the base of QueryArgs; TraceArgs (rt_trace.hip) carries the same
// fields in an order of its own, for the reason given there.
struct SceneRef {
  int nobj;
  int cull;  // RT_ACCEL_CULL: the FP32 culls of the object lists
  int off_geo, off_shade, off_kind, off_objmat, off_csg;
  // BVH flavour (DevScene::use_bvh)
  const float* bvh_nodes;
  const double* bvh_geo;
  const int* planes;
  int nplanes;
  double bvh_lo[3], bvh_hi[3];
};

struct QueryArgs : SceneRef {
  const rt_ray* rays;
  rt_hit* hits;       // closest mode
  uint8_t* occluded;  // occluded mode
  int n;
};

template <bool B>
struct BoolC {
  static constexpr bool value = B;
};

// csg_hit_all's search (rt_render.h) without its FP32 leaf cull: every leaf's
// interval is formed, as the oracle's csg_intersect does. For rays whose
// direction is not unit length (see the head of this file).
template <bool CL, typename DP, typename IP, typename GP>
__device__ __noinline__ bool csg_search_nocull(DP geo, IP kinds, IP code, int nobj, GP g, const Ray& r, double& t,
                                               int& face, double cut_lim, bool cut_strict) {
  const auto ci = as_i(g + 14);
  const int first = nobj + ci[0], count = ci[1];
  const auto prog = code + ci[2] + 1 + 6 * code[ci[2]];  // past the leaf groups (csg_hit)
  const int plen = ci[3];
  double A[RT_CSG_MAX_LEAVES], B[RT_CSG_MAX_LEAVES];
  int F[RT_CSG_MAX_LEAVES];
  uint64_t live0 = 0, live1 = 0;
  for (int j = 0; j < count; j++) {
    leaf_interval<CL>(kinds[first + j], geo + (size_t)(first + j) * GEO, r, A[j], B[j], F[j]);
    if (F[j] & 256) {
      if (j < 64)
        live0 |= 1ull << j;
      else
        live1 |= 1ull << (j - 64);
    }
  }
  double tc = 0.0;
  for (;;) {
    double te = __builtin_inf();
    int je = -1, jend = 0;
    for (int w = 0; w < 2; w++) {  // ascending leaf order (lowest leaf, entry first, on ties)
      uint64_t m = w ? live1 : live0;
      while (m) {
        const int j = w * 64 + __builtin_ctzll(m);
        m &= m - 1;
        if (A[j] > tc && A[j] < te) {
          te = A[j];
          je = j;
          jend = 0;
        }
        if (B[j] > tc && B[j] < te) {
          te = B[j];
          je = j;
          jend = 1;
        }
      }
    }
    if (je < 0) return false;
    if (cut_strict ? te > cut_lim : te >= cut_lim) return false;
    uint64_t b0 = 0, b1 = 0, a0 = 0, a1 = 0;
    for (int w = 0; w < 2; w++) {
      uint64_t m = w ? live1 : live0, bm = 0, am = 0;
      while (m) {
        const int q = __builtin_ctzll(m);
        m &= m - 1;
        const int j = w * 64 + q;
        if (A[j] < te && te <= B[j]) bm |= 1ull << q;
        if (A[j] <= te && te < B[j]) am |= 1ull << q;
      }
      if (w) {
        b1 = bm;
        a1 = am;
      } else {
        b0 = bm;
        a0 = am;
      }
    }
    const bool before = csg_eval(prog, plen, b0, b1), after = csg_eval(prog, plen, a0, a1);
    if (before != after) {
      const int flip = ((jend == 0) != after) ? 1 : 0;
      t = te;
      face = (je << 4) | (flip << 3) | (jend ? (F[je] >> 4) & 15 : F[je] & 15);
      return true;
    }
    tc = te;
  }
}

// 16-byte vector moves of the records (global_load / global_store_dwordx4)
struct __attribute__((aligned(16))) Q16 {
  double a, b;
};
struct __attribute__((aligned(16))) Q16i {
  int a, b, c, d;
};
struct __attribute__((aligned(16))) R16 {
  double z;
  int object, rays;
};

// An rt_ray record: four 16-byte loads of its 64 bytes ...
__device__ __forceinline__ void ray_load(const rt_ray* rec, Ray& ray, double& tmax, int& excl) {
  const Q16* rp = reinterpret_cast<const Q16*>(rec);
  const Q16 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
  ray.o = mk(r0.a, r0.b, r1.a);
  ray.d = mk(r1.b, r2.a, r2.b);
  tmax = r3.a;
  excl = __double2loint(r3.b);
}

// ... and four stores, for an exported camera ray: tmax = +Inf, exclude = -1
__device__ __forceinline__ void ray_store(rt_ray* rec, const d3& o, const d3& d) {
  Q16* rp = reinterpret_cast<Q16*>(rec);
  const Q16 r0 = {o.x, o.y}, r1 = {o.z, d.x}, r2 = {d.y, d.z};
  rp[0] = r0;
  rp[1] = r1;
  rp[2] = r2;
  const R16 r3 = {__builtin_inf(), -1, 0};
  *reinterpret_cast<R16*>(rp + 3) = r3;
}

// One search over the scene, for the query kernel and the radiance kernel
// (rt_trace.hip). Holds what is the same for every search of a wave: the scene
// references, the scalar-load pointers, the lane and the wave's stack slice.
template <bool BVH, bool CSG, typename AR>
struct SceneSearch {
  const AR& Q;  // a record with SceneRef's fields
  // scene records through scalar loads (wave-uniform indices)
  const cdptr cs_geo, cs_shade;
  const ciptr cs_kind, cs_csg;
  const bool cull;
  const int lane;
  WaveStack bst;  // (BVH only)

  // The search for the lanes in `act`. Closest mode (OC false): closestHit
  // with `tmax` and `excl` (rl and dist unused). Any-hit mode (OC true):
  // inShadow's loop for the hit on object `excl`, an occluder being a result
  // with t * rl < dist (raytracer.go:424); `found` then says occluded,
  // whichever occluder was met first (the verdict is the same).
  // rt_query_occluded_async is this mode with rl = 1.0 and dist = tmax:
  // t * 1.0 and tmax / 1.0 are exact, so its predicate t < tmax and its cull
  // limit tmax are what the lines below compute, bit for bit.
  // UNIT: the caller knows |ray.d| = 1 (the radiance kernel's shadow rays,
  // normalised by construction): the culls take the direction as it is. Every
  // other caller, the occluded query included, passes false and the culls get
  // the normalised direction and bounds scaled by |dir|.
  template <bool OC, bool UNIT>
  __device__ __forceinline__ void operator()(const Ray& ray, bool act, double tmax, int excl, BoolC<OC>, BoolC<UNIT>,
                                             double rl, double dist, bool& found, double& best_t, int& best_i,
                                             int& best_f) {
    constexpr bool occl = OC;
    // the culls' ray: unit direction, bounds in world units (see the head of this file)
    const F3 of = f3(ray.o);
    const float slack = ray_slack(of);
    double dlen = 1.0;
    F3 df;
    bool cullok;
    if constexpr (UNIT) {
      df = f3(ray.d);
      cullok = slack < 1e30f;
    } else {
      dlen = __builtin_sqrt(dot(ray.d, ray.d));
      const float dlf = (float)dlen;
      cullok = dlf > 1e-18f && dlf < 1e18f && slack < 1e30f;
      df = f3(scale(ray.d, 1.0 / dlen));
    }
    const bool nocull = !cullok;  // this lane passes every cull
    bool unit_dir = true;
    if constexpr (CSG) unit_dir = wave_all(!act || __builtin_fabs(dot(ray.d, ray.d) - 1.0) <= 1e-9);
    bool open = act;  // still searching (any-hit mode: not yet occluded)
    found = false;
    best_t = 0.0;
    best_i = 0;
    best_f = 0;
    const double slim = occl ? dist / rl : 0.0;
    // the bound a candidate has to stay below
    auto limit = [&]() { return occl ? slim : (found ? best_t : tmax); };
    auto bound_f = [&](double t0) {
      const double lim = limit();
      return lim < __builtin_inf() ? (float)((lim - t0) * dlen) * 1.0001f + 1e-4f : 3.0e38f;
    };
    // One candidate (object i of kind k, record g: all wave-uniform) for the
    // lanes in `test`. The linear loop visits objects in index order (strict <,
    // the first index wins ties); the BVH visits them in any order and breaks
    // ties on the index explicitly.
    auto exact = [&](int i, int k, const double* g, bool test) {
      if (test) {
        double t;
        int f;
        bool h;
        if constexpr (CSG) {
          if (k == RT_CSG) {
            const auto cg = cs_geo + (size_t)i * GEO;
            // Any-hit mode, no leaf cull: no cut limit. The search returns
            // the first surface crossing, its crossings ascend, and a cut at
            // a bound only turns "first crossing at or beyond the bound" into
            // "none"; the predicate below rejects that crossing as well, so a
            // cut cannot change the verdict.
            if constexpr (occl)
              h = unit_dir ? csg_hit<true>(cs_geo, cs_kind, cs_csg, Q.nobj, cg, ray, t, f, rl, dist, false)
                           : csg_search_nocull<true>(cs_geo, cs_kind, cs_csg, Q.nobj, cg, ray, t, f, __builtin_inf(),
                                                     false);
            else
              h = unit_dir ? csg_hit<true>(cs_geo, cs_kind, cs_csg, Q.nobj, cg, ray, t, f, 1.0, limit(), true)
                           : csg_search_nocull<true>(cs_geo, cs_kind, cs_csg, Q.nobj, cg, ray, t, f, limit(), true);
          } else {
            h = object_hit(k, g, ray, t, f);
          }
        } else {
          h = object_hit(k, g, ray, t, f);
        }
        if constexpr (occl) {
          if (h && t * rl < dist) {
            found = true;
            open = false;
          }
        } else {
          if (h && t < tmax && (!found || t < best_t || (BVH && t == best_t && i < best_i))) {
            found = true;
            best_t = t;
            best_i = i;
            best_f = f;
          }
        }
      }
    };
    // object i of an index-order list: the culls (when on), then the exact test
    auto list_obj = [&](int i) {
      const int k = cs_kind[i];
      double gl[GEO];
#pragma unroll
      for (int q = 0; q < GEO; q++) gl[q] = cs_geo[(size_t)i * GEO + q];
      bool test = open && i != excl;
      if (cull) {
        const float tm = bound_f(0.0);
        const bool c = k != RT_PLANE ? may_hit_a(test, of, df, tm, gl, slack)
                                     : CULL_AND(test, may_hit_plane(of, df, tm, cs_shade + (size_t)i * SHD));
        test = c || (test && nocull);
      }
      if (!wave_any(test)) return;
      exact(i, k, gl, test);
    };

    if constexpr (!BVH) {
      for (int i = 0; i < Q.nobj; i++) {
        if (occl && !wave_any(open)) break;
        list_obj(i);
      }
    } else {
      for (int p = 0; p < Q.nplanes; p++) {  // unbounded objects: planes, composites, never-culled objects
        if (occl && !wave_any(open)) break;
        list_obj(__builtin_amdgcn_readfirstlane(Q.planes[p]));
      }
      const F3 idf = f3_rcp(df);
      // far origins: the BVH culls' origin, slack and bounds (see far_shift)
      F3 bof = of;
      float bslack = slack;
      double bt0 = 0.0;
      bool btr = open;
      bool fsh = btr && cullok;  // (a lane that passes every cull keeps its origin)
      far_shift(fsh, ray, Q.bvh_lo, Q.bvh_hi, bof, bslack, bt0);
      if (cullok) btr = fsh;
      int ssp = 0;
      int nr = 0;  // the node visited next, kept in registers (see rt_render.h bvh_next)
      uint64_t nm = wave_ballot(btr);
      bool have = nm != 0;
      for (;;) {
        int r;
        uint64_t m;
        if (have) {
          r = nr;
          m = nm;
          have = false;
        } else {
          if (ssp == 0) break;
          ssp--;
          r = __builtin_amdgcn_readfirstlane(bst.ref[ssp]);
          m = ((uint64_t)__builtin_amdgcn_readfirstlane((int)(bst.mask[ssp] >> 32)) << 32) |
              (uint32_t)__builtin_amdgcn_readfirstlane((int)bst.mask[ssp]);
        }
        // (any-hit mode: a lane leaves the walk once it is occluded)
        const bool wact = btr && open && ((m >> lane) & 1);
        if (occl && !wave_any(open)) break;
        if (r & 7) {  // leaf
          const int first = r >> 3, count = r & 7;
          for (int j = first; j < first + count; j++) {
            const LeafRec L = ld_leaf(Q.bvh_geo, j);  // scalar loads (wave-uniform index)
            const bool la = wact && open && L.i != excl;
            const bool test = may_hit_s(la, bof, df, bound_f(bt0), L.cx, L.cy, L.cz, L.cr, bslack) || (la && nocull);
            if (!wave_any(test)) continue;
            exact(L.i, L.k, L.R.m, test);
          }
        } else {
          const cfptr nb = (cfptr)Q.bvh_nodes + (size_t)(r >> 3) * BN;  // scalar loads
          const ciptr ni = (ciptr)(nb + 12);
          const float tm = bound_f(bt0);
          float t0 = 0.0f, t1 = 0.0f;  // (set by may_hit_box_a when it returns true)
          const bool a0 = may_hit_box_a(wact, bof, idf, bslack, tm, nb, t0) || (wact && nocull);
          const bool a1 = may_hit_box_a(wact, bof, idf, bslack, tm, nb + 6, t1) || (wact && nocull);
          const uint64_t m0 = wave_ballot(a0), m1 = wave_ballot(a1);
          // near child first: the one most lanes enter first
          const bool c1_first = 2 * __popcll(wave_ballot(a0 && a1 && t1 < t0)) > __popcll(m0 & m1);
          bvh_next(bst, ssp, lane, c1_first, ni[0], ni[1], m0, m1, nr, nm, have);
        }
      }
    }
  }
};

// The searcher of the calling wave; s_mask and s_ref are the workgroup's
// stacks (WAVES_PER_WG * BVH_STACK entries each in a BVH kernel, the only LDS).
template <bool BVH, bool CSG, typename AR>
__device__ __forceinline__ SceneSearch<BVH, CSG, AR> scene_search(const char* blob, const AR& Q, uint64_t* s_mask,
                                                                  int* s_ref) {
  WaveStack bst;
  bst.mask = s_mask + (threadIdx.x >> 6) * BVH_STACK;
  bst.ref = s_ref + (threadIdx.x >> 6) * BVH_STACK;
  return SceneSearch<BVH, CSG, AR>{Q,
                               (cdptr)(blob + Q.off_geo),
                               (cdptr)(blob + Q.off_shade),
                               (ciptr)(blob + Q.off_kind),
                               (ciptr)(blob + Q.off_csg),
                               Q.cull != 0,
                               (int)(threadIdx.x & 63),
                               bst};
}

// ComputeSurfaceProps (raytracer.go:106-122, 182-194, 242-260, 339-370) of a
// search's winner (hit_i, hit_f, hit_t), the megakernel's SHADE block op for
// op: the surface si (the object, or a CSG composite's leaf), its face sf and
// kind k, Hit.PointObj p, the world point and normal, the material index.
template <bool CSG>
__device__ __forceinline__ void surface_props(const char* blob, const SceneRef& Q, const Ray& ray, int hit_i, int hit_f,
                                              double hit_t, int& si, int& sf, int& k, d3& p, d3& pw, d3& nw, int& mat) {
  // scene records through vector loads (per-lane indices)
  const double* v_geo = reinterpret_cast<const double*>(blob + Q.off_geo);
  const double* v_shade = reinterpret_cast<const double*>(blob + Q.off_shade);
  const int* v_kind = reinterpret_cast<const int*>(blob + Q.off_kind);
  const int* v_objmat = reinterpret_cast<const int*>(blob + Q.off_objmat);
  si = hit_i;
  sf = hit_f;
  bool flip = false;
  if constexpr (CSG) {
    if (v_kind[hit_i] == RT_CSG) {
      const int* ci = reinterpret_cast<const int*>(v_geo + (size_t)hit_i * GEO + 14);
      si = Q.nobj + ci[0] + (hit_f >> 4);
      flip = ((hit_f >> 3) & 1) != 0;
      sf = hit_f & 7;
    }
  }
  const double* g = v_geo + (size_t)si * GEO;
  const double* s = v_shade + (size_t)si * SHD;
  k = v_kind[si];
  const Ray l = to_obj(g, ray);
  p = add(l.o, scale(l.d, hit_t));
  pw = mk(s[0] * p.x + s[1] * p.y + s[2] * p.z + s[3], s[4] * p.x + s[5] * p.y + s[6] * p.z + s[7],
          s[8] * p.x + s[9] * p.y + s[10] * p.z + s[11]);
  if (k == RT_SPHERE) {
    nw = p;
  } else if (k == RT_CYLINDER || k == RT_CONE) {
    const d3 n = sf == 0 ? (k == RT_CONE ? mk(p.x, -p.y, p.z) : mk(p.x, 0, p.z)) : (sf == 1 ? mk(0, 1, 0) : mk(0, -1, 0));
    // NormalMat = WorldToObject^T (raytracer.go:814): MulDir then Normalize.
    nw = norm(mk(g[0] * n.x + g[4] * n.y + g[8] * n.z, g[1] * n.x + g[5] * n.y + g[9] * n.z,
                 g[2] * n.x + g[6] * n.y + g[10] * n.z));
  } else {
    nw = mk(s[12 + sf * 3], s[13 + sf * 3], s[14 + sf * 3]);
  }
  if (flip) nw = neg(nw);  // the composite's outward normal
  mat = v_objmat[(size_t)si * OMAT + sf];
}

// OC: the occluded mode (rt_query_occluded_async)
template <bool BVH, bool CSG, bool OC>
__global__ __launch_bounds__(WG) void rt_query_kernel(const char* __restrict__ blob, QueryArgs Q) {
  __shared__ uint64_t s_mask[BVH ? WAVES_PER_WG * BVH_STACK : 1];
  __shared__ int s_ref[BVH ? WAVES_PER_WG * BVH_STACK : 1];
  const int gid = (int)(blockIdx.x * WG + threadIdx.x);
  if (gid >= Q.n) return;  // lanes past n: inactive from here on, in no ballot

  Ray ray;
  double tmax;
  int excl;
  ray_load(Q.rays + gid, ray, tmax, excl);

  auto search = scene_search<BVH, CSG>(blob, Q, s_mask, s_ref);
  bool found;
  double best_t;
  int best_i, best_f;
  search(ray, true, tmax, excl, BoolC<OC>(), BoolC<false>(), 1.0, tmax, found, best_t, best_i, best_f);

  if constexpr (OC) {
    Q.occluded[gid] = found ? 1 : 0;
    return;
  }

  Q16* hp = reinterpret_cast<Q16*>(Q.hits + gid);
  if (!found) {
    const Q16 z = {0.0, 0.0};
    hp[0] = z;
    hp[1] = z;
    hp[2] = z;
    hp[3] = z;
    hp[4] = z;
    const Q16i zi = {-1, 0, 0, 0};
    *reinterpret_cast<Q16i*>(hp + 5) = zi;
    return;
  }
  int si, sf, k, mat;
  d3 p, pw, nw;
  surface_props<CSG>(blob, Q, ray, best_i, best_f, best_t, si, sf, k, p, pw, nw, mat);
  const Q16 h0 = {best_t, p.x}, h1 = {p.y, p.z}, h2 = {pw.x, pw.y}, h3 = {pw.z, nw.x}, h4 = {nw.y, nw.z};
  hp[0] = h0;
  hp[1] = h1;
  hp[2] = h2;
  hp[3] = h3;
  hp[4] = h4;
  const Q16i hi = {best_i, best_f, k, mat};
  *reinterpret_cast<Q16i*>(hp + 5) = hi;
}

// Index of a scene's kernel in a table of flavours [BVH | CSG << 1 | VM << 2]
int flavour(const DevScene& s) { return (s.use_bvh ? 1 : 0) | (s.has_csg ? 2 : 0) | (s.num_programs > 0 ? 4 : 0); }

// [BVH | CSG << 1 | OC << 2]
const void* const k_query_kernels[8] = {
    (const void*)rt_query_kernel<false, false, false>, (const void*)rt_query_kernel<true, false, false>,
    (const void*)rt_query_kernel<false, true, false>,  (const void*)rt_query_kernel<true, true, false>,
    (const void*)rt_query_kernel<false, false, true>,  (const void*)rt_query_kernel<true, false, true>,
    (const void*)rt_query_kernel<false, true, true>,   (const void*)rt_query_kernel<true, true, true>};

// The scene references of a launch on `c`: SceneRef's fields of R (zero-filled
// by the caller)
template <typename AR>
void scene_ref(const rt_context* c, AR& R) {
  const DevScene& s = c->sc;
  R.nobj = s.nobj;
  R.cull = (c->accel & RT_ACCEL_CULL) ? 1 : 0;
  R.off_geo = s.off_geo;
  R.off_shade = s.off_shade;
  R.off_kind = s.off_kind;
  R.off_objmat = s.off_objmat;
  R.off_csg = s.off_csg;
  if (s.use_bvh) {
    R.bvh_nodes = reinterpret_cast<const float*>(s.accel + s.off_nodes);
    R.bvh_geo = reinterpret_cast<const double*>(s.accel + s.off_bobj);
    R.planes = reinterpret_cast<const int*>(s.accel + s.off_planes);
    R.nplanes = s.nplanes;
    for (int k = 0; k < 3; k++) {
      R.bvh_lo[k] = s.bvh_lo[k];
      R.bvh_hi[k] = s.bvh_hi[k];
    }
  }
}

int query_launch(rt_context* c, const char* who, int n, const rt_ray* d_rays, void* d_out, bool occl, void* stream) {
  if (int rc = need_scene(c, who); rc != RT_OK) return rc;
  if (n < 0) return fail(RT_E_INVALID, std::string(who) + ": n < 0");
  if (n == 0) return RT_OK;
  if (!d_rays || !d_out) return fail(RT_E_INVALID, std::string(who) + ": NULL ray or output pointer");
  if (((uintptr_t)d_rays & 15) != 0 || (!occl && ((uintptr_t)d_out & 15) != 0))
    return fail(RT_E_INVALID, std::string(who) + ": ray and hit arrays must be 16-byte aligned");
  const DevScene& s = c->sc;
  DeviceGuard guard(c->device);
  QueryArgs Q;
  std::memset(&Q, 0, sizeof Q);
  scene_ref(c, Q);
  Q.rays = d_rays;
  Q.hits = occl ? nullptr : (rt_hit*)d_out;
  Q.occluded = occl ? (uint8_t*)d_out : nullptr;
  Q.n = n;
  const char* blob = s.blob;
  void* args[] = {(void*)&blob, (void*)&Q};
  // (the query kernels have no VM flag: bit 2 of their table is the mode)
  const void* kfn = k_query_kernels[(flavour(s) & 3) | (occl ? 4 : 0)];
  HIP_TRY(hipLaunchKernel(kfn, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), args, 0, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_query_closest_async(rt_context* c, int n, const rt_ray* d_rays, rt_hit* d_hits, void* stream) {
  return query_launch(c, "rt_query_closest_async", n, d_rays, d_hits, false, stream);
}

int rt_query_occluded_async(rt_context* c, int n, const rt_ray* d_rays, uint8_t* d_occluded, void* stream) {
  return query_launch(c, "rt_query_occluded_async", n, d_rays, d_occluded, true, stream);
}

}  // extern "C"
