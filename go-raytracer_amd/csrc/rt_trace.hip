// rt_trace.hip -- radiance queries and camera-ray export against the scene of
// rt_set_scene (include/rt_abi.h rt_query_radiance_async /
// rt_query_camera_rays_async).
//
// A kernel of its own beside rt_render_kernel, which it does not touch. For
// each ray of a batch it computes traceRay(ray, depth) (raytracer.go:487-562):
// closestHit, ComputeSurfaceProps (closure surfaces through run_vm),
// computeLighting with inShadow per light, the reflection and refraction
// children and the final combine -- with the exact tests of rt_render.h called
// unchanged (object_hit, csg_hit, run_vm, go_pow, combine), the search shared
// with the query kernel (SceneSearch, rt_query.hip) and the SHADE block of
// rt_render_kernel repeated op for op, so a query returns the colour a render
// sums for that ray, bit for bit.
//
// Persistent, bounded grid: trace_grid_wgs() workgroups whatever n is. Each
// lane holds one ray tree at a time; a lane that finishes takes the next ray
// index from the launch's ticket counter (one atomic per wave: the popcount of
// its idle lanes, each idle lane taking base + rank). Results are written by
// ray index. The ticket counter is the only state waves share: there is no
// waiting between waves or workgroups of any kind.
//
// The recursion is an explicit per-lane frame stack (no C++ recursion, no
// runtime-indexed local arrays) in a context-owned workspace: depth - 1 frames
// of TR_FIELDS doubles per lane in lane-interleaved rows [frame][field][lane].
// The workspace never exceeds TR_WS_MAX bytes: deeper calls run on a smaller
// grid (trace_grid_wgs).
//
// Per iteration, wave-lock-step: refill idle lanes, closest search for the
// lanes that hold a ray (SceneSearch of rt_query.hip, closest mode), shade the
// lanes that hit (the same search in any-hit mode once per light), then push a
// frame and descend or pop frames and combine.
//
// Ray directions are used as given; the FP32 culls get a unit direction and
// bounds scaled by |dir|, and composites of a wave that holds a non-unit
// direction take csg_search_nocull (see the head of rt_query.hip). Shadow rays
// are unit length by construction. The answer does not depend on rt_set_accel.
// Included by rt_kernel.hip after rt_query.hip (shares its helpers).

namespace {

enum { TR_LW = 0, TR_KR = 3, TR_PK = 4, TR_EXT = 5, TR_COL = 11, TR_REFL = 14, TR_FIELDS = 15 };
enum { TR_WG_PER_CU = 2 };                        // full grid: 2 workgroups (8 waves) per CU
constexpr size_t TR_WS_MAX = (size_t)128 << 20;  // bytes of frame stack per context, at most

// SceneRef's fields (rt_query.hip; filled by scene_ref, read by SceneSearch) are
// written out among the kernel's own, in this order, and not inherited: with
// SceneRef as a base, or placed after the other fields, most instantiations
// spill more SGPRs (up to 18) and c4csg radiance queries ran 2.3 % slower
// (DESIGN.md "Shared pieces ...", BASELINE.md "Shared search: same speed").
struct TraceArgs {
  const rt_ray* rays;
  rt_radiance* out;
  unsigned int* ticket;  // next ray index of this launch (zeroed on the stream before it)
  double* ws;            // frame stack [depth - 1][TR_FIELDS][lanes of the grid]
  int n, nobj, depth, nlights;
  int cull;  // RT_ACCEL_CULL: the FP32 culls of the object lists (wave-uniform)
  int off_geo, off_shade, off_kind, off_objmat, off_csg, off_mats, off_lights, off_code, off_consts, off_entry;
  // BVH flavour (DevScene::use_bvh)
  const float* bvh_nodes;
  const double* bvh_geo;
  const int* planes;
  int nplanes;
  double bvh_lo[3], bvh_hi[3];
};

// The kernel's argument record. GEN (camera renders, rt_camera.hip): the
// specialisation for true, defined there, adds the camera the lanes form their
// rays from; without GEN this is TraceArgs itself.
template <bool GEN>
struct TraceArgsT : TraceArgs {};

// The lanes of ballot `m` (not 0) take consecutive values of *ctr with one
// atomic per wave: the first lane of m adds their number, `base` is what it
// read, and a lane of m gets base + its rank in m (returned).
__device__ __forceinline__ unsigned int wave_take(unsigned int* ctr, uint64_t m, int lane, unsigned int& base) {
  const int first = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
  base = 0;
  if (lane == first) base = atomicAdd(ctr, (unsigned int)__popcll(m));
  base = (unsigned int)__builtin_amdgcn_readlane((int)base, first);
  return base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
}

// VM: the scene has closure surfaces (run_vm's register file lives in scratch)
// GEN: ticket t is sample t % S of the launch's pixel t / S and the lane forms
// that ray itself (cam_ticket_ray, rt_camera.hip) instead of loading Q.rays[t]
// ADP (with GEN; adaptive camera renders only): the pass's tickets go through
// its pixel list and batch, and their number is read from device memory
// (cam_ticket_limit), clamped to Q.n
template <bool BVH, bool CSG, bool VM, bool GEN, bool ADP = false>
__global__ __launch_bounds__(WG, 2) void rt_trace_kernel(const char* __restrict__ blob, TraceArgsT<GEN> Q) {
  __shared__ uint64_t s_mask[BVH ? WAVES_PER_WG * BVH_STACK : 1];
  __shared__ int s_ref[BVH ? WAVES_PER_WG * BVH_STACK : 1];
  const int lane = (int)(threadIdx.x & 63);
  const size_t nl = (size_t)gridDim.x * WG;  // lanes of the grid: the row length of the frame stack
  double* const stk = Q.ws + (size_t)blockIdx.x * WG + threadIdx.x;
  auto fld = [&](int level, int f) -> double& { return stk[((size_t)level * TR_FIELDS + f) * nl]; };

  // scene records through scalar loads (wave-uniform indices)
  const cdptr G = (cdptr)(blob + Q.off_lights);  // GLOB record, then the lights
  const cdptr lights = G + GLOB;
  // ... through vector loads (per-lane indices)
  const double* v_mats = reinterpret_cast<const double*>(blob + Q.off_mats);
  // closestHit and inShadow's loop (rt_query.hip)
  auto search = scene_search<BVH, CSG>(blob, Q, s_mask, s_ref);

  // the lane's ray tree
  bool act = false;  // holds a ray to trace
  int idx = 0;       // ray index of the tree
  int sp = 0;        // frames on the stack: the current ray's depth is Q.depth - sp
  int nrays = 0;     // rays traced for this query
  int top = -1;      // the object the query's own ray hit
  Ray ray;
  ray.o = mk(0, 0, 0);
  ray.d = mk(0, 0, 1);
  double tmax = __builtin_inf();
  int excl = -1;
  bool drained = false;  // every ray index has been handed out (wave-uniform)
  unsigned int lim = (unsigned int)Q.n;  // tickets of the launch
  if constexpr (GEN && ADP) lim = cam_ticket_limit(Q.cam, lim);

  for (;;) {
    // idle lanes take the next ray indices
    if (!drained) {
      const uint64_t im = wave_ballot(!act);
      if (im) {
        unsigned int base;
        const unsigned int mine = wave_take(Q.ticket, im, lane, base);
        if (base + (unsigned int)__popcll(im) >= lim) drained = true;
        if (!act && base < lim && mine < lim) {
          if constexpr (GEN) {
            cam_ticket_ray(Q.cam, mine, BoolC<ADP>(), ray.o, ray.d);
            tmax = __builtin_inf();
            excl = -1;
          } else {
            ray_load(Q.rays + mine, ray, tmax, excl);
          }
          idx = (int)mine;
          sp = 0;
          nrays = 1;
          top = -1;
          act = true;
        }
      }
    }
    if (!wave_any(act)) break;

    // closestHit (raytracer.go:469-483)
    bool found;
    double hit_t;
    int hit_i, hit_f;
    search(ray, act, tmax, excl, BoolC<false>(), BoolC<false>(), 1.0, 0.0, found, hit_t, hit_i, hit_f);
    if (act && sp == 0) top = found ? hit_i : -1;
    bool have_res = false;
    d3 res = mk(0, 0, 0);
    if (act && !found) {  // background gradient, raytracer.go:493-497
      const double t = 0.5 * (ray.d.y + 1.0);
      res = lerp(mk(G[3], G[4], G[5]), mk(G[6], G[7], G[8]), t);
      have_res = true;
    }
    const bool hit = act && found;
    if (wave_any(hit)) {
      // ComputeSurfaceProps (raytracer.go:106-122, 182-194, 242-260, 339-370)
      d3 pw = mk(0, 0, 0), nw = mk(0, 0, 1);
      int mat = 0;
      double vr[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // a closure surface's material (rt_material order)
      (void)vr;
      if (hit) {
        // surface_props (rt_query.hip) written out: called as a function, in
        // any form tried, it costs <1, 0, 0> 40 VGPRs and a wave per SIMD
        // (DESIGN.md "Shared pieces of the query, radiance and camera
        // kernels"). Keep the two in step.
        const double* v_geo = reinterpret_cast<const double*>(blob + Q.off_geo);
        const double* v_shade = reinterpret_cast<const double*>(blob + Q.off_shade);
        const int* v_kind = reinterpret_cast<const int*>(blob + Q.off_kind);
        const int* v_objmat = reinterpret_cast<const int*>(blob + Q.off_objmat);
        int si = hit_i, sf = hit_f;  // the surface: the object, or a CSG composite's leaf
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
        const int k = v_kind[si];
        const Ray l = to_obj(g, ray);
        const d3 p = add(l.o, scale(l.d, hit_t));  // Hit.PointObj
        pw = mk(s[0] * p.x + s[1] * p.y + s[2] * p.z + s[3], s[4] * p.x + s[5] * p.y + s[6] * p.z + s[7],
                s[8] * p.x + s[9] * p.y + s[10] * p.z + s[11]);
        if (k == RT_SPHERE) {
          nw = p;
        } else if (k == RT_CYLINDER || k == RT_CONE) {
          const d3 n =
              sf == 0 ? (k == RT_CONE ? mk(p.x, -p.y, p.z) : mk(p.x, 0, p.z)) : (sf == 1 ? mk(0, 1, 0) : mk(0, -1, 0));
          // NormalMat = WorldToObject^T (raytracer.go:814): MulDir then Normalize.
          nw = norm(mk(g[0] * n.x + g[4] * n.y + g[8] * n.z, g[1] * n.x + g[5] * n.y + g[9] * n.z,
                       g[2] * n.x + g[6] * n.y + g[10] * n.z));
        } else {
          nw = mk(s[12 + sf * 3], s[13 + sf * 3], s[14 + sf * 3]);
        }
        if (flip) nw = neg(nw);  // the composite's outward normal
        mat = v_objmat[(size_t)si * OMAT + sf];
        if constexpr (VM) {
          if (mat < 0) {
            // Closure surface: (face, u, v) as ComputeSurfaceProps computes them
            // (raytracer.go:124-150, 196-205, 249, 339-359), then the VM.
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
            if (bad)  // the material reads as all-zero (oracle convention); counted nowhere
              for (int q = 0; q < 10; q++) vr[q] = 0.0;
          }
        }
      }

      // computeLighting + inShadow (raytracer.go:372-429)
      const double* M = v_mats + (size_t)(mat < 0 ? 0 : mat) * MAT;
      double m_kd = 0.0, m_ks = 0.0, m_se = 0.0;
      if (hit) {
        m_kd = M[9];
        m_ks = M[10];
        m_se = M[11];
        if constexpr (VM) {
          if (mat < 0) {
            m_kd = vr[7];
            m_ks = vr[8];
            m_se = vr[9];
          }
        }
      }
      d3 L = mk(0, 0, 0);
      if (hit) L = scale(mk(G[0], G[1], G[2]), m_kd);
      const double rlen = len(ray.d);
      const d3 sorig = add(pw, scale(nw, 1e-4));
      const int exp_mode = (int)G[11];
      for (int li = 0; li < Q.nlights; li++) {
        const cdptr lt = lights + (size_t)li * LGT;
        const int lkind = (int)lt[9];  // wave-uniform
        // direction and distance to the light (raytracer.go:378-380)
        d3 ldir;
        double dist;
        if (lkind == RT_LIGHT_DIRECTIONAL) {  // extension: light at infinity
          ldir = mk(lt[6], lt[7], lt[8]);
          dist = __builtin_inf();
        } else {
          const d3 lth = sub(mk(lt[0], lt[1], lt[2]), pw);
          ldir = norm_len(lth, dist);  // dist = len(lth)
        }
        Ray sr;
        sr.o = sorig;
        sr.d = ldir;
        bool shadowed;
        double st;
        int si_, sf_;
        // (unit length: ldir is normalised above)
        search(sr, hit, __builtin_inf(), hit_i, BoolC<true>(), BoolC<true>(), rlen, dist, shadowed, st, si_, sf_);
        if (hit && !shadowed) {
          d3 lcol = mk(lt[3], lt[4], lt[5]);
          if (lkind == RT_LIGHT_SPOT) {  // extension: cone falloff
            const double ca = dot(neg(ldir), mk(lt[6], lt[7], lt[8]));
            lcol = scale(lcol, ca >= lt[10] ? go_pow(ca, lt[11], exp_mode) : 0.0);
          }
          const double ndl = go_max0(dot(nw, ldir));
          const d3 diffuse = scale(lcol, ndl * m_kd);
          const d3 H = norm(add(neg(ray.d), ldir));
          const double spec = go_max0(dot(nw, H));
          const d3 specular = scale(lcol, m_ks * go_pow(spec, m_se, exp_mode));
          L = add(add(L, diffuse), specular);
        }
      }

      // traceRay body after lighting (raytracer.go:505-561)
      if (hit) {
        // the material record's remaining entries (rt_render.h: mats): 4..5 the
        // baked fuzz offset, 6 fuzz >= 0, 12 = 1 / ior, 13 = ((1 - ior) / (1 + ior))^2
        d3 col = mk(M[0], M[1], M[2]);
        double refl = M[3], fz4 = M[4], fz5 = M[5], fz6 = M[6], T = M[7], ior = M[8], m12 = M[12], m13 = M[13];
        if constexpr (VM) {
          if (mat < 0) {
            col = mk(vr[0], vr[1], vr[2]);
            refl = vr[3];
            const double fz = vr[4];
            if (fz >= 0) {  // baked constant fuzz offset (raytracer.go:516-522)
              const double cf = rt::go_cos(fz), sf = rt::go_sin(fz);
              fz4 = fz * cf * cf;
              fz5 = fz * sf * sf;
              fz6 = 1.0;
            } else {
              fz4 = fz5 = fz6 = 0.0;
            }
            T = vr[5];
            ior = vr[6];
            m12 = 1.0 / ior;  // (the host's per-material terms, see rt_set_scene)
            const double r0 = (1.0 - ior) / (1.0 + ior);
            m13 = r0 * r0;
          }
        }
        if (refl == 0 && T == 0) {
          res = clamp(mul(L, col));
          have_res = true;
        } else {
          const bool hasR = refl > 0;
          Ray rr;
          rr.o = mk(0, 0, 0);
          rr.d = mk(0, 0, 1);
          if (hasR) {
            d3 rd = sub(ray.d, scale(nw, 2.0 * dot(ray.d, nw)));
            if (fz6 != 0.0) rd = add(rd, mk(fz4, fz5, 0.0));
            rr.o = sorig;  // (= add(pw, scale(nw, 1e-4)), raytracer.go:526)
            rr.d = norm(rd);
          }
          const bool tmode = T > 0;
          bool hasT = false;
          Ray trr;
          trr.o = mk(0, 0, 0);
          trr.d = mk(0, 0, 1);
          double kr = 0.0;
          d3 lw = L;
          if (tmode) {
            // n1 / n2: 1 / ior from outside, ior / 1 = ior from inside
            double ratio = m12;
            d3 nn = nw;
            if (dot(ray.d, nn) > 0.0) {
              ratio = ior;
              nn = scale(nn, -1.0);
            }
            // refract (raytracer.go:438-450)
            const double cosI = -dot(nn, ray.d);
            const double sinT2 = ratio * ratio * (1.0 - cosI * cosI);
            if (!(sinT2 > 1.0)) {
              const double cosT = gsqrt(1.0 - sinT2);
              const d3 td = add(scale(ray.d, ratio), scale(nn, ratio * cosI - cosT));
              if (!iszero(td)) {
                hasT = true;
                trr.o = sub(pw, scale(nn, 1e-4));
                trr.d = td;
              }
            }
            // fresnel (raytracer.go:456-467) on the unflipped normal
            const double cosi = dot(ray.d, nw) / (rlen * len(nw));  // (rlen = len(ray.d), above)
            const double cost = __builtin_fabs(cosi);
            kr = m13 + (1 - m13) * go_pow(1 - cost, 5);
            lw = scale(L, 1.0 - T);
          }
          const int d = Q.depth - sp;  // depth of the current ray
          if (d - 1 > 0 && (hasR || hasT)) {
            fld(sp, TR_LW + 0) = lw.x;
            fld(sp, TR_LW + 1) = lw.y;
            fld(sp, TR_LW + 2) = lw.z;
            fld(sp, TR_KR) = kr;
            if (hasR && hasT) {  // the pending refraction ray
              fld(sp, TR_EXT + 0) = trr.o.x;
              fld(sp, TR_EXT + 1) = trr.o.y;
              fld(sp, TR_EXT + 2) = trr.o.z;
              fld(sp, TR_EXT + 3) = trr.d.x;
              fld(sp, TR_EXT + 4) = trr.d.y;
              fld(sp, TR_EXT + 5) = trr.d.z;
            }
            fld(sp, TR_COL + 0) = col.x;
            fld(sp, TR_COL + 1) = col.y;
            fld(sp, TR_COL + 2) = col.z;
            fld(sp, TR_REFL) = refl;
            const long long packed = (tmode ? FL_TMODE : 0) | (hasR ? FL_HASR : 0) | (hasT ? FL_HAST : 0);
            fld(sp, TR_PK) = __longlong_as_double(packed);
            sp++;
            nrays += (hasR ? 1 : 0) + (hasT ? 1 : 0);  // both children will be traced (d - 1 > 0)
            ray = hasR ? rr : trr;
            tmax = __builtin_inf();  // tmax and exclude bound the query's own ray only
            excl = -1;
          } else {
            res = combine(tmode, lw, col, refl, kr, mk(0, 0, 0), mk(0, 0, 0));
            have_res = true;
          }
        }
      }
    }

    // A finished traceRay colour goes up the lane's frame stack (post-order,
    // raytracer.go:528/554/557-561): the lane ends tracing a pending
    // refraction child, or idle with its result written.
    while (wave_any(have_res)) {
      if (have_res) {
        if (sp == 0) {
          Q16* op = reinterpret_cast<Q16*>(Q.out + idx);
          const Q16 o0 = {res.x, res.y};
          const R16 o1 = {res.z, top, nrays};
          op[0] = o0;
          *reinterpret_cast<R16*>(op + 1) = o1;
          act = false;
          have_res = false;
        } else {
          const int fl = (int)(__double_as_longlong(fld(sp - 1, TR_PK)) & 0xff);
          if ((fl & FL_HASR) && (fl & FL_HAST) && !(fl & FL_STAGE)) {
            // reflection child done: trace the pending refraction child; the
            // reflection's colour takes the pending ray's first rows
            fld(sp - 1, TR_PK) = __longlong_as_double((long long)(fl | FL_STAGE));
            ray.o = mk(fld(sp - 1, TR_EXT + 0), fld(sp - 1, TR_EXT + 1), fld(sp - 1, TR_EXT + 2));
            ray.d = mk(fld(sp - 1, TR_EXT + 3), fld(sp - 1, TR_EXT + 4), fld(sp - 1, TR_EXT + 5));
            fld(sp - 1, TR_EXT + 0) = res.x;
            fld(sp - 1, TR_EXT + 1) = res.y;
            fld(sp - 1, TR_EXT + 2) = res.z;
            have_res = false;
          } else {
            d3 R = mk(0, 0, 0), Tr = mk(0, 0, 0);
            if ((fl & FL_HASR) && (fl & FL_HAST)) {
              R = mk(fld(sp - 1, TR_EXT + 0), fld(sp - 1, TR_EXT + 1), fld(sp - 1, TR_EXT + 2));
              Tr = res;
            } else if (fl & FL_HASR) {
              R = res;
            } else {
              Tr = res;
            }
            const d3 lw = mk(fld(sp - 1, TR_LW + 0), fld(sp - 1, TR_LW + 1), fld(sp - 1, TR_LW + 2));
            const d3 fcol = mk(fld(sp - 1, TR_COL + 0), fld(sp - 1, TR_COL + 1), fld(sp - 1, TR_COL + 2));
            res = combine((fl & FL_TMODE) != 0, lw, fcol, fld(sp - 1, TR_REFL), fld(sp - 1, TR_KR), R, Tr);
            sp--;
          }
        }
      }
    }
  }
}

// The reference camera's rays (raytracer.go:605-652) for rows [y0, y1): one
// thread per (column, 20-row strip) walks its rows in order with the strip's
// PCG stream, consuming the draws of rows before y0.
__global__ __launch_bounds__(WG) void rt_camera_rays_kernel(const char* __restrict__ blob, int off_lights, int width,
                                                             int height, int y0, int y1, int nstrips, rt_ray* out) {
  const int tid = (int)(blockIdx.x * WG + threadIdx.x);
  if (tid >= width * nstrips) return;
  const int x = tid % width;
  const int ymin = (y0 / 20 + tid / width) * 20;
  const int ymax = ymin + 20 < height ? ymin + 20 : height;
  const double* G = reinterpret_cast<const double*>(blob + off_lights);
  const double vw = G[9], vh = G[10];
  const double W1 = (double)(width - 1), H1 = (double)(height - 1);
  const d3 eye = mk(0.0, 0.0, -1.0);  // raytracer.go:605-609
  Pcg rng{0xDEADULL ^ (uint64_t)x, 0xBEEFULL ^ (uint64_t)ymin};  // raytracer.go:632-634
  for (int y = ymin; y < ymax && y < y1; y++) {
    for (int k = 0; k < 4; k++) {
      const double dx = pcg_float64(rng) - 0.5;
      const double dy = pcg_float64(rng) - 0.5;
      if (y < y0) continue;  // rows before the band: draws consumed only
      const double u = ((double)x + dx) / W1 * vw - vw / 2.0;
      const double v = ((double)y + dy) / H1 * vh - vh / 2.0;
      const d3 o = mk(u, -v, 0.0);
      const d3 d = norm(sub(o, eye));
      ray_store(out + ((size_t)(y - y0) * width + x) * 4 + k, o, d);
    }
  }
}

// [BVH | CSG << 1 | VM << 2]
const void* const k_trace_kernels[8] = {
    (const void*)rt_trace_kernel<false, false, false, false>, (const void*)rt_trace_kernel<true, false, false, false>,
    (const void*)rt_trace_kernel<false, true, false, false>,  (const void*)rt_trace_kernel<true, true, false, false>,
    (const void*)rt_trace_kernel<false, false, true, false>,  (const void*)rt_trace_kernel<true, false, true, false>,
    (const void*)rt_trace_kernel<false, true, true, false>,   (const void*)rt_trace_kernel<true, true, true, false>};

// Workgroups of the persistent grid for a call at `depth`: TR_WG_PER_CU per CU,
// fewer when depth - 1 frames for that many lanes would exceed TR_WS_MAX.
int trace_grid_wgs(const rt_context* c, int depth) {
  const size_t per_wg = (size_t)std::max(1, depth - 1) * TR_FIELDS * sizeof(double) * WG;
  const size_t fit = std::max<size_t>(1, TR_WS_MAX / per_wg);
  return (int)std::min<size_t>((size_t)std::max(1, c->cus) * TR_WG_PER_CU, fit);
}

int trace_depth(const rt_context* c, const char* who, int depth, int* out) {
  if (depth < 0 || depth > RT_RADIANCE_MAX_DEPTH)
    return fail(RT_E_INVALID, std::string(who) + ": depth outside [0, RT_RADIANCE_MAX_DEPTH]");
  *out = depth == 0 ? c->sc.depth : depth;  // (the scene's depth: 3 when the scene gave <= 0)
  if (*out > RT_RADIANCE_MAX_DEPTH)
    return fail(RT_E_INVALID, std::string(who) + ": the scene's depth exceeds RT_RADIANCE_MAX_DEPTH");
  return RT_OK;
}

// The output pointer of a camera-ray export
int ray_out_check(const rt_ray* d_rays, const char* who) {
  if (!d_rays) return fail(RT_E_INVALID, std::string(who) + ": NULL ray pointer");
  if (((uintptr_t)d_rays & 15) != 0) return fail(RT_E_INVALID, std::string(who) + ": ray array must be 16-byte aligned");
  return RT_OK;
}

// What a launch of n tickets at depth D needs before it: the grid, the frame
// stack (grown when a call needs more: calls on a context are ordered), the
// zeroed ticket and the argument record (zero-filled by the caller).
int trace_prepare(rt_context* c, int n, int D, const rt_ray* d_rays, rt_radiance* d_out, hipStream_t stream,
                  TraceArgs& Q, int& wgs_out) {
  const DevScene& s = c->sc;
  const int wgs = std::min(trace_grid_wgs(c, D), (n + WG - 1) / WG);
  const size_t need = (size_t)std::max(1, D - 1) * TR_FIELDS * sizeof(double) * WG * (size_t)wgs;
  if (int rc = grow(c->trace_ws, c->trace_ws_bytes, need); rc != RT_OK) return rc;
  if (!c->trace_ticket) HIP_TRY(hipMalloc((void**)&c->trace_ticket, 64));
  HIP_TRY(hipMemsetAsync(c->trace_ticket, 0, sizeof(unsigned int), stream));
  scene_ref(c, Q);
  Q.rays = d_rays;
  Q.out = d_out;
  Q.ticket = c->trace_ticket;
  Q.ws = c->trace_ws;
  Q.n = n;
  Q.depth = D;
  Q.nlights = s.nlights;
  Q.off_mats = s.off_mats;
  Q.off_lights = s.off_lights;
  Q.off_code = s.off_code;
  Q.off_consts = s.off_consts;
  Q.off_entry = s.off_entry;
  wgs_out = wgs;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_query_radiance_async(rt_context* c, int n, const rt_ray* d_rays, int depth, rt_radiance* d_out, void* stream) {
  const char* who = "rt_query_radiance_async";
  if (int rc = need_scene(c, who); rc != RT_OK) return rc;
  if (n < 0) return fail(RT_E_INVALID, std::string(who) + ": n < 0");
  int D = 0;
  if (int rc = trace_depth(c, who, depth, &D); rc != RT_OK) return rc;
  if (n == 0) return RT_OK;
  if (!d_rays || !d_out) return fail(RT_E_INVALID, std::string(who) + ": NULL ray or output pointer");
  if (((uintptr_t)d_rays & 15) != 0 || ((uintptr_t)d_out & 15) != 0)
    return fail(RT_E_INVALID, std::string(who) + ": ray and radiance arrays must be 16-byte aligned");
  const DevScene& s = c->sc;
  DeviceGuard guard(c->device);
  TraceArgs Q;
  std::memset(&Q, 0, sizeof Q);
  int wgs = 0;
  if (int rc = trace_prepare(c, n, D, d_rays, d_out, (hipStream_t)stream, Q, wgs); rc != RT_OK) return rc;
  const char* blob = s.blob;
  void* args[] = {(void*)&blob, (void*)&Q};
  const void* kfn = k_trace_kernels[flavour(s)];
  HIP_TRY(hipLaunchKernel(kfn, dim3((unsigned)wgs), dim3(WG), args, 0, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

int rt_query_radiance_lanes(rt_context* c, int depth) {
  const char* who = "rt_query_radiance_lanes";
  if (!c) return fail(RT_E_INVALID, std::string(who) + ": NULL context");
  if (depth == 0 && !c->has_scene) return fail(RT_E_INVALID, std::string(who) + ": no scene set");
  int D = 0;
  if (int rc = trace_depth(c, who, depth, &D); rc != RT_OK) return rc;
  return trace_grid_wgs(c, D) * WG;
}

int rt_query_camera_rays_async(rt_context* c, int y0, int y1, rt_ray* d_rays, void* stream) {
  const char* who = "rt_query_camera_rays_async";
  if (int rc = need_scene(c, who); rc != RT_OK) return rc;
  const DevScene& s = c->sc;
  if (y0 < 0 || y1 > s.height || y0 >= y1)
    return fail(RT_E_INVALID, std::string(who) + ": rows must satisfy 0 <= y0 < y1 <= height");
  if (int rc = ray_out_check(d_rays, who); rc != RT_OK) return rc;
  DeviceGuard guard(c->device);
  const int nstrips = (y1 - 1) / 20 - y0 / 20 + 1;
  const long long threads = (long long)s.width * nstrips;
  const char* blob = s.blob;
  int off_lights = s.off_lights, width = s.width, height = s.height, ns = nstrips;
  void* args[] = {(void*)&blob, (void*)&off_lights, (void*)&width, (void*)&height,
                  (void*)&y0,   (void*)&y1,         (void*)&ns,    (void*)&d_rays};
  HIP_TRY(hipLaunchKernel((const void*)rt_camera_rays_kernel, dim3((unsigned)((threads + WG - 1) / WG)), dim3(WG), args,
                          0, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return RT_OK;
}

}  // extern "C"
