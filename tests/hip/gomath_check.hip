// Device check (test infrastructure): rt_device.h go_sin / go_cos / go_asin /
// go_acos / go_atan2 / go_f2i / go_f64_to_u32 (the kernels' restatements of
// Go's math.Sin, Cos, Asin, Acos, Atan2 and of the amd64 float -> int
// conversions) against the oracle's host restatements (oracle/go_math.h),
// bit for bit; any NaN equals any NaN, signed zeros must match. Inputs come
// from a fixed-seed generator, by family (DESIGN "Go math on the device");
// the count of every family is reported. For |x| >= 2^29 the device sin / cos
// return NaN by design (Go would run Payne-Hanek, restated nowhere): NaN is
// required there and the oracle, which has no guard, is not asked.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (tests/hip/Makefile)
#include "rt_device.h"
extern "C" {
#include "go_math.h"
}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

__global__ void run(int nt, const double* xt, double* sn, double* cs, int na, const double* xa, double* as, double* ac,
                    int n2, const double* y2, const double* x2, double* at, int nf, const double* xf, long long* fi,
                    uint32_t* fu) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nt) {
    sn[i] = rt::go_sin(xt[i]);
    cs[i] = rt::go_cos(xt[i]);
  }
  if (i < na) {
    as[i] = rt::go_asin(xa[i]);
    ac[i] = rt::go_acos(xa[i]);
  }
  if (i < n2) at[i] = rt::go_atan2(y2[i], x2[i]);
  if (i < nf) {
    fi[i] = rt::go_f2i(xf[i]);
    fu[i] = rt::go_f64_to_u32(xf[i]);
  }
}

static uint64_t s_state = 0x13198A2E03707344ULL;
static uint64_t next() {
  s_state += 0x9E3779B97F4A7C15ULL;
  uint64_t z = s_state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
static double uni() { return (double)(next() >> 11) / 9007199254740992.0; }
static double sgn() { return (next() & 1) ? -1.0 : 1.0; }
static uint64_t bits(double a) {
  uint64_t u;
  memcpy(&u, &a, 8);
  return u;
}
static double from_bits(uint64_t u) {
  double a;
  memcpy(&a, &u, 8);
  return a;
}
static bool same(double a, double b) { return (a != a && b != b) || bits(a) == bits(b); }
// x moved by k units in the last place (finite x, away from the sign change)
static double ulps(double x, int k) { return from_bits(bits(x) + (uint64_t)(int64_t)k); }

// One function's inputs, with the families' counts in the order they were added.
struct Inputs {
  std::vector<double> a, b;
  std::vector<std::pair<std::string, long>> fam;
  void family(const char* name) { fam.push_back({name, 0}); }
  void add(double x, double y = 0.0) {
    a.push_back(x);
    b.push_back(y);
    fam.back().second++;
  }
  void both(double x) {
    add(x);
    add(-x);
  }
  int n() const { return (int)a.size(); }
};

static const double INF = __builtin_inf(), QNAN = __builtin_nan(""), P2_29 = 536870912.0, P2_63 = 9223372036854775808.0;
static const double OFFS_ULP[] = {0, 1, -1, 2, -2, 16, -16};

static void trig_inputs(Inputs& t, int n) {
  const double PI = 3.141592653589793, PI4 = 0.7853981633974483;
  t.family("uniform");
  for (int i = 0; i < n / 2; i++) t.add((uni() * 2.0 - 1.0) * 8.0 * PI);
  t.family("k_pi_4");
  const long kmax = (long)(P2_29 * 1.2732395447351628);  // the largest k with k*pi/4 < 2^29, or one above it
  for (int i = 0; i <= 64 + 16; i++) {
    const double c = (double)(i <= 64 ? (long)i : kmax - (i - 65)) * PI4;
    for (double o : OFFS_ULP) t.both(c == 0 ? from_bits((uint64_t)(o < 0 ? -o : o)) * (o < 0 ? -1.0 : 1.0) : ulps(c, (int)o));
    t.both(c + 1e-9);
    t.both(c - 1e-9);
  }
  t.family("log_uniform");
  for (int i = 0; i < n / 2; i++) {
    const int e = (int)(next() % (1074 + 29)) - 1073;  // [2^-1074, 2^29)
    t.add(sgn() * ldexp(0.5 + uni() * 0.5, e));
  }
  t.family("degrees");  // the VM's product for whole and half degrees
  for (int h = -1440; h <= 1440; h++) t.add((h * 0.5) * 0.017453292519943295);
  t.family("specials");
  for (double x : {0.0, 4.9e-324, 1e-310, 2.2250738585072009e-308, 2.2250738585072014e-308, INF}) t.both(x);
  t.add(QNAN);
  t.family("threshold");
  for (double x : {P2_29, ulps(P2_29, -1), P2_29 + 1.0, 1e300}) t.both(x);
}

static void asin_inputs(Inputs& t, int n) {
  t.family("uniform");
  for (int i = 0; i < n; i++) t.add(uni() * 2.0 - 1.0);
  t.family("around_0.7");
  for (int k = -16; k <= 16; k++) t.both(ulps(0.7, k));
  t.family("around_satan_0.66");  // ax / sqrt(1 - ax^2) = 0.66 at ax = 0.66 / sqrt(1 + 0.66^2)
  const double ax = 0.66 / sqrt(1.0 + 0.66 * 0.66);
  for (int k = -16; k <= 16; k++) t.both(ulps(ax, k));
  t.family("ends");
  for (double x : {1.0, ulps(1.0, -1), ulps(1.0, -2), ulps(1.0, 1), 2.0, 0.0}) t.both(x);
  t.family("specials");
  for (double x : {4.9e-324, 1e-310, 2.2250738585072009e-308, INF}) t.both(x);
  t.add(QNAN);
}

static void atan2_inputs(Inputs& t, int n) {
  t.family("log_uniform");
  for (int i = 0; i < n; i++) {
    const double y = sgn() * ldexp(0.5 + uni() * 0.5, (int)(next() % 601) - 300);
    t.add(y, sgn() * ldexp(0.5 + uni() * 0.5, (int)(next() % 601) - 300));
  }
  t.family("quotient_thresholds");  // y / x within a few ulps of 0.66 and of Tan3pio8
  for (int i = 0; i < 4096; i++) {
    const double x = 1.0 + uni(), q = (i & 1) ? 2.414213562373095 : 0.66;
    t.add(sgn() * ulps(x * q, (int)(next() % 9) - 4), sgn() * x);
  }
  t.family("quotient_underflow_overflow");
  for (int i = 0; i < 256; i++) {
    const double s = ldexp(0.5 + uni() * 0.5, -600 - (int)(next() % 400)), l = ldexp(0.5 + uni() * 0.5, 600 + (int)(next() % 400));
    t.add(sgn() * s, sgn() * l);
    t.add(sgn() * l, sgn() * s);
  }
  t.family("special_table");
  const double sp[7] = {QNAN, -INF, -1.0, -0.0, 0.0, 1.0, INF};
  for (double y : sp)
    for (double x : sp) t.add(y, x);
}

static void f2i_inputs(Inputs& t, int n) {
  t.family("around_2^63");
  for (double x : {P2_63, ulps(P2_63, -1), ulps(P2_63, -2), ulps(P2_63, 1), 9.3e18, 1e300}) t.both(x);
  t.family("around_2^32_2^53");
  for (double x : {4294967295.0, 4294967296.0, 4294967297.0, 4294967295.5, 9007199254740991.0, 9007199254740992.0,
                   9007199254740994.0, 2147483648.0, 2147483647.5})
    t.both(x);
  t.family("specials");
  for (double x : {0.0, 0.5, 1.5, 0.9999999999999999, 4.9e-324, INF}) t.both(x);
  t.add(QNAN);
  t.family("colour_channels");  // c * 65535.0 as the frame's bytes are made, c around 0, 1 and every byte boundary
  for (int k = 0; k <= 256; k++)
    for (double c0 : {k / 256.0, (k * 256) / 65535.0})
      for (double o : OFFS_ULP) {
        const double c = c0 == 0 ? from_bits((uint64_t)(o < 0 ? -o : o)) * (o < 0 ? -1.0 : 1.0) : ulps(c0, (int)o);
        t.add(c * 65535.0);
      }
  t.family("random_bits");
  for (int i = 0; i < n; i++) t.add(from_bits(next()));
}

template <class T>
static T* to_device(const std::vector<T>& v) {
  T* d;
  if (hipMalloc(&d, sizeof(T) * v.size()) || hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice)) exit(2);
  return d;
}
template <class T>
static void fetch(std::vector<T>& h, T* d) {
  if (hipMemcpy(h.data(), d, sizeof(T) * h.size(), hipMemcpyDeviceToHost)) exit(2);
}
template <class T>
static T* device_out(int n) {
  T* d;
  if (hipMalloc(&d, sizeof(T) * n) || hipMemset(d, 0xEE, sizeof(T) * n)) exit(2);
  return d;
}

static void print_families(const char* name, const Inputs& t, bool last = false) {
  printf("\"%s\": {", name);
  for (size_t i = 0; i < t.fam.size(); i++) printf("%s\"%s\": %ld", i ? ", " : "", t.fam[i].first.c_str(), t.fam[i].second);
  printf("}%s", last ? "" : ", ");
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : (1 << 20);
  if (n < 16 || n > (1 << 24)) return 2;
  Inputs T, A, B, F;
  trig_inputs(T, n);
  asin_inputs(A, n);
  atan2_inputs(B, n);
  f2i_inputs(F, n);
  const int nt = T.n(), na = A.n(), n2 = B.n(), nf = F.n();
  int top = nt;
  for (int m : {na, n2, nf}) top = m > top ? m : top;
  double *dxt = to_device(T.a), *dxa = to_device(A.a), *dy2 = to_device(B.a), *dx2 = to_device(B.b), *dxf = to_device(F.a);
  double *dsn = device_out<double>(nt), *dcs = device_out<double>(nt), *das = device_out<double>(na),
         *dac = device_out<double>(na), *dat = device_out<double>(n2);
  long long* dfi = device_out<long long>(nf);
  uint32_t* dfu = device_out<uint32_t>(nf);
  run<<<(top + 255) / 256, 256>>>(nt, dxt, dsn, dcs, na, dxa, das, dac, n2, dy2, dx2, dat, nf, dxf, dfi, dfu);
  if (hipDeviceSynchronize() != hipSuccess) return 3;
  std::vector<double> sn(nt), cs(nt), as(na), ac(na), at(n2);
  std::vector<long long> fi(nf);
  std::vector<uint32_t> fu(nf);
  fetch(sn, dsn), fetch(cs, dcs), fetch(as, das), fetch(ac, dac), fetch(at, dat), fetch(fi, dfi), fetch(fu, dfu);

  long bad_sin = 0, bad_cos = 0, bad_asin = 0, bad_acos = 0, bad_atan2 = 0, bad_f2i = 0, bad_u32 = 0;
  // sin / cos: octant = (uint64)(|x| * 4/Pi) & 7 as the reduction first computes it (before the odd step)
  long oct[8] = {0}, beyond = 0, beyond_not_nan = 0;
  for (int i = 0; i < nt; i++) {
    const double x = T.a[i];
    if (fabs(x) >= P2_29 && !__builtin_isinf(x)) {
      beyond++;
      beyond_not_nan += !(sn[i] != sn[i]) + !(cs[i] != cs[i]);
      continue;
    }
    if (x == x && !__builtin_isinf(x)) oct[(uint64_t)(fabs(x) * GO_4_OVER_PI) & 7]++;
    const double ws = go_sin(x), wc = go_cos(x);
    if (!same(sn[i], ws) && bad_sin++ < 5) fprintf(stderr, "sin(%.17g): gpu %.17g oracle %.17g\n", x, sn[i], ws);
    if (!same(cs[i], wc) && bad_cos++ < 5) fprintf(stderr, "cos(%.17g): gpu %.17g oracle %.17g\n", x, cs[i], wc);
  }
  // asin / acos: which side of 0.7 and of satan's 0.66 the inputs fall on
  long as_hi = 0, as_lo = 0, satan_lo = 0, satan_mid = 0, acos_neg_zero = 0;
  for (int i = 0; i < na; i++) {
    const double x = A.a[i], axx = fabs(x);
    if (axx <= 1) {
      (axx > 0.7 ? as_hi : as_lo)++;
      if (axx <= 0.7 && axx > 0) (axx / sqrt(1 - axx * axx) <= 0.66 ? satan_lo : satan_mid)++;
    }
    if (x == 0 && go_signbit(x)) acos_neg_zero += bits(ac[i]) == bits(GO_PI_2);
    const double ws = go_asin(x), wc = go_acos(x);
    if (!same(as[i], ws) && bad_asin++ < 5) fprintf(stderr, "asin(%.17g): gpu %.17g oracle %.17g\n", x, as[i], ws);
    if (!same(ac[i], wc) && bad_acos++ < 5) fprintf(stderr, "acos(%.17g): gpu %.17g oracle %.17g\n", x, ac[i], wc);
  }
  // atan2: the branch of satan the quotient takes
  long q_lo = 0, q_mid = 0, q_hi = 0, q_zero = 0, q_inf = 0;
  for (int i = 0; i < n2; i++) {
    const double y = B.a[i], x = B.b[i], q = fabs(y / x);
    if (y == y && x == x && y != 0 && x != 0 && !__builtin_isinf(x) && !__builtin_isinf(y)) {
      if (q == 0) q_zero++;
      else if (__builtin_isinf(q)) q_inf++;
      else (q <= 0.66 ? q_lo : q > 2.41421356237309504880 ? q_hi : q_mid)++;
    }
    const double w = go_atan2(y, x);
    if (!same(at[i], w) && bad_atan2++ < 5) fprintf(stderr, "atan2(%.17g, %.17g): gpu %.17g oracle %.17g\n", y, x, at[i], w);
  }
  long f_min = 0;
  for (int i = 0; i < nf; i++) {
    const double x = F.a[i];
    const int64_t w = go_f2i(x);
    f_min += w == INT64_MIN;
    if ((int64_t)fi[i] != w && bad_f2i++ < 5) fprintf(stderr, "f2i(%.17g): gpu %lld oracle %lld\n", x, fi[i], (long long)w);
    const uint32_t wu = go_f64_to_u32(x);
    if (fu[i] != wu && bad_u32++ < 5) fprintf(stderr, "u32(%.17g): gpu %u oracle %u\n", x, fu[i], wu);
  }

  printf("{\"n\": %d, \"cases\": {\"trig\": %d, \"asin\": %d, \"atan2\": %d, \"f2i\": %d}, ", n, nt, na, n2, nf);
  printf("\"mismatches\": {\"sin\": %ld, \"cos\": %ld, \"asin\": %ld, \"acos\": %ld, \"atan2\": %ld, \"f2i\": %ld, "
         "\"f64_to_u32\": %ld}, ", bad_sin, bad_cos, bad_asin, bad_acos, bad_atan2, bad_f2i, bad_u32);
  printf("\"octants\": [%ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld], ", oct[0], oct[1], oct[2], oct[3], oct[4], oct[5],
         oct[6], oct[7]);
  printf("\"beyond_2^29\": %ld, \"beyond_2^29_not_nan\": %ld, ", beyond, beyond_not_nan);
  printf("\"asin_above_0.7\": %ld, \"asin_below_0.7\": %ld, \"asin_satan_low\": %ld, \"asin_satan_mid\": %ld, "
         "\"acos_neg_zero_is_half_pi\": %ld, ", as_hi, as_lo, satan_lo, satan_mid, acos_neg_zero);
  printf("\"atan2_q_low\": %ld, \"atan2_q_mid\": %ld, \"atan2_q_high\": %ld, \"atan2_q_zero\": %ld, \"atan2_q_inf\": %ld, "
         "\"f2i_min_int64\": %ld, ", q_lo, q_mid, q_hi, q_zero, q_inf, f_min);
  printf("\"families\": {");
  print_families("trig", T);
  print_families("asin", A);
  print_families("atan2", B);
  print_families("f2i", F, true);
  printf("}}\n");
  const long bad = bad_sin + bad_cos + bad_asin + bad_acos + bad_atan2 + bad_f2i + bad_u32 + beyond_not_nan;
  return bad ? 1 : 0;
}
