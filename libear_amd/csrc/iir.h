// iir.h — the maths of the biquad filter matrix (include/earhip.h, group O) as plain C++ that the device kernels
// (iir_kernels.h), the C ABI (api_iir.hip) and a plain C++ program on the CPU (tests/cpp/iir_host.cpp) all compile, as
// loudness.h and limiter.h are.  No HIP header is needed to include it.
//
//   - the cascade step: up to 8 biquads in transposed direct form II, float64 arithmetic on float32 samples, every multiply-add
//     ONE rounding.  The state of a route is 2 S numbers (s1, s2 of each section), and as in loudness.h the state after a run is
//     linear in the state before it:  S_end = Phi^len S_start + e,  e = the end state of the same run from the zero state;
//   - Phi is BLOCK LOWER-TRIANGULAR (section k reads the sections before it only): row i has columns 0 .. (i | 1).  Only
//     Phi^(Lc 2^d), d = 0 .. 6, are kept per route: Phi^Lc made in long double by running the cascade on the unit states, then
//     squared in long double, every matrix rounded once;
//   - the chunk plan of a launch: chunks of Lc samples on the stage's own clock grid.  The first chunk of a launch (whole or
//     partial) starts from the carried state, so pass 1 runs it from that TRUE state; the last chunk only needs pass 2, which
//     also leaves the state the next launch starts from; the whole chunks between them are a scan;
//   - a sequential reference and the chunked form on the host, the latter in the order of operations the kernels use;
//   - the RBJ cookbook designer (earhip_iir_design).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EARHIP_IIR_HD __host__ __device__
#else
#define EARHIP_IIR_HD
#endif
#if defined(__clang__)
#define EARHIP_IIR_UNROLL _Pragma("unroll")
#else
#define EARHIP_IIR_UNROLL _Pragma("GCC unroll 16")
#endif

namespace earhip {

constexpr int kIirMaxChannels = 64, kIirMaxRoutes = 512, kIirMaxSections = 8;
constexpr int kIirMaxState = 2 * kIirMaxSections;                 // doubles of a route's state
constexpr int kIirMat = kIirMaxState * kIirMaxState;              // doubles of one transition matrix, row-major [16][16]
constexpr int kIirChunk = 256;                                    // Lc
constexpr int kIirScanLanes = 64;                                 // chunks per scan group: one wave
constexpr int kIirScanWaves = 4, kIirGroupsPerWave = 8;           // the propagation's workgroup
constexpr int kIirScanGroups = kIirScanWaves * kIirGroupsPerWave; // scan groups chained per workgroup
constexpr int kIirMaxWhole = kIirScanGroups * kIirScanLanes;      // whole chunks between the first and the last of a launch
constexpr int kIirMaxChunks = kIirMaxWhole + 2;                   // chunks of one launch (cap of the scratch)
constexpr int kIirPowers = 7;                                     // Phi^(Lc 2^d), d = 0 .. 6
// the most samples of one launch, whatever the clock: chunk 0 may start up to Lc - 1 samples before the launch
constexpr size_t kIirMaxLaunch = (size_t)(kIirMaxChunks - 1) * kIirChunk;

struct IirRoute {
  int in = 0, out = 0;
  double gain = 0.0;
  int S = 0;
  double c[kIirMaxSections][5];  // [section][b0 b1 b2 a1 a2]
};

template <typename T>
struct IirCoeffs {
  T c[kIirMaxSections][5];
};
template <typename T>
struct IirState {
  T s[kIirMaxState];  // s1, s2 of section 0; s1, s2 of section 1; ...
};

// One sample through the first S sections:  y = b0 x + s1;  s1 = b1 x - a1 y + s2;  s2 = b2 x - a2 y.  S = 0: y = x.
// (Unrolled over the 8 sections with a guard each, so that the state stays in registers on the device.)
template <typename T>
EARHIP_IIR_HD inline T iir_step(const IirCoeffs<T> &k, int S, IirState<T> &st, T x) {
  using std::fma;
  T y = x;
  EARHIP_IIR_UNROLL
  for (int i = 0; i < kIirMaxSections; i++) {
    if (i < S) {
      const T v = y;
      y = fma(k.c[i][0], v, st.s[2 * i]);
      st.s[2 * i] = fma(-k.c[i][3], y, fma(k.c[i][1], v, st.s[2 * i + 1]));
      st.s[2 * i + 1] = fma(-k.c[i][4], y, k.c[i][2] * v);
    }
  }
  return y;
}

EARHIP_IIR_HD inline IirState<double> iir_zero_state() {
  IirState<double> z;
  EARHIP_IIR_UNROLL
  for (int i = 0; i < kIirMaxState; i++) z.s[i] = 0.0;
  return z;
}

// M v + e for a block lower-triangular M (row-major [16][16]); rows at or beyond n2 = 2 S are zero
EARHIP_IIR_HD inline IirState<double> iir_advance(const double *M, int n2, const IirState<double> &v, const IirState<double> &e) {
  IirState<double> r;
  EARHIP_IIR_UNROLL
  for (int i = 0; i < kIirMaxState; i++) {
    double a = 0.0;
    if (i < n2) {
      a = e.s[i];
      EARHIP_IIR_UNROLL
      for (int j = 0; j < kIirMaxState; j++)
        if (j <= (i | 1)) a = std::fma(M[kIirMaxState * i + j], v.s[j], a);
    }
    r.s[i] = a;
  }
  return r;
}

// out [kIirPowers][kIirMat]: Phi^(Lc 2^d).  Column q of Phi^Lc is the state Lc samples after the unit state q with no input.
inline void iir_state_powers(const double coeffs[][5], int S, double *out) {
  IirCoeffs<long double> k;
  for (int s = 0; s < kIirMaxSections; s++)
    for (int i = 0; i < 5; i++) k.c[s][i] = s < S ? (long double)coeffs[s][i] : 0.0L;
  const int n2 = 2 * S;
  std::vector<long double> A((size_t)kIirMat, 0.0L), B((size_t)kIirMat);
  for (int q = 0; q < n2; q++) {
    IirState<long double> col;
    for (int i = 0; i < kIirMaxState; i++) col.s[i] = i == q ? 1.0L : 0.0L;
    for (int t = 0; t < kIirChunk; t++) (void)iir_step(k, S, col, 0.0L);
    for (int i = 0; i < n2; i++) A[(size_t)(kIirMaxState * i + q)] = col.s[i];
  }
  for (int d = 0; d < kIirPowers; d++) {
    for (int i = 0; i < kIirMat; i++) out[(size_t)d * kIirMat + i] = (double)A[(size_t)i];
    if (d + 1 == kIirPowers) break;
    for (int i = 0; i < kIirMaxState; i++)
      for (int j = 0; j < kIirMaxState; j++) {
        long double a = 0.0L;
        for (int m = 0; m < n2; m++) a += A[(size_t)(kIirMaxState * i + m)] * A[(size_t)(kIirMaxState * m + j)];
        B[(size_t)(kIirMaxState * i + j)] = a;
      }
    A.swap(B);
  }
}

// ---- what earhip_iir_create refuses, before anything is made (nullptr: fine) -------------------------------------------------
inline const char *iir_check_route(const IirRoute &r, int n_in, int n_out) {
  if (r.in < 0 || r.in >= n_in) return "a route's in must be in [0, n_in)";
  if (r.out < 0 || r.out >= n_out) return "a route's out must be in [0, n_out)";
  if (!std::isfinite(r.gain)) return "a route's gain must be finite";
  if (r.S < 0 || r.S > kIirMaxSections) return "a route's n_sections must be in [0, 8]";
  for (int s = 0; s < r.S; s++) {
    for (int i = 0; i < 5; i++)
      if (!std::isfinite(r.c[s][i])) return "a route's coefficients must be finite";
    const double a1 = r.c[s][3], a2 = r.c[s][4];
    if (!(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2)) return "a section is not stable: it needs |a2| < 1 and |a1| < 1 + a2";
  }
  return nullptr;
}
inline const char *iir_check_shape(int n_in, int n_out, int n_routes, size_t max_samples) {
  if (n_in < 1 || n_in > kIirMaxChannels) return "n_in must be in [1, 64]";
  if (n_out < 1 || n_out > kIirMaxChannels) return "n_out must be in [1, 64]";
  if (n_routes < 1 || n_routes > kIirMaxRoutes) return "n_routes must be in [1, 512]";
  if (max_samples < 1) return "max_samples must be >= 1";
  return nullptr;
}

// ---- the chunk plan of one launch ------------------------------------------------------------------------------------------
struct IirPlan {
  unsigned n = 0;        // samples of the launch (<= kIirMaxLaunch)
  unsigned off0 = 0;     // clock of sample 0 modulo Lc: chunk 0 starts off0 samples BEFORE sample 0
  unsigned nchunks = 0;  // >= 1
  unsigned whole() const { return nchunks >= 2 ? nchunks - 2 : 0; }  // chunks 1 .. nchunks - 2: the scan's
};
inline IirPlan iir_plan(unsigned long long clock, size_t n) {
  IirPlan p;
  p.n = (unsigned)n;
  p.off0 = (unsigned)(clock % (unsigned long long)kIirChunk);
  p.nchunks = (unsigned)((p.off0 + n + kIirChunk - 1) / kIirChunk);
  return p;
}
// samples [lo, hi) of the launch are chunk c's
EARHIP_IIR_HD inline void iir_chunk_range(unsigned n, unsigned off0, unsigned c, int &lo, int &hi) {
  const int b0 = (int)c * kIirChunk - (int)off0;
  lo = b0 > 0 ? b0 : 0;
  hi = b0 + kIirChunk < (int)n ? b0 + kIirChunk : (int)n;
}

// ---- the bank on the CPU, in the two forms the tests compare -----------------------------------------------------------------
struct IirBankRef {
  int n_in, n_out;
  std::vector<IirRoute> routes;
  std::vector<IirCoeffs<double>> k;
  std::vector<IirState<double>> st;
  std::vector<double> Q;  // [routes][kIirPowers][kIirMat]
  unsigned long long clock = 0;

  IirBankRef(int n_in_, int n_out_, const std::vector<IirRoute> &routes_) : n_in(n_in_), n_out(n_out_), routes(routes_) {
    k.resize(routes.size());
    st.assign(routes.size(), iir_zero_state());
    Q.resize(routes.size() * (size_t)kIirPowers * kIirMat);
    for (size_t r = 0; r < routes.size(); r++) {
      for (int s = 0; s < kIirMaxSections; s++)
        for (int i = 0; i < 5; i++) k[r].c[s][i] = s < routes[r].S ? routes[r].c[s][i] : 0.0;
      iir_state_powers(routes[r].c, routes[r].S, &Q[r * (size_t)kIirPowers * kIirMat]);
    }
  }

  // the header's sum: float64 from +0.0, one fused multiply-add per route in ascending list index, one rounding
  template <typename Run>
  void mix(size_t n, float *out, size_t out_stride, Run run) {
    std::vector<double> acc(n);
    for (int o = 0; o < n_out; o++) {
      std::fill(acc.begin(), acc.end(), 0.0);
      for (size_t r = 0; r < routes.size(); r++)
        if (routes[r].out == o) run(r, acc.data());
      for (size_t i = 0; i < n; i++) out[(size_t)o * out_stride + i] = (float)acc[i];
    }
  }

  // sample by sample
  void process_sequential(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    mix(n, out, out_stride, [&](size_t r, double *acc) {
      const float *x = in + (size_t)routes[r].in * in_stride;
      for (size_t i = 0; i < n; i++) acc[i] = std::fma(routes[r].gain, iir_step(k[r], routes[r].S, st[r], (double)x[i]), acc[i]);
    });
    clock += n;
  }

  // the decomposition the kernels run, launch by launch, in their order of operations
  void process_chunked(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    for (size_t at = 0; at < n;) {
      const size_t len = std::min(kIirMaxLaunch, n - at);
      launch(len, in + at, in_stride, out + at, out_stride);
      at += len;
    }
  }

  void launch(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    const IirPlan p = iir_plan(clock, n);
    mix(n, out, out_stride, [&](size_t r, double *acc) {
      const int S = routes[r].S, n2 = 2 * S;
      const float *x = in + (size_t)routes[r].in * in_stride;
      const double *Qr = &Q[r * (size_t)kIirPowers * kIirMat];
      std::vector<IirState<double>> start(p.nchunks, iir_zero_state());
      start[0] = st[r];
      if (p.nchunks >= 2 && S > 0) {
        // pass 1: chunk 0 from the true state, the whole chunks from zero
        std::vector<IirState<double>> e(p.nchunks - 1, iir_zero_state());
        e[0] = st[r];
        for (unsigned c = 0; c + 1 < p.nchunks; c++) {
          int lo, hi;
          iir_chunk_range(p.n, p.off0, c, lo, hi);
          for (int i = lo; i < hi; i++) (void)iir_step(k[r], S, e[c], (double)x[i]);
        }
        start[1] = e[0];
        // the scan over the whole chunks, in groups of 64: Hillis-Steele, the groups chained, then the carry by the bits of
        // the lane's distance
        const unsigned m = p.whole();
        IirState<double> carry = e[0];
        for (unsigned g0 = 0; g0 < m; g0 += kIirScanLanes) {
          const unsigned cnt = std::min<unsigned>(kIirScanLanes, m - g0);
          IirState<double> c[kIirScanLanes];
          for (unsigned l = 0; l < kIirScanLanes; l++) c[l] = l < cnt ? e[1 + g0 + l] : iir_zero_state();
          for (int d = 0; d < 6; d++)
            for (int l = kIirScanLanes - 1; l >= (1 << d); l--) c[l] = iir_advance(Qr + (size_t)d * kIirMat, n2, c[l - (1 << d)], c[l]);
          for (unsigned l = 0; l < cnt; l++) {
            IirState<double> v = carry;
            for (int d = 0; d < kIirPowers; d++)
              if (((l + 1) >> d) & 1) v = iir_advance(Qr + (size_t)d * kIirMat, n2, v, iir_zero_state());
            for (int i = 0; i < kIirMaxState; i++) v.s[i] = v.s[i] + c[l].s[i];
            start[2 + g0 + l] = v;
          }
          carry = iir_advance(Qr + (size_t)6 * kIirMat, n2, carry, c[kIirScanLanes - 1]);
        }
      }
      // pass 2: every chunk from its true start state
      for (unsigned c = 0; c < p.nchunks; c++) {
        int lo, hi;
        iir_chunk_range(p.n, p.off0, c, lo, hi);
        IirState<double> s = start[c];
        for (int i = lo; i < hi; i++) acc[i] = std::fma(routes[r].gain, iir_step(k[r], S, s, (double)x[i]), acc[i]);
        if (c + 1 == p.nchunks) st[r] = s;
      }
    });
    clock += n;
  }

  void reset() {
    std::fill(st.begin(), st.end(), iir_zero_state());
    clock = 0;
  }
};

// ---- the designer: the RBJ cookbook's biquads, normalised by a0 ----------------------------------------------------------------
enum { kIirLowpass = 0, kIirHighpass = 1, kIirPeaking = 2, kIirLowShelf = 3, kIirHighShelf = 4 };
inline const char *iir_design(int kind, double fs, double f0, double q, double gain_db, double out[5]) {
  if (kind < kIirLowpass || kind > kIirHighShelf) return "kind must be 0 lowpass, 1 highpass, 2 peaking, 3 low shelf or 4 high shelf";
  if (!(std::isfinite(fs) && std::isfinite(f0) && std::isfinite(q) && std::isfinite(gain_db))) return "the arguments must be finite";
  if (!(fs > 0.0)) return "sample_rate must be > 0";
  if (!(f0 > 0.0 && f0 < 0.5 * fs)) return "f0 must lie in (0, sample_rate / 2)";
  if (!(q > 0.0)) return "q must be > 0";
  const double pi = 3.14159265358979323846;
  const double w0 = 2.0 * pi * f0 / fs, cs = std::cos(w0), sn = std::sin(w0), alpha = sn / (2.0 * q);
  const double hs = std::sin(0.5 * w0), omc = 2.0 * hs * hs;  // 1 - cos w0 without the cancellation
  const double A = std::pow(10.0, gain_db / 40.0), rA = 2.0 * std::sqrt(A) * alpha;
  double b0, b1, b2, a0, a1, a2;
  switch (kind) {
    case kIirLowpass:
      b0 = 0.5 * omc, b1 = omc, b2 = 0.5 * omc, a0 = 1.0 + alpha, a1 = -2.0 * cs, a2 = 1.0 - alpha;
      break;
    case kIirHighpass:
      b0 = 0.5 * (1.0 + cs), b1 = -(1.0 + cs), b2 = 0.5 * (1.0 + cs), a0 = 1.0 + alpha, a1 = -2.0 * cs, a2 = 1.0 - alpha;
      break;
    case kIirPeaking:
      b0 = 1.0 + alpha * A, b1 = -2.0 * cs, b2 = 1.0 - alpha * A, a0 = 1.0 + alpha / A, a1 = -2.0 * cs, a2 = 1.0 - alpha / A;
      break;
    case kIirLowShelf:
      b0 = A * ((A + 1.0) - (A - 1.0) * cs + rA), b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cs), b2 = A * ((A + 1.0) - (A - 1.0) * cs - rA);
      a0 = (A + 1.0) + (A - 1.0) * cs + rA, a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cs), a2 = (A + 1.0) + (A - 1.0) * cs - rA;
      break;
    default:
      b0 = A * ((A + 1.0) + (A - 1.0) * cs + rA), b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cs), b2 = A * ((A + 1.0) + (A - 1.0) * cs - rA);
      a0 = (A + 1.0) - (A - 1.0) * cs + rA, a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cs), a2 = (A + 1.0) - (A - 1.0) * cs - rA;
      break;
  }
  out[0] = b0 / a0, out[1] = b1 / a0, out[2] = b2 / a0, out[3] = a1 / a0, out[4] = a2 / a0;
  return nullptr;
}

}  // namespace earhip
