// src.h — the maths of the polyphase sample-rate converter (include/earhip.h, group P) as plain C++ that the device kernels
// (src_kernels.h), the C ABI (api_src.hip) and a plain C++ program on the CPU (tests/cpp/src_host.cpp) all compile, as iir.h and
// limiter.h are.  No HIP header is needed to include it.
//
//   - the index arithmetic.  The rate is L / M; output j reads input i_j = floor(j M / L) at phase p_j = (j M) mod L.  A call
//     never sees j: it starts at input clock N0 with the LEAD r0 = j0 M - N0 L in [0, M), j0 = ceil(N0 L / M) the first output
//     not yet produced, and its output q (= j0 + q of the stream) has  (j0 + q) M = N0 L + r0 + q M,  so relative to the call
//         i = floor((r0 + q M) / L),   p = (r0 + q M) mod L,
//     and the call of n inputs produces the q with i < n:  ceil((n L - r0) / M) of them, none when n L <= r0;
//   - the history rule: the last T - 1 inputs, the tail of the old history followed by the call's samples when the call is short;
//   - the table the kernel reads: c[p][k] = (float)h[p + k L] at p * pitch + k, the pitch odd;
//   - the launch shape: which of the table and a tile's input window fit the LDS;
//   - the host form of the operation: the header's definition with std::fmaf;
//   - the designer (earhip_src_design).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EARHIP_SRC_HD __host__ __device__
#else
#define EARHIP_SRC_HD
#endif

namespace earhip {

constexpr int kSrcMaxChannels = 64, kSrcMaxRatio = 1024, kSrcMaxTaps = 256, kSrcMaxTable = 32768;
constexpr int kSrcThreads = 256, kSrcRun = 4;
constexpr int kSrcTile = kSrcThreads * kSrcRun;  // outputs of one tile
constexpr int kSrcLdsFloats = 16384;             // what a workgroup may use: 64 KB
constexpr int kSrcMaxWindow = 12288;             // the padded window's share of it
constexpr size_t kSrcMaxLaunch = (size_t)1 << 20;  // inputs of one launch: its outputs (up to 1024 each) stay below 2^31

// ---- what earhip_src_create refuses, before anything is made (nullptr: fine) ---------------------------------------------------
inline int src_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b, b = t;
  }
  return a;
}
inline const char *src_check_ratio(int up, int down, int taps_per_phase) {
  if (up < 1 || up > kSrcMaxRatio) return "up must be in [1, 1024]";
  if (down < 1 || down > kSrcMaxRatio) return "down must be in [1, 1024]";
  if (src_gcd(up, down) != 1) return "up and down must have no common factor";
  if (taps_per_phase < 1 || taps_per_phase > kSrcMaxTaps) return "taps_per_phase must be in [1, 256]";
  if ((long)up * taps_per_phase > kSrcMaxTable) return "up * taps_per_phase must be at most 32768";
  return nullptr;
}
inline const char *src_check_shape(int channels, int up, int down, int taps_per_phase, size_t max_samples) {
  if (channels < 1 || channels > kSrcMaxChannels) return "channels must be in [1, 64]";
  if (const char *why = src_check_ratio(up, down, taps_per_phase)) return why;
  if (max_samples < 1) return "max_samples must be >= 1";
  return nullptr;
}
inline const char *src_check_taps(const double *taps, size_t count) {
  for (size_t i = 0; i < count; i++)
    if (!std::isfinite(taps[i]) || !std::isfinite((float)taps[i])) return "every tap must be finite (as a float32 too)";
  return nullptr;
}

// ---- the index arithmetic -------------------------------------------------------------------------------------------------------
// the lead of a call that starts at input clock N0: j0 M - N0 L, j0 = ceil(N0 L / M)
inline unsigned src_lead(uint64_t clock, int L, int M) {
  const uint64_t rem = ((clock % (uint64_t)M) * (uint64_t)L) % (uint64_t)M;
  return (unsigned)((uint64_t)M - rem) % (unsigned)M;
}
// the outputs of a call of n inputs that starts with lead r0
inline size_t src_outputs(size_t n, unsigned r0, int L, int M) {
  const uint64_t fed = (uint64_t)n * (uint64_t)L;
  return fed > r0 ? (size_t)((fed - r0 + (uint64_t)M - 1) / (uint64_t)M) : 0;
}
// the most outputs of any call of up to n inputs (the lead only takes away)
inline size_t src_max_outputs(size_t n, int L, int M) { return src_outputs(n, 0, L, M); }
// output q of a call with lead r0: input i relative to the call's first sample, phase p
EARHIP_SRC_HD inline void src_index(unsigned r0, uint64_t q, int L, int M, uint64_t *i, int *p) {
  const uint64_t u = (uint64_t)r0 + q * (uint64_t)M;
  *i = u / (uint64_t)L;
  *p = (int)(u % (uint64_t)L);
}

// ---- the history rule -----------------------------------------------------------------------------------------------------------
// entry k of the history after a call of n inputs (H = T - 1 entries, entry H + i is sample i < 0 of the next call): sample
// n - H + k of the call, from the old history where that is negative
template <typename Old, typename In>
EARHIP_SRC_HD inline float src_history_entry(int H, uint64_t n, int k, Old old, In in) {
  const int64_t i = (int64_t)n - H + k;
  return i < 0 ? old((int)(H + i)) : in((uint64_t)i);
}

// ---- the table --------------------------------------------------------------------------------------------------------------------
inline int src_pitch(int T) { return T | 1; }  // odd: rows p, p + 1 .. start on different banks
inline void src_table_make(const double *h, int L, int T, float *table) {
  const int pitch = src_pitch(T);
  for (int p = 0; p < L; p++)
    for (int k = 0; k < pitch; k++) table[(size_t)p * pitch + k] = k < T ? (float)h[p + (size_t)k * L] : 0.0f;
}

// ---- the launch shape -------------------------------------------------------------------------------------------------------------
struct SrcShape {
  int pitch = 0;
  int window = 0;       // input samples a tile's outputs read: floor(((tile - 1) M + L - 1) / L) + T
  int window_lds = 0;   // floats of the padded window in LDS; 0: the window is read through the caches
  int table_lds = 0;    // floats of the table in LDS; 0: the table is read through the caches
  int tile_in = 0;      // ceil(tile M / L): a tile's length in inputs
  size_t lds_bytes() const { return sizeof(float) * ((size_t)window_lds + (size_t)table_lds); }
};
EARHIP_SRC_HD inline int src_pad(int w) { return w + (w >> 5); }  // a word of the window in LDS: one idle word after every 32
inline SrcShape src_shape(int L, int M, int T) {
  SrcShape s;
  s.pitch = src_pitch(T);
  const long span = ((long)(kSrcTile - 1) * M + L - 1) / L + T;
  s.tile_in = (int)(((long)kSrcTile * M + L - 1) / L);
  s.window = (int)std::min<long>(span, 0x7fffffff);
  if (span <= kSrcMaxWindow && src_pad((int)span) + 1 <= kSrcMaxWindow) s.window_lds = src_pad((int)span) + 1;
  const long table = (long)L * s.pitch;
  if (table + s.window_lds <= kSrcLdsFloats) s.table_lds = (int)table;
  return s;
}

// ---- the host form ----------------------------------------------------------------------------------------------------------------
// y = fmaf(c[p][T - 1], x[i - (T - 1)], .. fmaf(c[p][0], x[i], +0.0f)): the header's chain; x(k) is x[i - k]
template <typename X>
EARHIP_SRC_HD inline float src_dot(const float *c, int T, X x) {
  float acc = 0.0f;
  for (int k = 0; k < T; k++) acc = fmaf(c[k], x(k), acc);
  return acc;
}

class SrcRef {
 public:
  SrcRef(int channels, int L, int M, int T, const double *h)
      : C_(channels), L_(L), M_(M), T_(T), H_(T - 1), pitch_(src_pitch(T)), table_((size_t)L * src_pitch(T)),
        hist_((size_t)channels * (size_t)(T - 1) + 1, 0.0f), next_(hist_.size(), 0.0f) {
    src_table_make(h, L, T, table_.data());
  }
  void reset() {
    std::fill(hist_.begin(), hist_.end(), 0.0f);
    clock_ = 0;
  }
  uint64_t clock() const { return clock_; }
  size_t next_out(size_t n) const { return src_outputs(n, src_lead(clock_, L_, M_), L_, M_); }
  // rows in[c * in_stride + i], i < n -> out[c * out_stride + q], q < the returned count (the caller has made room)
  size_t process(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    const unsigned r0 = src_lead(clock_, L_, M_);
    const size_t n_out = src_outputs(n, r0, L_, M_);
    for (int c = 0; c < C_; c++) {
      const float *row = in + (size_t)c * in_stride;
      const float *hist = hist_.data() + (size_t)c * H_;
      const int H = H_;
      for (size_t q = 0; q < n_out; q++) {
        uint64_t i;
        int p;
        src_index(r0, q, L_, M_, &i, &p);
        out[(size_t)c * out_stride + q] = src_dot(table_.data() + (size_t)p * pitch_, T_, [&](int k) {
          const int64_t at = (int64_t)i - k;
          return at < 0 ? hist[H + at] : row[at];
        });
      }
      float *next = next_.data() + (size_t)c * H_;
      for (int k = 0; k < H_; k++)
        next[k] = src_history_entry(H_, n, k, [&](int e) { return hist[e]; }, [&](uint64_t i) { return row[i]; });
    }
    hist_.swap(next_);
    clock_ += n;
    return n_out;
  }

 private:
  int C_, L_, M_, T_, H_, pitch_;
  std::vector<float> table_, hist_, next_;
  uint64_t clock_ = 0;
};

// ---- the designer -----------------------------------------------------------------------------------------------------------------
// I0 by its power series: the terms ((x / 2)^k / k!)^2 are positive, so the sum loses nothing to cancellation
inline double src_bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 1000; k++) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}
// a Kaiser-windowed sinc of length L T, cutoff `cutoff / max(L, M)` of the prototype's Nyquist, unit DC gain, times L
inline const char *src_design(int up, int down, int taps_per_phase, double beta, double cutoff, double *out) {
  if (const char *why = src_check_ratio(up, down, taps_per_phase)) return why;
  if (!std::isfinite(beta) || beta < 0.0) return "beta must be finite and >= 0";
  if (!std::isfinite(cutoff) || !(cutoff > 0.0) || cutoff > 1.0) return "cutoff must be in (0, 1]";
  const int n = up * taps_per_phase;
  const double fc = cutoff / (double)std::max(up, down), alpha = 0.5 * (double)(n - 1), pi = 3.14159265358979323846;
  const double i0b = src_bessel_i0(beta);
  double sum = 0.0;
  for (int i = 0; i < n; i++) {
    const double m = (double)i - alpha, y = pi * fc * m;
    const double sinc = y == 0.0 ? 1.0 : std::sin(y) / y;
    const double r = n > 1 ? m / alpha : 0.0;
    const double w = src_bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    out[i] = fc * sinc * w;
    sum += out[i];
  }
  for (int i = 0; i < n; i++) out[i] = out[i] / sum * (double)up;
  return nullptr;
}

}  // namespace earhip
