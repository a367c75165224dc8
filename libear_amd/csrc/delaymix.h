// delaymix.h — the maths of the delay matrix (include/earhip.h, group S) as plain C++ that the device kernels
// (delaymix_kernels.h), the C ABI (api_delaymix.hip) and a plain C++ program on the CPU (tests/cpp/delaymix_host.cpp) all
// compile, as src.h and iir.h are.  No HIP header is needed to include it.
//
//   - the checks of earhip_delaymix_create;
//   - the tables the kernel reads: the routes grouped by output row, in list order within a row, and the taps in one array;
//   - the history rule: the last H = max_r (D_r + T_r - 1) inputs of every row that is read, the tail of the old history
//     followed by the call's samples when the call is short (src.h's rule);
//   - the launch shape: the tile and how a tile's window lies in LDS;
//   - the host form of the operation: the header's definition with std::fmaf;
//   - the two designers (earhip_delaymix_fractional, earhip_delaymix_align).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "src.h"  // src_bessel_i0, src_history_entry

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EARHIP_DELAYMIX_HD __host__ __device__
#else
#define EARHIP_DELAYMIX_HD
#endif

namespace earhip {

constexpr int kDelaymixMaxRows = 64, kDelaymixMaxRoutes = 512, kDelaymixMaxTaps = 32, kDelaymixMaxDelay = 65536;
constexpr int kDelaymixThreads = 256, kDelaymixRun = 4;
constexpr int kDelaymixTile = kDelaymixThreads * kDelaymixRun;  // outputs of one tile
// a tile's window: its outputs, the T - 1 samples in front of them, up to 3 in front of those to the 16-byte boundary of the
// input row, rounded up to whole vectors
constexpr int kDelaymixWindow = (kDelaymixTile + kDelaymixMaxTaps - 1 + 3 + 3) / 4 * 4;
constexpr size_t kDelaymixMaxLaunch = (size_t)1 << 20;  // samples of one launch: every index of a launch stays far below 2^31

// one route as the create call gets it (the layout of earhip_delaymix_route)
struct DelaymixRoute {
  int in, out, delay, n_taps;
  float taps[kDelaymixMaxTaps];
};

// ---- what earhip_delaymix_create refuses, before anything is made (nullptr: fine) ------------------------------------------------
inline const char *delaymix_check_shape(int n_in, int n_out, int n_routes, size_t max_samples) {
  if (n_in < 1 || n_in > kDelaymixMaxRows) return "n_in must be in [1, 64]";
  if (n_out < 1 || n_out > kDelaymixMaxRows) return "n_out must be in [1, 64]";
  if (n_routes < 1 || n_routes > kDelaymixMaxRoutes) return "n_routes must be in [1, 512]";
  if (max_samples < 1) return "max_samples must be >= 1";
  return nullptr;
}
inline const char *delaymix_check_routes(int n_in, int n_out, int n_routes, const DelaymixRoute *routes) {
  for (int r = 0; r < n_routes; r++) {
    const DelaymixRoute &q = routes[r];
    if (q.in < 0 || q.in >= n_in) return "a route's in must be in [0, n_in)";
    if (q.out < 0 || q.out >= n_out) return "a route's out must be in [0, n_out)";
    if (q.delay < 0 || q.delay > kDelaymixMaxDelay) return "a route's delay must be in [0, 65536]";
    if (q.n_taps < 1 || q.n_taps > kDelaymixMaxTaps) return "a route's n_taps must be in [1, 32]";
    for (int j = 0; j < q.n_taps; j++)
      if (!std::isfinite(q.taps[j])) return "every tap must be finite";
  }
  return nullptr;
}

// ---- the tables -------------------------------------------------------------------------------------------------------------------
struct DelaymixEntry {
  int in, delay, n_taps, tap_at;  // tap_at: the route's first tap in the tap array
};
struct DelaymixTables {
  std::vector<DelaymixEntry> entries;  // the routes, grouped by output row, in ascending list index within a row
  std::vector<int> row_start;          // [n_out + 1]: the entries of output k are [row_start[k], row_start[k + 1])
  std::vector<float> taps;
  uint64_t reads = 0;  // bit c: some route reads input row c
  int history = 0;     // H
  int max_fan_in = 0;  // the most routes into one output
};
inline DelaymixTables delaymix_tables(int n_out, int n_routes, const DelaymixRoute *routes) {
  DelaymixTables t;
  t.row_start.assign((size_t)n_out + 1, 0);
  for (int k = 0; k < n_out; k++) {
    for (int r = 0; r < n_routes; r++) {
      const DelaymixRoute &q = routes[r];
      if (q.out != k) continue;
      t.entries.push_back({q.in, q.delay, q.n_taps, (int)t.taps.size()});
      t.taps.insert(t.taps.end(), q.taps, q.taps + q.n_taps);
      t.reads |= (uint64_t)1 << q.in;
      t.history = std::max(t.history, q.delay + q.n_taps - 1);
    }
    t.row_start[(size_t)k + 1] = (int)t.entries.size();
    t.max_fan_in = std::max(t.max_fan_in, t.row_start[(size_t)k + 1] - t.row_start[(size_t)k]);
  }
  return t;
}

// ---- the launch shape -------------------------------------------------------------------------------------------------------------
// a word of a tile's window in LDS: one idle word after every 32, so that lanes four words apart fall on different banks
EARHIP_DELAYMIX_HD inline int delaymix_pad(int w) { return w + (w >> 5); }
constexpr int kDelaymixLds = kDelaymixWindow + (kDelaymixWindow >> 5) + 1;  // floats

// ---- the host form ----------------------------------------------------------------------------------------------------------------
class DelaymixRef {
 public:
  DelaymixRef(int n_in, int n_out, int n_routes, const DelaymixRoute *routes)
      : n_in_(n_in), n_out_(n_out), t_(delaymix_tables(n_out, n_routes, routes)), H_(t_.history),
        hist_((size_t)n_in * (size_t)t_.history + 1, 0.0f), next_(hist_.size(), 0.0f) {}
  void reset() {
    std::fill(hist_.begin(), hist_.end(), 0.0f);
    clock_ = 0;
  }
  uint64_t clock() const { return clock_; }
  const DelaymixTables &tables() const { return t_; }
  // rows in[c] (n samples each; the pointer of a row no route reads is not looked at) -> out[k] (n samples each)
  void process(size_t n, const float *const *in, float *const *out) {
    const int64_t H = H_;
    for (int k = 0; k < n_out_; k++) {
      for (size_t i = 0; i < n; i++) {
        float acc = 0.0f;
        for (int e = t_.row_start[(size_t)k]; e < t_.row_start[(size_t)k + 1]; e++) {
          const DelaymixEntry &q = t_.entries[(size_t)e];
          const float *row = in[q.in], *hist = hist_.data() + (size_t)q.in * (size_t)H_, *h = t_.taps.data() + q.tap_at;
          for (int j = 0; j < q.n_taps; j++) {
            const int64_t at = (int64_t)i - q.delay - j;
            acc = std::fmaf(h[j], at < 0 ? hist[H + at] : row[at], acc);
          }
        }
        out[k][i] = acc;
      }
    }
    for (int c = 0; c < n_in_; c++) {
      if (!(t_.reads >> c & 1)) continue;
      const float *row = in[c], *hist = hist_.data() + (size_t)c * (size_t)H_;
      float *next = next_.data() + (size_t)c * (size_t)H_;
      for (int k = 0; k < H_; k++)
        next[k] = src_history_entry(H_, n, k, [&](int e) { return hist[e]; }, [&](uint64_t i) { return row[i]; });
    }
    hist_.swap(next_);
    clock_ += n;
  }

 private:
  int n_in_, n_out_;
  DelaymixTables t_;
  int H_;
  std::vector<float> hist_, next_;
  uint64_t clock_ = 0;
};

// ---- the designers ----------------------------------------------------------------------------------------------------------------
// a delay of `delay` samples as a whole delay and n_taps taps: n_taps = 1 rounds to the nearest sample; an even n_taps is a
// Kaiser-windowed sinc centred on the fraction, normalised to unit DC gain
inline const char *delaymix_fractional(double delay, int n_taps, double beta, int *whole, double *taps) {
  if (n_taps < 1 || n_taps > kDelaymixMaxTaps || (n_taps > 1 && n_taps % 2)) return "n_taps must be 1 or even, in [1, 32]";
  if (!std::isfinite(beta) || beta < 0.0) return "beta must be finite and >= 0";
  if (!std::isfinite(delay) || delay < 0.0) return "delay must be finite and >= 0";
  if (n_taps == 1) {
    const double w = std::floor(delay + 0.5);
    if (w > (double)kDelaymixMaxDelay) return "the whole delay must be at most 65536";
    *whole = (int)w, taps[0] = 1.0;
    return nullptr;
  }
  const int T = n_taps;
  const double c = (double)(T / 2 - 1), pi = 3.14159265358979323846;
  if (delay < c) return "delay must be at least n_taps / 2 - 1";
  const double w = std::floor(delay - c);
  if (w > (double)kDelaymixMaxDelay) return "the whole delay must be at most 65536";
  const double mu = delay - c - w, i0b = src_bessel_i0(beta);
  double sum = 0.0;
  for (int j = 0; j < T; j++) {
    const double t = (double)j - c - mu, y = pi * t, r = 2.0 * t / (double)T;
    const double sinc = y == 0.0 ? 1.0 : std::sin(y) / y;
    taps[j] = sinc * src_bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    sum += taps[j];
  }
  for (int j = 0; j < T; j++) taps[j] /= sum;
  *whole = (int)w;
  return nullptr;
}

// loudspeakers at distance_m[c]: the delay (in samples) and gain that bring each to the farthest one's arrival time and level
inline const char *delaymix_align(int n, const double *distance_m, double sample_rate, double speed_of_sound, double *delay_samples,
                                  double *gain) {
  if (n < 1) return "n must be >= 1";
  if (!std::isfinite(sample_rate) || !(sample_rate > 0.0)) return "sample_rate must be finite and > 0";
  if (!std::isfinite(speed_of_sound) || !(speed_of_sound > 0.0)) return "speed_of_sound must be finite and > 0";
  double far = 0.0;
  for (int c = 0; c < n; c++) {
    if (!std::isfinite(distance_m[c]) || !(distance_m[c] > 0.0)) return "every distance must be finite and > 0";
    far = std::max(far, distance_m[c]);
  }
  for (int c = 0; c < n; c++) {
    delay_samples[c] = (far - distance_m[c]) / speed_of_sound * sample_rate;
    gain[c] = distance_m[c] / far;
  }
  return nullptr;
}

}  // namespace earhip
