// true_peak.h — the maths of the true-peak meter (include/earhip.h, group L: ITU-R BS.1770-4 annex 2) as plain C++ that the
// device kernels (true_peak_kernels.h), the C ABI (api_loudness.hip) and a plain C++ program on the CPU
// (tests/cpp/true_peak_host.cpp) all compile, like loudness.h beside it.  No HIP header is needed to include it.
//
//   - the polyphase interpolator: y[phases n + p] = sum over k of h[p][k] x[n - k], float32, k = 0 first, one fused
//     multiply-add per tap from an accumulator of zero: tp_dot for any number of taps (k_true_peak_any), tp_dot_n for a number
//     known at compile time (k_true_peak_4x12 with n = 12, where the unrolled loop indexes registers); the CPU meter below
//     takes the same one of the two as the device does for its table's shape.  Every y is a fixed function of `taps` input
//     samples, so how a stream is cut into calls cannot change a bit of it;
//   - the two maxima (|y| and |x|) ignore NaN and are exact, so neither their order nor their grouping matters;
//   - a one-channel meter on the CPU that carries taps - 1 samples of history and the peaks of the open 100 ms step;
//   - the table a meter or a limiter is made with (TpTable): the caller's earhip_true_peak checked, or annex 2's.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/earhip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EARHIP_TP_HD __host__ __device__
#define EARHIP_TP_UNROLL _Pragma("unroll")
#else
#define EARHIP_TP_HD
#define EARHIP_TP_UNROLL
#endif

namespace earhip {

constexpr int kTpMaxPhases = 8, kTpMaxTaps = 64;

// BS.1770-4 annex 2, phases 0 and 1, times 8192 (phases 2 and 3 are phases 1 and 0 reversed): exact in float32
static const int kTruePeakTable8192[2][12] = {
    {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68},
    {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155},
};

inline void true_peak_default_table(double h[4][12]) {
  for (int k = 0; k < 12; k++) {
    h[0][k] = kTruePeakTable8192[0][k] / 8192.0;
    h[1][k] = kTruePeakTable8192[1][k] / 8192.0;
    h[2][k] = kTruePeakTable8192[1][11 - k] / 8192.0;
    h[3][k] = kTruePeakTable8192[0][11 - k] / 8192.0;
  }
}

// The table as the kernels take it: v [phases][taps] in float32 for the device, and h, the same numbers where the shape is 4 x 12
// (the kernels of that shape take them as an argument), else zero.
struct TpTable { int phases = 0, taps = 0; std::vector<float> v; float h[4][12] = {}; };

// The caller's table (tp->coeffs) or, without one (tp or tp->coeffs NULL), annex 2's for the rates it was designed for.
// Returns why the table is refused, or nullptr.
inline const char *tp_table_make(const earhip_true_peak *tp, int sample_rate, TpTable *t) {
  if (tp && tp->coeffs) {
    if (!(tp->phases >= 1 && tp->phases <= kTpMaxPhases)) return "true peak: phases must be in [1, 8]";
    if (!(tp->taps >= 1 && tp->taps <= kTpMaxTaps)) return "true peak: taps must be in [1, 64]";
    t->phases = tp->phases, t->taps = tp->taps;
    t->v.resize((size_t)t->phases * (size_t)t->taps);
    for (size_t i = 0; i < t->v.size(); i++) {
      if (!(std::isfinite(tp->coeffs[i]) && std::isfinite((float)tp->coeffs[i]))) return "true peak: coefficients must be finite";
      t->v[i] = (float)tp->coeffs[i];
    }
  } else {
    if (sample_rate != 44100 && sample_rate != 48000)
      return "the built-in true-peak table is 4x oversampling for 44100 and 48000 Hz: another rate must bring its own";
    double h[4][12];
    true_peak_default_table(h);
    t->phases = 4, t->taps = 12;
    t->v.resize(48);
    for (int i = 0; i < 48; i++) t->v[(size_t)i] = (float)h[i / 12][i % 12];
  }
  if (t->phases == 4 && t->taps == 12) std::memcpy(t->h, t->v.data(), sizeof(t->h));
  else std::memset(t->h, 0, sizeof(t->h));
  return nullptr;
}

// one output of one phase: x(k) = x[n - k]
template <typename Get>
EARHIP_TP_HD inline float tp_dot(const float *h, int taps, Get x) {
  float acc = 0.0f;
  for (int k = 0; k < taps; k++) acc = fmaf(h[k], x(k), acc);
  return acc;
}

template <int kTaps, typename Get>
EARHIP_TP_HD inline float tp_dot_n(const float *h, Get x) {
  float acc = 0.0f;
  EARHIP_TP_UNROLL
  for (int k = 0; k < kTaps; k++) acc = fmaf(h[k], x(k), acc);
  return acc;
}

// m is never NaN; a NaN v leaves it alone
EARHIP_TP_HD inline float tp_absmax(float m, float v) { return fmaxf(m, fabsf(v)); }

// One channel on the CPU.  Finished steps are appended to tp_steps / sp_steps; tp_open / sp_open are the open step's.
struct TruePeakChannelRef {
  int phases, taps, step;
  std::vector<float> h;     // [phases][taps]
  std::vector<float> hist;  // the last taps - 1 samples, oldest first
  size_t clock = 0;
  float tp_open = 0.0f, sp_open = 0.0f;
  std::vector<float> tp_steps, sp_steps;

  TruePeakChannelRef(int phases_, int taps_, const double *table, int step_samples)
      : phases(phases_), taps(taps_), step(step_samples), h((size_t)phases_ * (size_t)taps_), hist((size_t)taps_ - 1, 0.0f) {
    for (size_t i = 0; i < h.size(); i++) h[i] = (float)table[i];
  }

  void process(const float *x, size_t n) {
    const int halo = taps - 1;
    std::vector<float> w((size_t)halo + n);
    for (int i = 0; i < halo; i++) w[(size_t)i] = hist[(size_t)i];
    for (size_t i = 0; i < n; i++) w[(size_t)halo + i] = x[i];
    for (size_t i = 0; i < n; i++) {
      const float *at = w.data() + halo + i;
      for (int p = 0; p < phases; p++) {
        const float *hp = h.data() + (size_t)p * (size_t)taps;
        const auto xk = [&](int k) { return at[-k]; };
        tp_open = tp_absmax(tp_open, phases == 4 && taps == 12 ? tp_dot_n<12>(hp, xk) : tp_dot(hp, taps, xk));
      }
      sp_open = tp_absmax(sp_open, at[0]);
      if (++clock % (size_t)step == 0) {
        tp_steps.push_back(tp_open), sp_steps.push_back(sp_open);
        tp_open = sp_open = 0.0f;
      }
    }
    for (int i = 0; i < halo; i++) hist[(size_t)i] = w[n + (size_t)i];
  }
};

}  // namespace earhip
