// limiter.h — the maths of the look-ahead limiter (include/earhip.h, group N) as plain C++ that the device kernels
// (limiter_kernels.h), the C ABI (api_limiter.hip) and a plain C++ program on the CPU (tests/cpp/limiter_host.cpp) all compile,
// like true_peak.h beside it, whose interpolator the detector is.  No HIP header is needed to include it.
//
//   - the required gain r = min(1, c / e): one correctly rounded float32 division, e = 0 gives 1, e = +inf gives 0;
//   - the smoothing sum s = m[n] + m[n-1] + .. + m[n-L], in that order from +0.0f, and the final g = min(s / (float)K, r[n-L]):
//     every g is a fixed function of M - 1 + L + 1 values of r, so how a stream is cut into calls cannot change a bit of it;
//   - the sliding minimum is exact, so any algorithm gives the same bits: the kernels take it by doubling in LDS, the CPU
//     limiter below by the definition;
//   - a limiter over all channels on the CPU that carries the histories the header lists.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "true_peak.h"

namespace earhip {

constexpr int kLimMaxChannels = 64, kLimMinLookahead = 8, kLimMaxLookahead = 1024, kLimMaxHold = 8192;

// what earhip_limiter_create refuses, before anything is made (nullptr: fine); phases / taps: the table's shape (detect = 1)
inline const char *limiter_check_config(int n_channels, int sample_rate, float ceiling, int lookahead, int hold, int detect,
                                        size_t max_samples) {
  if (n_channels < 1 || n_channels > kLimMaxChannels) return "n_channels must be in [1, 64]";
  if (sample_rate <= 0) return "sample_rate must be > 0";
  if (!(std::isfinite(ceiling) && ceiling > 0.0f)) return "ceiling must be finite and > 0";
  if (lookahead < kLimMinLookahead || lookahead > kLimMaxLookahead) return "lookahead must be in [8, 1024]";
  if (hold < 0 || hold > kLimMaxHold) return "hold must be in [0, 8192]";
  if (detect != 0 && detect != 1) return "detect must be 0 (sample peak) or 1 (true peak)";
  if (max_samples < 1) return "max_samples must be >= 1";
  return nullptr;
}

// the lengths that follow from a configuration
struct LimiterShape {
  int L = 0, H = 0, D = 0, M = 0, K = 0, taps = 0, phases = 0;
  int latency() const { return D + L; }
  int x_hist() const { return std::max(D + L, taps - 1); }  // samples per channel: the delay line and the interpolator's window
  int r_hist() const { return M - 1 + L; }                  // values of r
};
inline LimiterShape limiter_shape(int lookahead, int hold, int detect, int phases, int taps) {
  LimiterShape s;
  s.L = lookahead, s.H = hold;
  s.phases = detect ? phases : 0, s.taps = detect ? taps : 0;
  s.D = s.taps / 2;
  s.M = lookahead + 2 + hold;
  s.K = lookahead + 1;
  return s;
}

EARHIP_TP_HD inline float lim_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

// e is never NaN (tp_absmax)
EARHIP_TP_HD inline float lim_required_gain(float c, float e) { return e > 0.0f ? fminf(1.0f, lim_div(c, e)) : 1.0f; }

// N samples side by side (independent chains of adds): m(i, k) = m[n_i - k]
template <int N, typename Get>
EARHIP_TP_HD inline void lim_sum(int K, float (&s)[N], Get m) {
  for (int i = 0; i < N; i++) s[i] = 0.0f;
  for (int k = 0; k < K; k++)
    for (int i = 0; i < N; i++) s[i] = s[i] + m(i, k);
}

EARHIP_TP_HD inline float lim_gain(float s, int K, float r_delayed) { return fminf(lim_div(s, (float)K), r_delayed); }

// All channels on the CPU.  process() may be called with any n >= 0.
struct LimiterRef {
  int C;
  float c;
  LimiterShape sh;
  std::vector<float> h;      // [phases][taps]
  std::vector<float> xhist;  // [C][x_hist], oldest first
  std::vector<float> rhist;  // [r_hist], oldest first
  float min_gain = 1.0f;
  uint64_t limited = 0;

  // table: [phases][taps] doubles (detect = 1), ignored with detect = 0
  LimiterRef(int channels, float ceiling, int lookahead, int hold, int detect, int phases, int taps, const double *table)
      : C(channels), c(ceiling), sh(limiter_shape(lookahead, hold, detect, phases, taps)) {
    h.resize((size_t)sh.phases * (size_t)sh.taps);
    for (size_t i = 0; i < h.size(); i++) h[i] = (float)table[i];
    xhist.assign((size_t)C * (size_t)sh.x_hist(), 0.0f);
    rhist.assign((size_t)sh.r_hist(), 1.0f);
  }

  // rows in[c * in_stride + i] -> out[c * out_stride + i], gain[i] (or nullptr)
  void process(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride, float *gain) {
    const int HX = sh.x_hist(), HR = sh.r_hist(), L = sh.L, M = sh.M;
    // the windows: history, then this call
    std::vector<float> x((size_t)C * ((size_t)HX + n)), r((size_t)HR + n);
    for (int ch = 0; ch < C; ch++) {
      float *w = x.data() + (size_t)ch * ((size_t)HX + n);
      std::memcpy(w, xhist.data() + (size_t)ch * (size_t)HX, sizeof(float) * (size_t)HX);
      if (n) std::memcpy(w + HX, in + (size_t)ch * in_stride, sizeof(float) * n);
    }
    std::memcpy(r.data(), rhist.data(), sizeof(float) * (size_t)HR);
    for (size_t i = 0; i < n; i++) {
      float e = 0.0f;
      for (int ch = 0; ch < C; ch++) {
        const float *at = x.data() + (size_t)ch * ((size_t)HX + n) + (size_t)HX + i;
        e = tp_absmax(e, at[-sh.D]);
        for (int p = 0; p < sh.phases; p++) {
          const float *hp = h.data() + (size_t)p * (size_t)sh.taps;
          const auto xk = [&](int k) { return at[-k]; };
          e = tp_absmax(e, sh.phases == 4 && sh.taps == 12 ? tp_dot_n<12>(hp, xk) : tp_dot(hp, sh.taps, xk));
        }
      }
      r[(size_t)HR + i] = lim_required_gain(c, e);
    }
    // m over [first output - L, end): m_at(j) is m of sample j - L of the call
    std::vector<float> m((size_t)L + n);
    for (size_t j = 0; j < (size_t)L + n; j++) {
      const float *at = r.data() + (size_t)(M - 1) + j;  // r of sample j - L
      float v = at[0];
      for (int i = 1; i < M; i++) v = fminf(v, at[-i]);
      m[j] = v;
    }
    for (size_t i = 0; i < n; i++) {
      const float *mt = m.data() + (size_t)L + i;
      float s[1];
      lim_sum(sh.K, s, [&](int, int k) { return mt[-k]; });
      const float g = lim_gain(s[0], sh.K, r[(size_t)HR + i - (size_t)L]);
      if (gain) gain[i] = g;
      min_gain = fminf(min_gain, g);
      limited += g < 1.0f ? 1u : 0u;
      for (int ch = 0; ch < C; ch++)
        out[(size_t)ch * out_stride + i] = x[(size_t)ch * ((size_t)HX + n) + (size_t)HX + i - (size_t)sh.latency()] * g;
    }
    for (int ch = 0; ch < C; ch++)
      std::memcpy(xhist.data() + (size_t)ch * (size_t)HX, x.data() + (size_t)ch * ((size_t)HX + n) + n, sizeof(float) * (size_t)HX);
    std::memcpy(rhist.data(), r.data() + n, sizeof(float) * (size_t)HR);
  }
};

}  // namespace earhip
