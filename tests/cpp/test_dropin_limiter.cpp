// Drop-in test of ear::hip::Limiter and ObjectsRenderer::attach_limiter, compiled against the C++14 mirror headers only
// (libear_amd/host/ear/...).  A limiter attached to a renderer must leave in its sink the operation of include/earhip.h
// (group N) — written out here from the header, in float64, step by step — over the float samples the renderer returned,
// under the bound of tests/limiter_model.py; a stand-alone limiter fed the same rows must give the sink's bits; no output
// sample passes the ceiling; a limiter of the wrong width and a call beyond the sink are refused.
// Needs a GPU (without one the constructors throw: no CPU fallback).
// Build (one line): g++ -std=c++14 -Wall -Wextra -Werror -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_limiter.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_limiter
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <ear/decorrelate.hpp>
#include <ear/dsp/objects_renderer.hpp>
#include <ear/hip_limiter.hpp>

#include "dropin_check.h"

using ear::dsp::ObjectsRenderer;
using ear::hip::Limiter;


static const size_t M = 13, N = 6, B = 512, T = 6, n = B * T;
static const int L = 48, H = 200, TAPS = 12, D = TAPS / 2, K = L + 1, MW = L + 2 + H;
static const double H0[12] = {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68};
static const double H1[12] = {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155};

static void set_curves(ObjectsRenderer &r) {
  for (size_t m = 0; m < M; m++) {
    std::vector<int64_t> t = {0, (int64_t)(700 + 37 * m), (int64_t)(2 * n)};
    std::vector<std::vector<float>> d, f;
    for (int k = 0; k < 3; k++) {
      std::vector<float> g(N), h(N);
      for (size_t c = 0; c < N; c++) g[c] = 0.25f * (float)((m + c + k) % 7), h[c] = 0.15f * (float)((m * 3 + c + 2 * k) % 5);
      d.push_back(g), f.push_back(h);
    }
    r.set_object_points(m, t, d, f);
  }
}

// The operation of the header in float64 over rows [N][len]; detect: true peak with annex 2's table.  Returns the worst
// |got - want| over the bound for the outputs and for the gain row; *peak = the largest |got|.
static void worst_errors(const std::vector<std::vector<float>> &rows, double c, bool detect, const float *sink, size_t sink_stride,
                         const std::vector<float> &gain, double *worst_out, double *worst_gain, double *peak) {
  const size_t len = rows[0].size();
  const int d = detect ? D : 0;
  auto x = [&](size_t ch, long i) { return i < 0 ? 0.0 : (double)rows[ch][(size_t)i]; };
  double h[4][12], A = 0, X = 0;
  for (int k = 0; k < 12; k++) h[0][k] = H0[k] / 8192, h[1][k] = H1[k] / 8192, h[2][k] = H1[11 - k] / 8192, h[3][k] = H0[11 - k] / 8192;
  for (int p = 0; p < 4; p++) {
    double a = 0;
    for (int k = 0; k < 12; k++) a += std::fabs(h[p][k]);
    A = std::fmax(A, a);
  }
  std::vector<double> r(len), m(len), g(len);
  for (size_t i = 0; i < len; i++) {
    double e = 0;
    for (size_t ch = 0; ch < N; ch++) {
      e = std::fmax(e, std::fabs(x(ch, (long)i - d)));
      X = std::fmax(X, std::fabs(x(ch, (long)i)));
      for (int p = 0; detect && p < 4; p++) {
        double y = 0;
        for (int k = 0; k < 12; k++) y += h[p][k] * x(ch, (long)i - k);
        e = std::fmax(e, std::fabs(y));
      }
    }
    r[i] = e > 0 ? std::fmin(1.0, c / e) : 1.0;
  }
  auto at = [](const std::vector<double> &v, long i) { return i < 0 ? 1.0 : v[(size_t)i]; };
  for (size_t i = 0; i < len; i++) {
    double v = 1.0;
    for (int k = 0; k < MW; k++) v = std::fmin(v, at(r, (long)i - k));
    m[i] = v;
  }
  const double unit = ((detect ? (TAPS + 1) * A * X / c : 0.0) + K + 4) * std::ldexp(1.0, -24);
  *worst_out = *worst_gain = *peak = 0;
  for (size_t i = 0; i < len; i++) {
    double s = 0;
    for (int k = 0; k < K; k++) s += at(m, (long)i - k);
    g[i] = std::fmin(s / K, at(r, (long)i - L));
    *worst_gain = std::fmax(*worst_gain, std::fabs((double)gain[i] - g[i]) / unit);
    for (size_t ch = 0; ch < N; ch++) {
      const double xd = x(ch, (long)i - d - L), got = (double)sink[ch * sink_stride + i];
      *peak = std::fmax(*peak, std::fabs(got));
      if (xd == 0) {
        CHECK(got == 0);
      } else {
        *worst_out = std::fmax(*worst_out, std::fabs(got - xd * g[i]) / (std::fabs(xd) * unit));
      }
    }
  }
}

int main() {
  const std::vector<std::string> names = {"M+030", "M-030", "M+000", "LFE1", "M+110", "M-110"};
  ObjectsRenderer r(M, N, B, ear::designDecorrelators(names), 255, T);
  set_curves(r);
  ear::hip::Context &ctx = ear::hip::default_context();

  std::mt19937 rng(11);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  const float c = 0.5f;
  Limiter lim(N, c, L, H, n), alone(N, c, L, H, n), sample(N, c, L, H, 2 * n, 48000, Limiter::Detect::SamplePeak);
  CHECK(lim.latency() == (size_t)(D + L) && sample.latency() == (size_t)L && lim.num_channels() == N);
  CHECK(lim.stats().min_gain == 1.0f && lim.stats().limited_samples == 0);

  // two calls of process() from host pointers with the limiter attached; the sink in device-reachable host memory
  const size_t cap = 2 * n, stride = cap + 8;
  float *sink = ctx.alloc_host(N * stride);
  for (size_t i = 0; i < N * stride; i++) sink[i] = 9.0f;
  std::vector<std::vector<float>> in(M, std::vector<float>(2 * n)), out(N, std::vector<float>(2 * n));
  for (auto &row : in)
    for (auto &v : row) v = 0.5f * u(rng);
  std::vector<std::vector<float>> lone(N, std::vector<float>(2 * n));
  std::vector<float> gain(2 * n);
  r.attach_limiter(lim, sink, stride, cap);
  CHECK(r.limiter_position() == 0);
  for (size_t call = 0; call < 2; call++) {
    std::vector<const float *> ip;
    std::vector<float *> op, lp;
    for (auto &row : in) ip.push_back(row.data() + call * n);
    for (auto &row : out) op.push_back(row.data() + call * n);
    for (auto &row : lone) lp.push_back(row.data() + call * n);
    r.process(T, ip.data(), op.data());
    std::vector<const float *> rp(op.begin(), op.end());
    alone.process(n, rp.data(), lp.data(), gain.data() + call * n);
  }
  ctx.synchronize();
  CHECK(r.limiter_position() == cap);
  for (size_t k = 0; k < N; k++) {
    CHECK(std::memcmp(sink + k * stride, lone[k].data(), cap * sizeof(float)) == 0);
    for (size_t i = cap; i < stride; i++) CHECK(sink[k * stride + i] == 9.0f);
  }
  double wo, wg, peak;
  worst_errors(out, c, true, sink, stride, gain, &wo, &wg, &peak);
  std::printf("attached through process(), true peak: worst error %.3f of the bound (out), %.3f (gain); max |out| / c = %.9f\n", wo, wg,
              peak / c);
  CHECK(wo <= 1.0 && wg <= 1.0);
  CHECK(peak <= (double)c * (1.0 + std::ldexp(1.0, -22)));
  const Limiter::Stats st = lim.stats(), sa = alone.stats();
  CHECK(st.limited_samples > 1000 && st.limited_samples == sa.limited_samples && st.min_gain == sa.min_gain);
  CHECK(st.min_gain == *std::min_element(gain.begin(), gain.end()));
  CHECK(st.limited_samples == (uint64_t)std::count_if(gain.begin(), gain.end(), [](float g) { return g < 1.0f; }));

  // the sample-peak detector, stand-alone, the float** overload, one call over both halves
  {
    std::vector<float *> ip, op;
    std::vector<std::vector<float>> lim_rows(N, std::vector<float>(2 * n));
    for (auto &row : out) ip.push_back(row.data());
    for (auto &row : lim_rows) op.push_back(row.data());
    sample.process(2 * n, ip.data(), op.data(), gain.data());
    std::vector<float> flat(N * 2 * n);
    for (size_t k = 0; k < N; k++) std::memcpy(flat.data() + k * 2 * n, lim_rows[k].data(), 2 * n * sizeof(float));
    worst_errors(out, c, false, flat.data(), 2 * n, gain, &wo, &wg, &peak);
    std::printf("stand-alone, sample peak: worst error %.3f of the bound (out), %.3f (gain); max |out| / c = %.9f\n", wo, wg, peak / c);
    CHECK(wo <= 1.0 && wg <= 1.0);
    CHECK(peak <= (double)c * (1.0 + std::ldexp(1.0, -22)));
  }

  // the sink is full: the next call is refused before anything is rendered
  bool threw = false;
  try {
    std::vector<const float *> ip;
    std::vector<float *> op;
    for (auto &row : in) ip.push_back(row.data());
    for (auto &row : out) op.push_back(row.data());
    r.process(T, ip.data(), op.data());
  } catch (const ear::invalid_argument &) {
    threw = true;
  }
  CHECK(threw && r.limiter_position() == cap);

  // attaching again rewinds; reset() of the renderer leaves the limiter alone; the PCM-out form feeds it too
  r.attach_limiter(lim, sink, stride, cap);
  CHECK(r.limiter_position() == 0);
  r.reset(0);
  CHECK(lim.stats().limited_samples == st.limited_samples);
  lim.reset();
  CHECK(lim.stats().limited_samples == 0 && lim.stats().min_gain == 1.0f);
  std::vector<int16_t> frames(n * M), pcm(n * N);
  for (auto &v : frames) v = (int16_t)(rng() & 0xFFFF);
  r.process_frames(T, frames.data(), (int)M, 0, pcm.data());
  CHECK(r.limiter_position() == n);
  r.detach_limiter();
  r.process_frames(T, frames.data(), (int)M, 0, pcm.data());
  CHECK(r.limiter_position() == 0);  // detached

  // a limiter of the wrong width is refused, and so is a configuration outside the header's limits
  Limiter wide(N + 1, c, L, H, n);
  CHECK_THROWS_AS(r.attach_limiter(wide, sink, stride, cap), ear::invalid_argument);
  for (int which = 0; which < 4; which++) {
    threw = false;
    try {
      if (which == 0) Limiter bad(N, 0.0f, L, H, n);
      if (which == 1) Limiter bad(N, c, 7, H, n);
      if (which == 2) Limiter bad(N, c, L, 8193, n);
      if (which == 3) Limiter bad(N, c, L, H, n, 96000);  // annex 2's table at another rate
    } catch (const ear::invalid_argument &) {
      threw = true;
    }
    CHECK(threw);
  }
  Limiter own(2, c, 8, 0, 64, 96000, 2, 3, std::vector<double>{0.1, 0.8, 0.1, 0.3, 0.6, 0.1});
  CHECK(own.latency() == 8 + 1);

  return summary();
}
