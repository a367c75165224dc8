// Drop-in test of ear::hip::LoudnessMeter and ObjectsRenderer::attach_loudness, compiled against the C++14 mirror headers only
// (libear_amd/host/ear/...).  A meter attached to a renderer must hold the step energies of the K-weighting cascade of
// include/earhip.h (group L) — written out here from the header, in float64, sample by sample — over the float samples the
// renderer returned, through process() and through the PCM-out process_frames; the free functions must agree with the meter's
// result(); a stand-alone meter fed the same rows must give the attached one's bits.
// Needs a GPU (without one the constructors throw: no CPU fallback).
// Build (one line): g++ -std=c++14 -Wall -Wextra -Werror -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_loudness.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_loudness
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <ear/decorrelate.hpp>
#include <ear/dsp/objects_renderer.hpp>
#include <ear/hip_loudness.hpp>

#include "dropin_check.h"

using ear::dsp::ObjectsRenderer;
using ear::hip::LoudnessMeter;


static const size_t M = 13, N = 6, B = 512, T = 60, n = B * T, STEP = 4800;

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

// the cascade of the header, in the direct form it is written in there
static std::vector<double> model_steps(const std::vector<std::vector<float>> &rows) {
  static const double c[2][5] = {{1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585},
                                 {1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621}};
  const size_t steps = rows[0].size() / STEP;
  std::vector<double> z(steps * rows.size());
  for (size_t ch = 0; ch < rows.size(); ch++) {
    double x1[2] = {0, 0}, x2[2] = {0, 0}, y1[2] = {0, 0}, y2[2] = {0, 0}, acc = 0;
    for (size_t i = 0; i < steps * STEP; i++) {
      double v = (double)rows[ch][i];
      for (int s = 0; s < 2; s++) {
        const double y = c[s][0] * v + c[s][1] * x1[s] + c[s][2] * x2[s] - c[s][3] * y1[s] - c[s][4] * y2[s];
        x2[s] = x1[s], x1[s] = v, y2[s] = y1[s], y1[s] = y;
        v = y;
      }
      acc += v * v;
      if ((i + 1) % STEP == 0) z[(i / STEP) * rows.size() + ch] = acc / (double)STEP, acc = 0;
    }
  }
  return z;
}

static bool within_bound(const std::vector<double> &got, const std::vector<double> &want, size_t channels, double *worst) {
  if (got.size() != want.size()) return false;
  bool ok = true;
  *worst = 0;
  for (size_t ch = 0; ch < channels; ch++) {
    double zc = 0;
    for (size_t i = ch; i < want.size(); i += channels) zc = std::fmax(zc, want[i]);
    for (size_t i = ch; i < want.size(); i += channels) {
      const double err = std::fabs(got[i] - want[i]);
      if (!(err <= 1e-9 * want[i] + 1e-18 * zc)) ok = false;
      if (want[i] > 0) *worst = std::fmax(*worst, err / want[i]);
    }
  }
  return ok;
}

int main() {
  const std::vector<std::string> names = {"M+030", "M-030", "M+000", "LFE1", "M+110", "M-110"};
  ObjectsRenderer r(M, N, B, ear::designDecorrelators(names), 255, T);
  set_curves(r);
  LoudnessMeter meter(N), alone(N);
  CHECK(meter.num_channels() == N && meter.num_steps() == 0);

  const std::vector<double> w = ear::hip::loudness_layout_weights("0+5+0");
  CHECK((w == std::vector<double>{1.0, 1.0, 1.0, 0.0, 1.41, 1.41}));
  CHECK_THROWS_AS(ear::hip::loudness_layout_weights("no such layout"), ear::unknown_layout);

  // two calls of process() from host pointers with the meter attached
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> u(-0.5f, 0.5f);
  std::vector<std::vector<float>> in(M, std::vector<float>(2 * n)), out(N, std::vector<float>(2 * n));
  for (auto &row : in)
    for (auto &v : row) v = u(rng);
  r.attach_loudness(meter);
  for (size_t call = 0; call < 2; call++) {
    std::vector<const float *> ip;
    std::vector<float *> op;
    for (auto &row : in) ip.push_back(row.data() + call * n);
    for (auto &row : out) op.push_back(row.data() + call * n);
    r.process(T, ip.data(), op.data());
    std::vector<const float *> rp(op.begin(), op.end());
    alone.process(rp.data(), n);
  }
  CHECK(meter.num_steps() == 2 * n / STEP);
  const std::vector<double> got = meter.steps(), want = model_steps(out);
  double worst = 0;
  CHECK(within_bound(got, want, N, &worst));
  std::printf("attached through process(): %zu steps, worst relative difference %.3e\n", meter.num_steps(), worst);
  const std::vector<double> same = alone.steps();
  CHECK(same.size() == got.size() && std::memcmp(same.data(), got.data(), got.size() * sizeof(double)) == 0);

  const ear::hip::Loudness a = meter.result(w), b = ear::hip::loudness_gate(got, w);
  CHECK(a.integrated == b.integrated && a.max_momentary == b.max_momentary && a.max_short_term == b.max_short_term);
  CHECK(std::isfinite(a.integrated) && std::isfinite(a.max_momentary) && std::isinf(a.max_short_term));
  std::printf("integrated %.4f LKFS, maximum momentary %.4f LKFS\n", a.integrated, a.max_momentary);

  // reset() of the renderer leaves the meter alone; the PCM-out form is metered on its float samples (those of process_frames)
  r.reset(0);
  CHECK(meter.num_steps() == 2 * n / STEP);
  meter.reset();
  CHECK(meter.num_steps() == 0);
  std::vector<int16_t> frames(n * M), pcm(n * N);
  for (auto &v : frames) v = (int16_t)(rng() & 0xFFFF);
  r.process_frames(T, frames.data(), (int)M, 0, pcm.data());
  CHECK(meter.num_steps() == n / STEP);
  r.detach_loudness();
  r.reset(0);
  std::vector<std::vector<float>> fl(N, std::vector<float>(n));
  std::vector<float *> fp;
  for (auto &row : fl) fp.push_back(row.data());
  r.process_frames(T, frames.data(), (int)M, 0, fp.data());
  CHECK(meter.num_steps() == n / STEP);  // detached: no more steps
  CHECK(within_bound(meter.steps(), model_steps(fl), N, &worst));
  std::printf("attached through the PCM-out process_frames: %zu steps, worst relative difference %.3e\n", meter.num_steps(), worst);

  // a meter of the wrong width is refused
  LoudnessMeter wrong(N + 1, 48000, 8);
  CHECK_THROWS_AS(r.attach_loudness(wrong), ear::invalid_argument);

  return summary();
}
