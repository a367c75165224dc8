// Drop-in test of true peak and loudness range through ear::hip::LoudnessMeter, compiled against the C++14 mirror headers only
// (libear_amd/host/ear/...).  A meter made with TruePeak::bs1770() and attached to a renderer must hold the peaks of the
// interpolator of include/earhip.h (group L) — written out here from the header, in float64, sample by sample — over the float
// samples the renderer returned, within the header's bound; its sample peaks must be the samples' own; range() must agree with the
// free function and with Tech 3342 written out here; a stand-alone meter fed the same rows must give the attached one's bits; a
// meter made without true peak must refuse the peak queries.
// Needs a GPU (without one the constructors throw: no CPU fallback).
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
#include <ear/hip_loudness.hpp>

#include "dropin_check.h"

using ear::dsp::ObjectsRenderer;
using ear::hip::LoudnessMeter;
using ear::hip::TruePeak;


static const size_t M = 13, N = 6, B = 512, T = 300, n = B * T, STEP = 4800, CALLS = 4;

static void set_curves(ObjectsRenderer &r) {
  for (size_t m = 0; m < M; m++) {
    std::vector<int64_t> t = {0, (int64_t)(700 + 37 * m), (int64_t)(CALLS * n)};
    std::vector<std::vector<float>> d, f;
    for (int k = 0; k < 3; k++) {
      std::vector<float> g(N), h(N);
      for (size_t c = 0; c < N; c++) g[c] = 0.25f * (float)((m + c + k) % 7), h[c] = 0.15f * (float)((m * 3 + c + 2 * k) % 5);
      d.push_back(g), f.push_back(h);
    }
    r.set_object_points(m, t, d, f);
  }
}

// the table of the header
static void table(double h[4][12]) {
  static const int h0[12] = {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68};
  static const int h1[12] = {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155};
  for (int k = 0; k < 12; k++)
    h[0][k] = h0[k] / 8192.0, h[1][k] = h1[k] / 8192.0, h[2][k] = h1[11 - k] / 8192.0, h[3][k] = h0[11 - k] / 8192.0;
}

struct ModelPeaks {
  std::vector<double> tp, sp;      // [channels] over everything
  std::vector<double> step_tp;     // [steps][channels]
};

static ModelPeaks model_peaks(const std::vector<std::vector<float>> &rows) {
  double h[4][12];
  table(h);
  const size_t C = rows.size(), steps = rows[0].size() / STEP;
  ModelPeaks p;
  p.tp.assign(C, 0.0), p.sp.assign(C, 0.0), p.step_tp.assign(steps * C, 0.0);
  for (size_t ch = 0; ch < C; ch++)
    for (size_t i = 0; i < rows[ch].size(); i++) {
      double m = 0;
      for (int q = 0; q < 4; q++) {
        double y = 0;
        for (size_t k = 0; k < 12 && k <= i; k++) y += h[q][k] * (double)rows[ch][i - k];
        m = std::fmax(m, std::fabs(y));
      }
      p.tp[ch] = std::fmax(p.tp[ch], m);
      p.sp[ch] = std::fmax(p.sp[ch], std::fabs((double)rows[ch][i]));
      if (i / STEP < steps) p.step_tp[(i / STEP) * C + ch] = std::fmax(p.step_tp[(i / STEP) * C + ch], m);
    }
  return p;
}

// the worst |got - want| over the bound (taps + 1) 2^-24 A X_c, A = 2.023
static double worst_ratio(const std::vector<float> &got, const std::vector<double> &want, const std::vector<double> &sp) {
  double worst = got.size() == want.size() ? 0.0 : 1e30;
  for (size_t i = 0; i < got.size() && i < want.size(); i++) {
    const double bound = 13.0 * std::ldexp(1.0, -24) * 2.023 * sp[i % sp.size()];
    const double err = std::fabs((double)got[i] - want[i]);
    worst = std::fmax(worst, bound > 0 ? err / bound : (err > 0 ? 1e30 : 0.0));
  }
  return worst;
}

// EBU Tech 3342 from the header's text
static ear::hip::LoudnessRange model_range(const std::vector<double> &z, const std::vector<double> &w) {
  const size_t C = w.size(), steps = z.size() / C;
  ear::hip::LoudnessRange r = {0.0, -INFINITY, -INFINITY};
  if (steps < 30) return r;
  std::vector<double> P, l;
  for (size_t j = 0; j + 30 <= steps; j++) {
    double p = 0;
    for (size_t c = 0; c < C; c++) {
      double s = 0;
      for (size_t i = 0; i < 30; i++) s += z[(j + i) * C + c];
      p += w[c] * (s / 30.0);
    }
    P.push_back(p), l.push_back(-0.691 + 10.0 * std::log10(p));
  }
  double sum = 0;
  size_t cnt = 0;
  for (size_t j = 0; j < P.size(); j++)
    if (l[j] > -70.0) sum += P[j], cnt++;
  if (!cnt) return r;
  const double gamma = -0.691 + 10.0 * std::log10(sum / (double)cnt) - 20.0;
  std::vector<double> s;
  for (size_t j = 0; j < P.size(); j++)
    if (l[j] > -70.0 && l[j] > gamma) s.push_back(l[j]);
  if (s.empty()) return r;
  std::sort(s.begin(), s.end());
  r.low = s[(size_t)std::floor((double)(s.size() - 1) * 0.10 + 0.5)];
  r.high = s[(size_t)std::floor((double)(s.size() - 1) * 0.95 + 0.5)];
  r.lra = r.high - r.low;
  return r;
}

int main() {
  const std::vector<std::string> names = {"M+030", "M-030", "M+000", "LFE1", "M+110", "M-110"};
  ObjectsRenderer r(M, N, B, ear::designDecorrelators(names), 255, T);
  set_curves(r);
  LoudnessMeter meter(N, 48000, 400, std::vector<double>(), ear::hip::default_context(), TruePeak::bs1770());
  LoudnessMeter alone(N, 48000, 400, std::vector<double>(), ear::hip::default_context(), TruePeak::bs1770());
  LoudnessMeter plain(N, 48000, 400);
  const std::vector<double> w = ear::hip::loudness_layout_weights("0+5+0");

  // four calls of process() from host pointers with the meter attached: 12.8 s of noise whose level drops by 12 dB half way
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> u(-0.5f, 0.5f);
  const size_t total = CALLS * n;
  std::vector<std::vector<float>> in(M, std::vector<float>(total)), out(N, std::vector<float>(total));
  for (auto &row : in)
    for (size_t i = 0; i < total; i++) row[i] = u(rng) * (i < total / 2 ? 0.2f : 0.05f);
  r.attach_loudness(meter);
  for (size_t call = 0; call < CALLS; call++) {
    std::vector<const float *> ip;
    std::vector<float *> op;
    for (auto &row : in) ip.push_back(row.data() + call * n);
    for (auto &row : out) op.push_back(row.data() + call * n);
    r.process(T, ip.data(), op.data());
    std::vector<const float *> rp(op.begin(), op.end());
    alone.process(rp.data(), n);
    plain.process(rp.data(), n);
  }
  CHECK(meter.num_steps() == total / STEP);
  const ModelPeaks want = model_peaks(out);
  const ear::hip::Peaks got = meter.peaks(), steps = meter.step_peaks();
  CHECK(got.true_peak.size() == N && steps.true_peak.size() == (total / STEP) * N);
  for (size_t c = 0; c < N; c++) CHECK((double)got.sample_peak[c] == want.sp[c] && want.sp[c] > 0);
  double worst = worst_ratio(got.true_peak, want.tp, want.sp);
  CHECK(worst <= 1.0);
  std::printf("attached through process(): true peaks so far, worst error %.3f of the bound\n", worst);
  worst = worst_ratio(steps.true_peak, want.step_tp, want.sp);
  CHECK(worst <= 1.0);
  std::printf("attached through process(): %zu steps, worst error %.3f of the bound\n", meter.num_steps(), worst);
  const ear::hip::Peaks same = alone.peaks(), same_steps = alone.step_peaks();
  CHECK(std::memcmp(same.true_peak.data(), got.true_peak.data(), N * sizeof(float)) == 0);
  CHECK(std::memcmp(same_steps.true_peak.data(), steps.true_peak.data(), steps.true_peak.size() * sizeof(float)) == 0);
  CHECK(std::memcmp(same_steps.sample_peak.data(), steps.sample_peak.data(), steps.sample_peak.size() * sizeof(float)) == 0);

  // loudness range: the meter's, the free function's and the header's definition
  const std::vector<double> z = meter.steps();
  const ear::hip::LoudnessRange a = meter.range(w), b = ear::hip::loudness_range(z, w), c = model_range(z, w);
  CHECK(a.lra == b.lra && a.low == b.low && a.high == b.high);
  CHECK(std::fabs(a.lra - c.lra) <= 1e-9 && std::fabs(a.low - c.low) <= 1e-9 && std::fabs(a.high - c.high) <= 1e-9);
  CHECK(std::isfinite(a.low) && a.lra > 1.0);  // (the input's two levels lie 12 dB apart; the objects' gains move too)
  std::printf("loudness range %.4f LU (%.4f .. %.4f LKFS)\n", a.lra, a.low, a.high);
  // the energies do not know of the peaks: two meters over the same calls, one with true peak and one without, hold the same bits
  const std::vector<double> ps = plain.steps(), as = alone.steps();
  CHECK(ps.size() == as.size() && std::memcmp(ps.data(), as.data(), as.size() * sizeof(double)) == 0);
  const ear::hip::LoudnessRange d = plain.range(w), e = alone.range(w);
  CHECK(e.lra == d.lra && e.low == d.low && e.high == d.high);

  // a meter made without true peak has no peaks to give; a table of the wrong shape is refused
  CHECK_THROWS_AS(plain.peaks(), ear::invalid_argument);
  CHECK_THROWS_AS(LoudnessMeter bad(N, 48000, 8, std::vector<double>(), ear::hip::default_context(),
                                    TruePeak::table(9, 2, std::vector<double>(18, 0.5))),
                  ear::invalid_argument);
  // reset() of the renderer leaves the peaks alone, reset() of the meter clears them
  r.reset(0);
  CHECK(meter.peaks().true_peak == got.true_peak);
  meter.reset();
  CHECK(meter.num_steps() == 0 && meter.peaks().true_peak == std::vector<float>(N, 0.0f));
  r.detach_loudness();

  return summary();
}
