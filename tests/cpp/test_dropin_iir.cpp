// Drop-in test of ear::hip::IirBank, compiled against the C++14 mirror headers only (libear_amd/host/ear/...).  A bank (the
// bass management of a 0+5+0 bus) fed the float rows an ObjectsRenderer returned must give the operation of include/earhip.h
// (group O) — written out here from the header, in float64, sample by sample — under the header's bound; the device form fed the
// same rows in the same calls must give the host form's bits; reset() starts over; configurations outside the header's limits
// are refused.
// Needs a GPU (without one the constructors throw: no CPU fallback).
// Build (one line): g++ -std=c++14 -Wall -Wextra -Werror -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_iir.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_iir
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
#include <ear/hip_iir.hpp>

#include "dropin_check.h"

using ear::dsp::ObjectsRenderer;
using ear::hip::IirBank;


static const size_t M = 13, N = 6, B = 512, T = 6, n = B * T, LFE = 3;

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

// the header's operation in float64 over rows [n_in][len]: the worst |got - want| over 2^-24 |want| + 1e-9 peak(row)
static double worst_error(const std::vector<std::vector<float>> &rows, const std::vector<IirBank::Route> &routes, size_t n_out,
                          const float *sink, size_t sink_stride) {
  const size_t len = rows[0].size();
  double worst = 0;
  for (size_t k = 0; k < n_out; k++) {
    std::vector<double> want(len, 0.0);
    for (const auto &rt : routes) {
      if (rt.out != k) continue;
      std::vector<double> s(2 * rt.sections.size(), 0.0);
      for (size_t i = 0; i < len; i++) {
        double v = (double)rows[rt.in][i];
        for (size_t q = 0; q < rt.sections.size(); q++) {
          const IirBank::Section &c = rt.sections[q];
          const double y = c[0] * v + s[2 * q];
          s[2 * q] = c[1] * v - c[3] * y + s[2 * q + 1];
          s[2 * q + 1] = c[2] * v - c[4] * y;
          v = y;
        }
        want[i] += rt.gain * v;
      }
    }
    double peak = 0;
    for (double v : want) peak = std::fmax(peak, std::fabs(v));
    for (size_t i = 0; i < len; i++) {
      const double err = std::fabs((double)sink[k * sink_stride + i] - want[i]), b = std::ldexp(std::fabs(want[i]), -24) + 1e-9 * peak;
      if (b == 0) {
        CHECK(err == 0);
      } else {
        worst = std::fmax(worst, err / b);
      }
    }
  }
  return worst;
}

int main() {
  const std::vector<std::string> names = {"M+030", "M-030", "M+000", "LFE1", "M+110", "M-110"};
  ObjectsRenderer r(M, N, B, ear::designDecorrelators(names), 255, T);
  set_curves(r);
  ear::hip::Context &ctx = ear::hip::default_context();

  // bass management: mains through a high-pass LR4, their low-pass LR4 summed into the LFE, the LFE passed through
  const auto hp = IirBank::linkwitz_riley4(IirBank::Kind::Highpass, 48000.0, 80.0);
  const auto lp = IirBank::linkwitz_riley4(IirBank::Kind::Lowpass, 48000.0, 80.0);
  CHECK(std::fabs(lp[0][0] + lp[0][1] + lp[0][2] - (1.0 + lp[0][3] + lp[0][4])) < 1e-12);  // unity at DC
  std::vector<IirBank::Route> routes;
  for (size_t c = 0; c < N; c++)
    if (c != LFE) routes.push_back({c, c, 1.0, hp});
  routes.push_back({LFE, LFE, 1.0, {}});
  for (size_t c = 0; c < N; c++)
    if (c != LFE) routes.push_back({c, LFE, 1.0, lp});
  IirBank bank(N, N, routes, n), alone(N, N, routes, n);
  CHECK(bank.num_inputs() == N && bank.num_outputs() == N && bank.chunk_length() >= 1);

  std::mt19937 rng(11);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  const size_t cap = 2 * n, stride = cap + 8;
  float *bus = ctx.alloc_host(N * stride), *sink = ctx.alloc_host(N * stride);
  for (size_t i = 0; i < N * stride; i++) sink[i] = 9.0f;
  std::vector<std::vector<float>> in(M, std::vector<float>(2 * n)), out(N, std::vector<float>(2 * n));
  for (auto &row : in)
    for (auto &v : row) v = 0.5f * u(rng);
  std::vector<std::vector<float>> managed(N, std::vector<float>(2 * n));
  for (size_t call = 0; call < 2; call++) {
    std::vector<const float *> ip;
    std::vector<float *> op, mp;
    for (auto &row : in) ip.push_back(row.data() + call * n);
    for (auto &row : out) op.push_back(row.data() + call * n);
    for (auto &row : managed) mp.push_back(row.data() + call * n);
    r.process(T, ip.data(), op.data());
    // the host form, and the device form on rows in device-reachable memory
    std::vector<const float *> rp(op.begin(), op.end());
    bank.process(n, rp.data(), mp.data());
    for (size_t k = 0; k < N; k++) std::memcpy(bus + k * stride + call * n, out[k].data() + call * n, n * sizeof(float));
    alone.process_device(n, bus + call * n, stride, sink + call * n, stride);
  }
  ctx.synchronize();
  std::vector<float> flat(N * cap);
  for (size_t k = 0; k < N; k++) {
    CHECK(std::memcmp(sink + k * stride, managed[k].data(), cap * sizeof(float)) == 0);
    for (size_t i = cap; i < stride; i++) CHECK(sink[k * stride + i] == 9.0f);
    std::memcpy(flat.data() + k * cap, managed[k].data(), cap * sizeof(float));
  }
  const double w = worst_error(out, routes, N, flat.data(), cap);
  std::printf("bass management of 0+5+0 over a renderer's rows: worst error %.3f of the bound\n", w);
  CHECK(w <= 1.0);

  // a call longer than max_samples is refused and consumes nothing; reset() starts over
  CHECK_THROWS_AS(alone.process_device(n + 1, bus, stride, sink, stride), ear::invalid_argument);
  bank.reset();
  {
    std::vector<float *> ip, mp;
    std::vector<std::vector<float>> again(N, std::vector<float>(n));
    for (auto &row : out) ip.push_back(row.data());
    for (auto &row : again) mp.push_back(row.data());
    bank.process(n, ip.data(), mp.data());  // (the float** overload)
    for (size_t k = 0; k < N; k++) CHECK(std::memcmp(again[k].data(), managed[k].data(), n * sizeof(float)) == 0);
  }

  // configurations outside the header's limits
  for (int which = 0; which < 4; which++) {
    bool threw = false;
    try {
      if (which == 0) IirBank bad(N, N, {}, n);
      if (which == 1) IirBank bad(N, N, {{0, 0, 1.0, {IirBank::Section{{1.0, 0.0, 0.0, 0.0, 1.0}}}}}, n);
      if (which == 2) IirBank bad(N, N, {{0, N, 1.0, {}}}, n);
      if (which == 3) (void)IirBank::design(IirBank::Kind::Peaking, 48000.0, 24000.0, 1.0, 3.0);
    } catch (const ear::invalid_argument &) {
      threw = true;
    }
    CHECK(threw);
  }

  return summary();
}
