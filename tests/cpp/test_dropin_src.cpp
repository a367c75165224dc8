// Drop-in test of ear::hip::SampleRateConverter, compiled against the C++14 mirror headers only (libear_amd/host/ear/...).  A
// converter from 48 kHz to 44.1 kHz (147 / 160, 48 taps per phase, the designer's prototype) fed the float rows an
// ObjectsRenderer returned must give the BITS of the operation of include/earhip.h (group P) — written out here from the header,
// with std::fmaf, sample by sample — and ceil(N L / M) outputs after N inputs; the device form fed the same rows in the same calls
// must give the same bits; reset() starts over; configurations outside the header's limits are refused.
// Needs a GPU (without one the constructors throw: no CPU fallback).
// Build (one line): g++ -std=c++14 -Wall -Wextra -Werror -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_src.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_src
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include <ear/decorrelate.hpp>
#include <ear/dsp/objects_renderer.hpp>
#include <ear/hip_src.hpp>

#include "dropin_check.h"

using ear::dsp::ObjectsRenderer;
using ear::hip::SampleRateConverter;


static const size_t M = 13, N = 6, B = 512, T = 6, n = B * T;
static const size_t UP = 147, DOWN = 160, TAPS = 48;

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

// the header's operation over one whole row: output j = the chain over c[p_j][k] x[i_j - k], x = +0.0f in front of the stream
static std::vector<float> convert(const std::vector<float> &x, const std::vector<double> &h) {
  const size_t total = (x.size() * UP + DOWN - 1) / DOWN;
  std::vector<float> y(total);
  for (size_t j = 0; j < total; j++) {
    const size_t i = j * DOWN / UP, p = j * DOWN % UP;
    float acc = 0.0f;
    for (size_t k = 0; k < TAPS; k++) acc = std::fmaf((float)h[p + k * UP], k <= i ? x[i - k] : 0.0f, acc);
    y[j] = acc;
  }
  return y;
}

int main() {
  const std::vector<std::string> names = {"M+030", "M-030", "M+000", "LFE1", "M+110", "M-110"};
  ObjectsRenderer r(M, N, B, ear::designDecorrelators(names), 255, T);
  set_curves(r);
  ear::hip::Context &ctx = ear::hip::default_context();

  const std::vector<double> h = SampleRateConverter::design(UP, DOWN, TAPS);
  CHECK(h.size() == UP * TAPS);
  double dc = 0;
  for (double v : h) dc += v;
  CHECK(std::fabs(dc - (double)UP) < 1e-9);  // unit DC gain, times L
  SampleRateConverter host(N, UP, DOWN, TAPS, h, n), device(N, UP, DOWN, TAPS, h, n);
  CHECK(host.num_channels() == N && host.max_out() == (n * UP + DOWN - 1) / DOWN);
  CHECK(host.info().latency_in == (double)(UP * TAPS - 1) / (2.0 * UP));

  std::mt19937 rng(11);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  const size_t total = (2 * n * UP + DOWN - 1) / DOWN, stride_in = 2 * n + 8, stride_out = total + 8;
  float *bus = ctx.alloc_host(N * stride_in), *sink = ctx.alloc_host(N * stride_out);
  for (size_t i = 0; i < N * stride_out; i++) sink[i] = 9.0f;
  std::vector<std::vector<float>> in(M, std::vector<float>(2 * n)), out(N, std::vector<float>(2 * n));
  for (auto &row : in)
    for (auto &v : row) v = 0.5f * u(rng);
  std::vector<std::vector<float>> resampled(N, std::vector<float>(total));
  size_t made = 0;
  for (size_t call = 0; call < 2; call++) {
    std::vector<const float *> ip;
    std::vector<float *> op, mp;
    for (auto &row : in) ip.push_back(row.data() + call * n);
    for (auto &row : out) op.push_back(row.data() + call * n);
    for (auto &row : resampled) mp.push_back(row.data() + made);
    r.process(T, ip.data(), op.data());
    // the host form, and the device form on rows in device-reachable memory
    std::vector<const float *> rp(op.begin(), op.end());
    const size_t want = host.next_out(n);
    CHECK(made + want == ((call + 1) * n * UP + DOWN - 1) / DOWN);
    CHECK(host.process(n, rp.data(), mp.data(), total - made) == want);
    for (size_t k = 0; k < N; k++) std::memcpy(bus + k * stride_in + call * n, out[k].data() + call * n, n * sizeof(float));
    CHECK(device.process_device(n, bus + call * n, stride_in, sink + made, stride_out, want) == want);
    made += want;
  }
  ctx.synchronize();
  CHECK(made == total);
  for (size_t k = 0; k < N; k++) {
    const std::vector<float> want = convert(out[k], h);
    CHECK(want.size() == total);
    CHECK(std::memcmp(resampled[k].data(), want.data(), total * sizeof(float)) == 0);
    CHECK(std::memcmp(sink + k * stride_out, want.data(), total * sizeof(float)) == 0);
    for (size_t i = total; i < stride_out; i++) CHECK(sink[k * stride_out + i] == 9.0f);
  }
  std::printf("48 kHz to 44.1 kHz over a renderer's rows: %zu outputs of %zu inputs, the header's bits\n", total, 2 * n);

  // a call longer than max_samples, or with too little room, is refused and consumes nothing; reset() starts over
  for (int which = 0; which < 2; which++) {
    bool threw = false;
    try {
      if (which == 0) device.process_device(n + 1, bus, stride_in, sink, stride_out, stride_out);
      if (which == 1) device.process_device(n, bus, stride_in, sink, stride_out, device.next_out(n) - 1);
    } catch (const ear::invalid_argument &) {
      threw = true;
    }
    CHECK(threw);
  }
  host.reset();
  {
    std::vector<float *> ip, mp;
    std::vector<std::vector<float>> again(N, std::vector<float>(total));
    for (auto &row : out) ip.push_back(row.data());
    for (auto &row : again) mp.push_back(row.data());
    const size_t got = host.process(n, ip.data(), mp.data(), total);  // (the float** overload)
    CHECK(got == (n * UP + DOWN - 1) / DOWN);
    for (size_t k = 0; k < N; k++) CHECK(std::memcmp(again[k].data(), resampled[k].data(), got * sizeof(float)) == 0);
  }

  // configurations outside the header's limits
  for (int which = 0; which < 6; which++) {
    bool threw = false;
    try {
      if (which == 0) SampleRateConverter bad(N, 4, 2, 8, std::vector<double>(32, 0.0), n);  // a common factor
      if (which == 1) SampleRateConverter bad(N, 3, 2, 8, std::vector<double>(23, 0.0), n);  // too few taps
      if (which == 2) SampleRateConverter bad(65, 3, 2, 8, std::vector<double>(24, 0.0), n);
      if (which == 3) SampleRateConverter bad(N, 3, 2, 8, std::vector<double>(24, std::numeric_limits<double>::infinity()), n);
      if (which == 4) SampleRateConverter bad(N, 3, 2, 8, std::vector<double>(24, 0.0), 0);
      if (which == 5) (void)SampleRateConverter::design(3, 2, 8, 10.0, 1.5);
    } catch (const ear::invalid_argument &) {
      threw = true;
    }
    CHECK(threw);
  }

  return summary();
}
