// Drop-in test of ear::hip::FirMatrix and ObjectsRenderer::attach_fir_matrix, compiled against the C++14 mirror headers only
// (libear_amd/host/ear/...).  A matrix attached to a renderer must leave in its sink the formula of include/earhip.h
// (group M) — written out here from the header, in float64, tap by tap — over the float samples the renderer returned; a
// stand-alone matrix fed the same rows in the same calls must give the sink's bits; pairs whose taps are all zero are
// dropped; a matrix of the wrong width and a call beyond the sink are refused.
// Needs a GPU (without one the constructors throw: no CPU fallback).
// Build (one line): g++ -std=c++14 -Wall -Wextra -Werror -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_firmix.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_firmix
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <ear/decorrelate.hpp>
#include <ear/dsp/objects_renderer.hpp>
#include <ear/hip_firmix.hpp>

#include "dropin_check.h"

using ear::dsp::ObjectsRenderer;
using ear::hip::FirMatrix;


static const size_t M = 13, N = 6, K = 2, B = 512, T = 6, n = B * T, J = 700, LFE = 3;

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

// the formula of the header in float64; returns the worst ||got - want|| / ||want|| over the outputs
static double worst_error(const std::vector<float> &taps, const std::vector<std::vector<float>> &rows, const float *sink,
                          size_t sink_stride) {
  const size_t len = rows[0].size();
  double worst = 0;
  for (size_t k = 0; k < K; k++) {
    double num = 0, den = 0;
    for (size_t i = 0; i < len; i++) {
      double y = 0;
      for (size_t c = 0; c < N; c++)
        for (size_t j = 0; j < J && j <= i; j++) y += (double)taps[(k * N + c) * J + j] * (double)rows[c][i - j];
      const double e = (double)sink[k * sink_stride + i] - y;
      num += e * e, den += y * y;
    }
    worst = std::fmax(worst, std::sqrt(num / den));
  }
  return worst;
}

int main() {
  const std::vector<std::string> names = {"M+030", "M-030", "M+000", "LFE1", "M+110", "M-110"};
  ObjectsRenderer r(M, N, B, ear::designDecorrelators(names), 255, T);
  set_curves(r);
  ear::hip::Context &ctx = ear::hip::default_context();

  std::mt19937 rng(11);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  std::vector<float> taps(K * N * J);
  for (size_t k = 0; k < K; k++)
    for (size_t c = 0; c < N; c++)
      for (size_t j = 0; j < J; j++) taps[(k * N + c) * J + j] = c == LFE ? 0.0f : u(rng) * std::exp(-4.0f * (float)j / (float)J);
  FirMatrix fm(N, K, B, J, taps, T), alone(N, K, B, J, taps, T);
  CHECK(fm.num_inputs() == N && fm.num_outputs() == K && fm.block_size() == B && fm.partitions() == 2);
  CHECK(fm.nonzero_pairs() == K * (N - 1));  // the LFE's pairs are all zero: dropped

  // two calls of process() from host pointers with the matrix attached; the sink in device-reachable host memory
  const size_t cap = 2 * n, stride = cap + 8;
  float *sink = ctx.alloc_host(K * stride);
  for (size_t i = 0; i < K * stride; i++) sink[i] = 9.0f;
  std::vector<std::vector<float>> in(M, std::vector<float>(2 * n)), out(N, std::vector<float>(2 * n));
  for (auto &row : in)
    for (auto &v : row) v = 0.5f * u(rng);
  std::vector<std::vector<float>> mix(K, std::vector<float>(2 * n));
  r.attach_fir_matrix(fm, sink, stride, cap);
  CHECK(r.fir_matrix_position() == 0);
  for (size_t call = 0; call < 2; call++) {
    std::vector<const float *> ip;
    std::vector<float *> op, mp;
    for (auto &row : in) ip.push_back(row.data() + call * n);
    for (auto &row : out) op.push_back(row.data() + call * n);
    for (auto &row : mix) mp.push_back(row.data() + call * n);
    r.process(T, ip.data(), op.data());
    std::vector<const float *> rp(op.begin(), op.end());
    alone.process(T, rp.data(), mp.data());
  }
  ctx.synchronize();
  CHECK(r.fir_matrix_position() == cap);
  for (size_t k = 0; k < K; k++) {
    CHECK(std::memcmp(sink + k * stride, mix[k].data(), cap * sizeof(float)) == 0);
    for (size_t i = cap; i < stride; i++) CHECK(sink[k * stride + i] == 9.0f);
  }
  const double worst = worst_error(taps, out, sink, stride);
  std::printf("attached through process(): worst relative error %.3e\n", worst);
  CHECK(worst <= 1e-6);  // float32 partitioned convolution: a few 1e-7

  // the sink is full: the next call is refused before anything is rendered, in every form
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
  CHECK(threw && r.fir_matrix_position() == cap);

  // attaching again rewinds; reset() of the renderer leaves the matrix alone; the PCM-out form feeds it too
  r.attach_fir_matrix(fm, sink, stride, cap);
  CHECK(r.fir_matrix_position() == 0);
  r.reset(0);
  std::vector<int16_t> frames(n * M), pcm(n * N);
  for (auto &v : frames) v = (int16_t)(rng() & 0xFFFF);
  r.process_frames(T, frames.data(), (int)M, 0, pcm.data());
  CHECK(r.fir_matrix_position() == n);
  r.detach_fir_matrix();
  r.process_frames(T, frames.data(), (int)M, 0, pcm.data());
  CHECK(r.fir_matrix_position() == 0);  // detached

  // a matrix of the wrong width or block size is refused
  FirMatrix wide(N + 1, K, B, 4, std::vector<float>((N + 1) * K * 4, 1.0f)), small(N, K, B / 2, 4, std::vector<float>(N * K * 4, 1.0f));
  for (FirMatrix *w : {&wide, &small}) {
    CHECK_THROWS_AS(r.attach_fir_matrix(*w, sink, stride, cap), ear::invalid_argument);
  }
  CHECK_THROWS_AS(FirMatrix bad(N, K, 96, 4, std::vector<float>(N * K * 4, 1.0f)), ear::invalid_argument);

  return summary();
}
