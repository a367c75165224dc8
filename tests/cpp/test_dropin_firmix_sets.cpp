// Drop-in test of the filter sets of ear::hip::FirMatrix, compiled against the C++14 mirror headers only
// (libear_amd/host/ear/...): a matrix made with room for two sets, the second loaded while it runs, a crossfade of one block at
// the start of a call (the one_block shape of tests/firmix_sets_model.py: 3 -> 2 x 129 taps, B = 64, calls of 1, 2 and 4
// blocks, select(1, 1) before block 1).  The output must be the formula of include/earhip.h (group M, FILTER SETS) — written
// out here from the header, in float64, tap by tap: y_from before the select, (1 - a) y_from + a y_to with
// a = (q B + n) / (F B) in the fade, y_to after it — and the refusals must throw ear::invalid_argument.
// Needs a GPU (without one the constructors throw: no CPU fallback).
// Build (one line): g++ -std=c++14 -Wall -Wextra -Werror -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_firmix_sets.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_firmix_sets
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include <ear/hip_firmix.hpp>

#include "dropin_check.h"

using ear::hip::FirMatrix;


static const size_t C = 3, K = 2, J = 129, B = 64, T = 7, n = B * T, S = 1, F = 1;

template <typename Fn>
static bool refused(Fn fn) {
  try {
    fn();
  } catch (const ear::invalid_argument &) {
    return true;
  }
  return false;
}

static double formula(const std::vector<float> &h, const std::vector<std::vector<float>> &x, size_t k, size_t i) {
  double y = 0;
  for (size_t c = 0; c < C; c++)
    for (size_t j = 0; j < J && j <= i; j++) y += (double)h[(k * C + c) * J + j] * (double)x[c][i - j];
  return y;
}

int main() {
  std::mt19937 rng(21);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  std::vector<float> h0(K * C * J), h1(K * C * J);
  for (std::vector<float> *h : {&h0, &h1})
    for (size_t p = 0; p < K * C; p++)
      for (size_t j = 0; j < J; j++) (*h)[p * J + j] = u(rng) * std::exp(-4.0f * (float)j / (float)J);
  std::vector<std::vector<float>> x(C, std::vector<float>(n)), y(K, std::vector<float>(n));
  for (auto &row : x)
    for (auto &v : row) v = u(rng);

  FirMatrix fm(C, K, B, J, h0, 4, 2);
  CHECK(fm.num_inputs() == C && fm.num_outputs() == K && fm.partitions() == 3 && fm.nonzero_pairs() == K * C);
  CHECK(fm.set_loaded(0) && !fm.set_loaded(1) && fm.set_nonzero_pairs(1) == 0);
  CHECK(refused([&] { fm.select(1, 1); }));  // not loaded
  CHECK(refused([&] { fm.load_set(0, h1); }));  // the current set
  CHECK(refused([&] { fm.load_set(1, std::vector<float>(5)); }));
  fm.load_set(1, h1);
  CHECK(fm.set_loaded(1) && fm.set_nonzero_pairs(1) == K * C);
  CHECK(refused([&] { fm.select(1, 65); }));
  CHECK(refused([&] { fm.select(2, 1); }));

  size_t at = 0;
  for (size_t nb : {(size_t)1, (size_t)2, (size_t)4}) {
    if (at == S) {
      fm.select(1, F);
      const FirMatrix::State st = fm.state();
      CHECK(st.current == 1 && st.from == 0 && st.done == 0 && st.total == (int)F);
    }
    std::vector<const float *> ip;
    std::vector<float *> op;
    for (auto &row : x) ip.push_back(row.data() + at * B);
    for (auto &row : y) op.push_back(row.data() + at * B);
    fm.process(nb, ip.data(), op.data());
    at += nb;
  }
  const FirMatrix::State st = fm.state();
  CHECK(st.current == 1 && st.from == -1 && st.done == 0 && st.total == 0);
  CHECK(fm.nonzero_pairs() == K * C);

  double worst = 0;
  for (size_t k = 0; k < K; k++) {
    double num = 0, den = 0;
    for (size_t i = 0; i < n; i++) {
      const size_t t = i / B;
      double want;
      if (t < S) want = formula(h0, x, k, i);
      else if (t >= S + F) want = formula(h1, x, k, i);
      else {
        const double a = (double)((t - S) * B + i % B) / (double)(F * B);
        want = (1.0 - a) * formula(h0, x, k, i) + a * formula(h1, x, k, i);
      }
      const double e = (double)y[k][i] - want;
      num += e * e, den += want * want;
    }
    worst = std::fmax(worst, std::sqrt(num / den));
  }
  std::printf("one_block through the mirror: worst relative error %.3e\n", worst);
  CHECK(worst <= 1e-6);  // float32 partitioned convolution: a few 1e-7

  // reset in mid-fade: the target is current
  fm.select(0, 3);
  {
    std::vector<const float *> ip;
    std::vector<float *> op;
    for (auto &row : x) ip.push_back(row.data());
    for (auto &row : y) op.push_back(row.data());
    fm.process(1, ip.data(), op.data());
  }
  CHECK(fm.state().done == 1 && refused([&] { fm.select(1, 1); }));
  fm.reset();
  CHECK(fm.state().current == 0 && fm.state().from == -1 && fm.set_loaded(1));

  CHECK(refused([&] { FirMatrix none(C, K, B, J, h0, 4, 0); }));
  CHECK(refused([&] { FirMatrix many(C, K, B, J, h0, 4, 4097); }));

  return summary();
}
