// Drop-in test of ObjectsRenderer::process_frames: a libear application's render loop fed with interleaved PCM frames (as a
// BW64 reader hands them over), compiled against the C++14 mirror headers only (libear_amd/host/ear/...).  It renders s16 and
// s24 frames (an odd channel offset inside wider frames; planar and interleaved outputs) and checks
// each against ObjectsRenderer::process on the same samples converted to float rows by the rules of include/earhip.h, bit for
// bit.  Needs a GPU (without one the renderer's constructor throws: no CPU fallback).
// Build (one line): g++ -std=c++14 -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_frames.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_frames
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include <ear/decorrelate.hpp>
#include <ear/dsp/objects_renderer.hpp>

#include "dropin_check.h"

using ear::dsp::ObjectsRenderer;


static const size_t M = 13, N = 6, B = 512, T = 4, n = B * T;
static const int C = 2 * (int)M + 1, FIRST = 5;

static void set_curves(ObjectsRenderer &r) {
  for (size_t m = 0; m < M; m++) {
    std::vector<std::vector<float>> d, f;
    for (int k = 0; k < 3; k++) {
      std::vector<float> g(N), h(N);
      for (size_t c = 0; c < N; c++) g[c] = 0.05f * (float)((m + c + k) % 7), h[c] = 0.03f * (float)((m * 3 + c + 2 * k) % 5);
      d.push_back(g), f.push_back(h);
    }
    r.set_object_points(m, {0, (int64_t)(700 + 37 * m), (int64_t)n}, d, f);
  }
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(float) * a.size()) == 0;
}

// renders the planar rows x [M][n] with process(), and the frames with process_frames(); fresh renderers, same curves
template <typename Sample>
static void check_form(const char *name, const std::vector<Sample> &frames, const std::vector<float> &x) {
  const std::vector<std::string> names{"M+030", "M-030", "M+000", "LFE1", "M+110", "M-110"};
  const auto dec = ear::designDecorrelators(names);
  std::vector<float> want(N * n), got(N * n), got_ilv(n * N);
  {
    ObjectsRenderer r(M, N, B, dec, 255, T);
    set_curves(r);
    std::vector<const float *> ip(M);
    std::vector<float *> op(N);
    for (size_t m = 0; m < M; m++) ip[m] = x.data() + m * n;
    for (size_t c = 0; c < N; c++) op[c] = want.data() + c * n;
    r.process(T, ip.data(), op.data());
  }
  {
    ObjectsRenderer r(M, N, B, dec, 255, T);
    set_curves(r);
    std::vector<float *> op(N);
    for (size_t c = 0; c < N; c++) op[c] = got.data() + c * n;
    r.process_frames(T, frames.data(), C, FIRST, op.data());
  }
  {
    ObjectsRenderer r(M, N, B, dec, 255, T);
    set_curves(r);
    r.process_frames(T, frames.data(), C, FIRST, got_ilv.data());
  }
  std::vector<float> ilv_planar(N * n);
  for (size_t f = 0; f < n; f++)
    for (size_t c = 0; c < N; c++) ilv_planar[c * n + f] = got_ilv[f * N + c];
  bool nonzero = false;
  for (float v : want) nonzero = nonzero || v != 0.0f;
  CHECK(nonzero);
  CHECK(same_bits(got, want));
  CHECK(same_bits(ilv_planar, want));
  std::printf("%s: planar %s, interleaved %s\n", name, same_bits(got, want) ? "bit-identical" : "DIFFERS",
              same_bits(ilv_planar, want) ? "bit-identical" : "DIFFERS");
}

int main() {
  std::mt19937 rng(11);
  try {
    {  // s16, the common file format: (float)x * 2^-15
      std::vector<int16_t> frames(n * C);
      for (auto &v : frames) v = (int16_t)(rng() & 0xffff);
      frames[FIRST] = -32768, frames[FIRST + 1] = 32767;
      std::vector<float> x(M * n);
      for (size_t f = 0; f < n; f++)
        for (size_t m = 0; m < M; m++) x[m * n + f] = (float)frames[f * C + FIRST + m] * (1.0f / 32768.0f);
      check_form("s16", frames, x);
    }
    {  // s24, 3 bytes a sample, little-endian, sign-extended: (float)x * 2^-23
      std::vector<uint8_t> frames(n * C * 3);
      for (auto &v : frames) v = (uint8_t)(rng() & 0xff);
      std::vector<float> x(M * n);
      for (size_t f = 0; f < n; f++)
        for (size_t m = 0; m < M; m++) {
          const uint8_t *p = frames.data() + (f * C + FIRST + m) * 3;
          int32_t v = (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
          if (v & 0x800000) v -= 0x1000000;
          x[m * n + f] = (float)v * (1.0f / 8388608.0f);
        }
      check_form("s24", frames, x);
    }
  } catch (const std::exception &e) {
    std::printf("FAILED: %s\n", e.what());
    return 1;
  }
  return summary();
}
