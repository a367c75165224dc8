// Drop-in test of the PCM-out overloads of ObjectsRenderer::process_frames (file to file: interleaved PCM frames in, interleaved
// PCM frames out), compiled against the C++14 mirror headers only (libear_amd/host/ear/...).  Each overload — typed by its output
// pointer: int16_t s16, uint8_t s24, int32_t s32 — must give the bytes of the C call earhip_render_process_frames_pcm on a
// renderer with the same curves, with and without dither, and output_levels() the numbers of earhip_render_output_levels.
// Needs a GPU (without one the renderer's constructor throws: no CPU fallback).
// Build (one line): g++ -std=c++14 -Wall -Wextra -Werror -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_pcm_out.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_pcm_out
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <ear/decorrelate.hpp>
#include <ear/dsp/objects_renderer.hpp>

#include "dropin_check.h"

using ear::dsp::ObjectsRenderer;


static const size_t M = 13, N = 6, B = 512, T = 4, n = B * T;
static const int C = 2 * (int)M + 1, FIRST = 5;

static std::vector<std::vector<float>> decorrelators() {
  return ear::designDecorrelators(std::vector<std::string>{"M+030", "M-030", "M+000", "LFE1", "M+110", "M-110"});
}

static void curve(size_t m, std::vector<int64_t> &t, std::vector<std::vector<float>> &d, std::vector<std::vector<float>> &f) {
  t = {0, (int64_t)(700 + 37 * m), (int64_t)n};
  d.clear(), f.clear();
  for (int k = 0; k < 3; k++) {
    std::vector<float> g(N), h(N);
    for (size_t c = 0; c < N; c++) g[c] = 0.25f * (float)((m + c + k) % 7), h[c] = 0.15f * (float)((m * 3 + c + 2 * k) % 5);
    d.push_back(g), f.push_back(h);
  }
}

// the same scene through the C ABI
static earhip_render *c_renderer(ear::hip::Context &ctx) {
  const auto dec = decorrelators();
  std::vector<float> flat;
  for (auto &v : dec) flat.insert(flat.end(), v.begin(), v.end());
  earhip_render_config cfg;
  cfg.n_objects = (int)M, cfg.n_out = (int)N, cfg.block_size = (int)B, cfg.n_buses = 2;
  cfg.decorrelators = flat.data(), cfg.n_taps = (int)dec[0].size(), cfg.delay = 255, cfg.max_blocks = (int)T;
  earhip_render *r = nullptr;
  ear::hip::check(earhip_render_create(ctx.get(), &cfg, &r));
  for (size_t m = 0; m < M; m++) {
    std::vector<int64_t> t;
    std::vector<std::vector<float>> d, f;
    curve(m, t, d, f);
    std::vector<float> df, ff;
    for (auto &v : d) df.insert(df.end(), v.begin(), v.end());
    for (auto &v : f) ff.insert(ff.end(), v.begin(), v.end());
    ear::hip::check(earhip_render_set_object_points(r, (int)m, 3, t.data(), df.data(), ff.data()));
  }
  return r;
}

template <typename Out>
static void check_form(const char *name, earhip_pcm_format out_fmt, size_t sample_bytes, const std::vector<int16_t> &frames, bool dither) {
  ear::hip::Context &ctx = ear::hip::default_context();
  std::vector<uint8_t> want(n * N * sample_bytes, 0xAB), got(n * N * sample_bytes, 0xCD);
  std::vector<float> peak_c(N);
  std::vector<uint64_t> clip_c(N);
  {
    earhip_render *r = c_renderer(ctx);
    ear::hip::check(earhip_render_reset(r, 1000));
    earhip_pcm_out o;
    o.format = out_fmt, o.dither = dither ? 1 : 0, o.seed = 42;
    ear::hip::check(earhip_render_process_frames_pcm(r, T, frames.data(), EARHIP_PCM_S16, C, FIRST, want.data(), &o));
    ear::hip::check(earhip_render_output_levels(r, peak_c.data(), clip_c.data(), 0));
    earhip_render_destroy(r);
  }
  std::vector<float> peak;
  std::vector<uint64_t> clip;
  {
    ObjectsRenderer r(M, N, B, decorrelators(), 255, T);
    for (size_t m = 0; m < M; m++) {
      std::vector<int64_t> t;
      std::vector<std::vector<float>> d, f;
      curve(m, t, d, f);
      r.set_object_points(m, t, d, f);
    }
    r.reset(1000);
    r.process_frames(T, frames.data(), C, FIRST, reinterpret_cast<Out *>(got.data()), ObjectsRenderer::PcmOutOptions(dither, 42));
    r.output_levels(peak, clip);
  }
  const bool same = want == got;
  uint64_t clipped = 0;
  bool differs = false;
  for (size_t i = 1; i < want.size(); i++) differs = differs || want[i] != want[0];
  for (auto c : clip) clipped += c;
  CHECK(differs);
  CHECK(same);
  CHECK(peak.size() == N && clip.size() == N);
  CHECK(std::memcmp(peak.data(), peak_c.data(), sizeof(float) * N) == 0);
  CHECK(clip == clip_c);
  CHECK(clipped > 0 && clipped < (uint64_t)(n * N));
  std::printf("%s%s: %s, %llu clipped\n", name, dither ? " dither" : "", same ? "byte-identical" : "DIFFERS", (unsigned long long)clipped);
}

int main() {
  std::mt19937 rng(11);
  try {
    std::vector<int16_t> frames(n * C);
    for (auto &v : frames) v = (int16_t)(rng() & 0xffff);
    check_form<int16_t>("s16", EARHIP_PCM_S16, 2, frames, false);
    check_form<int16_t>("s16", EARHIP_PCM_S16, 2, frames, true);
    check_form<uint8_t>("s24", EARHIP_PCM_S24, 3, frames, false);
    check_form<int32_t>("s32", EARHIP_PCM_S32, 4, frames, false);
    // dither with another format is libear's invalid_argument
    bool threw = false;
    try {
      ObjectsRenderer r(M, N, B, decorrelators(), 255, T);
      std::vector<uint8_t> out(n * N * 3);
      r.process_frames(T, frames.data(), C, FIRST, out.data(), ObjectsRenderer::PcmOutOptions(true, 1));
    } catch (const ear::invalid_argument &) {
      threw = true;
    }
    CHECK(threw);
  } catch (const std::exception &e) {
    std::printf("FAILED: %s\n", e.what());
    return 1;
  }
  return summary();
}
