// pcm_convert.h — the float -> PCM conversion include/earhip.h defines for earhip_render_process_frames_pcm (group F), as one
// function the device kernel (pcm_out_kernels.h) and a plain C++ program on the CPU (tests/cpp/test_pcm_convert.cpp) both compile:
// what is tested against the numpy model on the CPU is the code the kernel runs — and the host fold of the levels that kernel
// keeps (pcm_levels_fold).  No HIP header is needed to include it.
//
// Every floating-point step is ONE float32 operation rounded once.  What keeps the dither add apart from the multiply before it
// is the build's -ffp-contract=off (csrc/Makefile; the host test passes it too): __fadd_rn is a plain add to this compiler.
// Were the two ever fused the samples would not change — x * 2^15 is exact, so fma(x, 2^15, d) rounds to the same value, and an
// overflow saturates either way — but the definition is the two-step one.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EARHIP_PCM_HD __host__ __device__
#else
#define EARHIP_PCM_HD
#endif

namespace earhip {

// formats as earhip_pcm_format
constexpr int kPcmS16 = 1, kPcmS24 = 2, kPcmS32 = 3, kPcmF32 = 4;

// one round of the hash: Wellons' "lowbias32" finaliser (public domain), a bijection of 32-bit words
EARHIP_PCM_HD inline uint32_t pcm_mix32(uint32_t a) {
  a ^= a >> 16;
  a *= 0x7FEB352Du;
  a ^= a >> 15;
  a *= 0x846CA68Bu;
  a ^= a >> 16;
  return a;
}

// h(seed, t, n): four rounds, one per word, the seed last (two seeds are then related by a pseudo-random permutation of
// (t, n), not by a shift in time).  t: the sample clock as the 64 bits of its two's complement.
EARHIP_PCM_HD inline uint32_t pcm_dither_hash(uint32_t seed, uint64_t t, uint32_t n) {
  uint32_t h = pcm_mix32((uint32_t)t + 0x9E3779B9u);
  h = pcm_mix32(h ^ (uint32_t)(t >> 32));
  h = pcm_mix32(h + n * 0x85EBCA6Bu);
  return pcm_mix32(h ^ seed);
}

// TPDF over (-1, 1) LSB: the sum of the hash's two 16-bit halves, centred; every value is a multiple of 2^-16, exact in float32
EARHIP_PCM_HD inline float pcm_dither_value(uint32_t h) {
  return (float)((int)(h & 0xFFFFu) + (int)(h >> 16) - 65535) * 0x1p-16f;
}

EARHIP_PCM_HD inline float pcm_add_once(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(a, b);
#else
  volatile float s = a + b;  // (a separate rounding whatever the host compiler's contraction setting is)
  return s;
#endif
}

// x -> the stored integer (FMT = S16 / S24 / S32); *clipped: saturation changed the rounded value, or x + dither was NaN.
// d: the dither value (S16 with dither only; kDither = false leaves the add out altogether).
template <int FMT, bool kDither>
EARHIP_PCM_HD inline int32_t pcm_from_float(float x, float d, bool *clipped) {
  constexpr float scale = FMT == kPcmS16 ? 0x1p15f : FMT == kPcmS24 ? 0x1p23f : 0x1p31f;
  constexpr float hi = scale, lo = -scale;  // in range: lo <= r < hi (hi itself does not fit the format)
  constexpr int32_t qmax = FMT == kPcmS16 ? 32767 : FMT == kPcmS24 ? 8388607 : INT32_MAX, qmin = -qmax - 1;
  const float p = x * scale;
  const float v = kDither ? pcm_add_once(p, d) : p;
  const float r = rintf(v);  // round to nearest, ties to even (the default rounding mode; v_rndne_f32 on the device)
  if (!(r == r)) {
    *clipped = true;
    return 0;
  }
  if (r >= hi) {
    *clipped = true;
    return qmax;
  }
  if (r < lo) {
    *clipped = true;
    return qmin;
  }
  *clipped = false;
  return (int32_t)r;  // (exact: r is an integer inside the range of int32)
}

// The levels of the kernel that converts (pcm_out_kernels.h keeps `slots` copies [slots][C] of each, so that its waves do not all
// meet on C addresses) folded on the host: per channel the largest of the peaks' bit patterns — bits of non-negative floats order
// as integers — and the sum of the clip counts.
inline void pcm_levels_fold(int slots, int C, const unsigned *peak_bits, const unsigned long long *clip_counts, float *peak,
                            uint64_t *clipped) {
  for (int c = 0; c < C; c++) {
    unsigned m = 0;
    uint64_t sum = 0;
    for (size_t at = (size_t)c; at < (size_t)slots * (size_t)C; at += (size_t)C) {
      if (peak_bits[at] > m) m = peak_bits[at];
      sum += clip_counts[at];
    }
    std::memcpy(&peak[c], &m, sizeof(float));
    clipped[c] = sum;
  }
}

}  // namespace earhip
