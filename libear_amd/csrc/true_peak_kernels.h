// true_peak_kernels.h — the device side of the true-peak meter (include/earhip.h, group L; the maths: true_peak.h).
//
// The interpolator is not recursive, so a launch is cut per channel into tiles that know nothing of each other.  Two kernels:
//   k_true_peak_4x12   the shape of BS.1770-4's table (4 phases of 12 taps; the coefficients travel as kernel arguments and
//                      sit in scalar registers).  A wave takes 512 consecutive samples, a lane a RUN of 8 of them: its 8 + 11
//                      inputs are read once from LDS into registers and the window slides over them with compile-time
//                      indices: 19 LDS reads for 8 x 48 multiply-adds.  The wave's 523 inputs are fetched coalesced (lane l
//                      takes sample l of every 64) and laid down with one pad word after every 8, so that the lanes' runs,
//                      9 words apart, start on different banks.  Measured alike within 2 us of 28: runs of 4, 8 and 16, 4 or
//                      8 waves per SIMD, coefficients in vector registers.
//   k_true_peak_any    any table up to 8 x 64 from device memory, a lane per sample.  Nothing hot runs through it.
// Both read the taps - 1 samples in front of the launch from the history buffer hist_in and leave the launch's last taps - 1
// in hist_out, the OTHER of two buffers: the first tile may still be reading while the last one's samples are written.
// The maxima: max is exact and order-free, and non-negative floats order like their bit patterns, so a wave reduces its
// samples to one number per 100 ms step it touches (one step for nine tiles in ten) and folds it into the step's word of the
// store with an integer atomic max (a vector memory operation): the same samples give the same bits however they were cut or
// scheduled.  The word of the step a call leaves open is simply the next row of the store: it goes on growing in the next call.
#pragma once
#include <hip/hip_runtime.h>

#include "true_peak.h"

namespace earhip {

constexpr int kTpRun = 8;                              // consecutive samples of a lane
constexpr int kTpWaveTile = 64 * kTpRun;               // samples of a wave
constexpr int kTpWaves = 4;                            // waves of a workgroup
constexpr int kTpBlockTile = kTpWaves * kTpWaveTile;   // samples of a workgroup
constexpr int kTpHalo = 11;                            // taps - 1 of the 4 x 12 shape
constexpr int kTpWindow = kTpWaveTile + kTpHalo;       // inputs of a wave
constexpr int kTpLds = kTpWindow + kTpWindow / kTpRun + 1;  // ... with a pad word after every run
constexpr int kTpAnyTile = 256;                        // samples of a workgroup of k_true_peak_any
constexpr int kTpHist = kTpMaxTaps - 1;                // floats of history per channel and buffer

struct TpArgs {
  const float *rows;  // [C][stride], samples [0, n) of this launch
  size_t stride;
  unsigned n;
  int C;
  unsigned r0;               // clock of sample 0 modulo the step
  unsigned step;             // samples of a step
  unsigned long long step0;  // the step sample 0 lies in
  const float *hist_in;      // [C][kTpHist]: entry taps - 1 + i is sample i < 0 of the launch
  float *hist_out;           // [C][kTpHist]
  unsigned *tp, *sp;         // [max_steps + 1][C] bit patterns of non-negative floats
  int phases, taps;
  const float *table;  // [phases][taps] in device memory (k_true_peak_any)
  float h[4][12];      // (k_true_peak_4x12)
};

// The largest of a non-negative, non-NaN float over the wave, in every lane.  Such floats order like their bit patterns, so
// this is an unsigned max; it runs on the vector ALU's own lane permutes (DPP), not through LDS: rotations by 8, 4, 2, 1 inside
// each row of 16 lanes leave the row's maximum in all of its lanes (max is idempotent), lane 15 of rows 0 and 2 is handed to
// rows 1 and 3, lane 31 to rows 2 and 3, and lane 63 holds the result.
__device__ inline float tp_wave_max(float v) {
  unsigned x = __float_as_uint(v);
#define EARHIP_TP_DPP(ctrl, rows) x = max(x, (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, ctrl, rows, 0xf, false))
  EARHIP_TP_DPP(0x128, 0xf);  // row_ror:8
  EARHIP_TP_DPP(0x124, 0xf);  // row_ror:4
  EARHIP_TP_DPP(0x122, 0xf);  // row_ror:2
  EARHIP_TP_DPP(0x121, 0xf);  // row_ror:1
  EARHIP_TP_DPP(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
  EARHIP_TP_DPP(0x143, 0xc);  // row_bcast:31 into rows 2 and 3
#undef EARHIP_TP_DPP
  return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)x, 63));
}

// (zero is what the store holds already)
__device__ inline void tp_fold(unsigned *word, float v) {
  const unsigned b = __float_as_uint(v);
  if (b) atomicMax(word, b);
}

// sample i of the launch, i >= -halo; unconditional, the index clamped into what exists (a clamped value is never consumed)
__device__ inline float tp_sample(const float *row, const float *hist, int halo, int last, int i) {
  const float *p = i < 0 ? hist + max(halo + i, 0) : row + min(i, last);
  return *p;
}

// the launch's last `halo` samples (older ones from the history where the launch is shorter than that) -> the other buffer
__device__ inline void tp_keep_history(const TpArgs &a, const float *row, const float *hist, int ch, int halo, int t) {
  if (t < halo) {
    const int i = (int)a.n - halo + t;
    a.hist_out[(size_t)ch * kTpHist + t] = i < 0 ? hist[halo + i] : row[i];
  }
}

// (the limiter's kernels, limiter_kernels.h, share everything above this line and define EARHIP_TP_HELPERS_ONLY: the meter's
// kernels exist once, in api_loudness.hip)
#ifndef EARHIP_TP_HELPERS_ONLY
__global__ __launch_bounds__(64 * kTpWaves) void k_true_peak_4x12(TpArgs a) {
  __shared__ float tile[kTpWaves][kTpLds];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ch = blockIdx.y;
  const int base = (int)blockIdx.x * kTpBlockTile + wave * kTpWaveTile;  // the wave's first sample of the launch
  const float *row = a.rows + (size_t)ch * a.stride;
  const float *hist = a.hist_in + (size_t)ch * kTpHist;
  const int last = (int)a.n - 1;
  float *t = tile[wave];
  // window word w is sample base - 11 + w.  A wave whose window lies inside the launch's samples (all but the first and
  // the last of a row) loads it from one address with immediate offsets; the others clamp, and read the history
  const bool inside = base >= kTpHalo && base + kTpWaveTile <= (int)a.n;  // (uniform over the wave)
  if (inside) {
    const float *p = row + (base - kTpHalo) + lane;
    float v[(kTpWindow + 63) / 64];
#pragma unroll
    for (int k = 0; k < kTpWaveTile / 64; k++) v[k] = p[64 * k];
    v[kTpWaveTile / 64] = lane < kTpHalo ? p[kTpWaveTile] : 0.0f;
#pragma unroll
    for (int k = 0; k < (kTpWindow + 63) / 64; k++) {
      const int w = lane + 64 * k;
      if (w < kTpWindow) t[w + w / kTpRun] = v[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < (kTpWindow + 63) / 64; k++) {
      const int w = lane + 64 * k;
      const float v = tp_sample(row, hist, kTpHalo, last, base - kTpHalo + w);
      if (w < kTpWindow) t[w + w / kTpRun] = v;
    }
  }
  if (blockIdx.x == 0) tp_keep_history(a, row, hist, ch, kTpHalo, (int)threadIdx.x);
  __syncthreads();
  if (base > last) return;
  float x[kTpRun + kTpHalo];  // the lane's run j = 0 .. 7 is x[11 + j]
#pragma unroll
  for (int m = 0; m < kTpRun + kTpHalo; m++) x[m] = t[(kTpRun + 1) * lane + m + m / kTpRun];
  // output p of the lane's sample j (true_peak.h's dot product, unrolled over registers)
  auto y = [&](int j, int p) { return tp_dot_n<12>(a.h[p], [&](int k) { return x[kTpHalo + j - k]; }); };
  // the steps of the wave's samples, counted from the launch's first step (all of this is uniform over the wave)
  const unsigned rb = a.r0 + (unsigned)base;
  const unsigned sA = rb / a.step;
  const bool one = base + kTpWaveTile <= (int)a.n && (rb + kTpWaveTile - 1) / a.step == sA;
  unsigned *tpA = a.tp + (size_t)(a.step0 + sA) * a.C + ch, *spA = a.sp + (size_t)(a.step0 + sA) * a.C + ch;
  if (one) {
    // every sample of the wave lies in one step: two running maxima
    float mt = 0.0f, ms = 0.0f;
#pragma unroll
    for (int j = 0; j < kTpRun; j++) {
      mt = tp_absmax(tp_absmax(mt, y(j, 0)), y(j, 1));
      mt = tp_absmax(tp_absmax(mt, y(j, 2)), y(j, 3));
      ms = tp_absmax(ms, x[kTpHalo + j]);
    }
    mt = tp_wave_max(mt), ms = tp_wave_max(ms);
    if (lane == 0) tp_fold(tpA, mt), tp_fold(spA, ms);
    return;
  }
  float tp[kTpRun], sp[kTpRun];
#pragma unroll
  for (int j = 0; j < kTpRun; j++) {
    tp[j] = tp_absmax(tp_absmax(tp_absmax(tp_absmax(0.0f, y(j, 0)), y(j, 1)), y(j, 2)), y(j, 3));
    sp[j] = tp_absmax(0.0f, x[kTpHalo + j]);
  }
  // a tile across a step boundary, or the launch's last: samples of the wave's first step, of the one after it, and (steps
  // shorter than a tile) of any later one, which go to the store one by one
  const unsigned rl = rb + (unsigned)(kTpRun * lane);
  unsigned s = rl / a.step, rem = rl - s * a.step;
  float mtA = 0.0f, msA = 0.0f, mtB = 0.0f, msB = 0.0f;
#pragma unroll
  for (int j = 0; j < kTpRun; j++) {
    if (base + kTpRun * lane + j <= last) {
      if (s == sA) {
        mtA = fmaxf(mtA, tp[j]), msA = fmaxf(msA, sp[j]);
      } else if (s == sA + 1) {
        mtB = fmaxf(mtB, tp[j]), msB = fmaxf(msB, sp[j]);
      } else {
        tp_fold(a.tp + (size_t)(a.step0 + s) * a.C + ch, tp[j]);
        tp_fold(a.sp + (size_t)(a.step0 + s) * a.C + ch, sp[j]);
      }
    }
    if (++rem == a.step) rem = 0, s++;
  }
  mtA = tp_wave_max(mtA), msA = tp_wave_max(msA), mtB = tp_wave_max(mtB), msB = tp_wave_max(msB);
  if (lane == 0) {
    tp_fold(tpA, mtA), tp_fold(spA, msA);
    tp_fold(tpA + a.C, mtB), tp_fold(spA + a.C, msB);  // (zero where the wave has no sample there: nothing is written)
  }
}

__global__ __launch_bounds__(kTpAnyTile) void k_true_peak_any(TpArgs a) {
  __shared__ float xs[kTpAnyTile + kTpHist];
  __shared__ float hs[kTpMaxPhases * kTpMaxTaps];
  const int tid = threadIdx.x, lane = tid & 63, ch = blockIdx.y;
  const int halo = a.taps - 1;
  const int base = (int)blockIdx.x * kTpAnyTile;
  const float *row = a.rows + (size_t)ch * a.stride;
  const float *hist = a.hist_in + (size_t)ch * kTpHist;
  const int last = (int)a.n - 1;
  for (int w = tid; w < kTpAnyTile + halo; w += kTpAnyTile) xs[w] = tp_sample(row, hist, halo, last, base - halo + w);
  for (int i = tid; i < a.phases * a.taps; i += kTpAnyTile) hs[i] = a.table[i];
  if (blockIdx.x == 0) tp_keep_history(a, row, hist, ch, halo, tid);
  __syncthreads();
  const int i = base + tid;
  const float *at = xs + halo + tid;
  float mt = 0.0f;
  for (int p = 0; p < a.phases; p++) mt = tp_absmax(mt, tp_dot(hs + p * a.taps, a.taps, [&](int k) { return at[-k]; }));
  float ms = tp_absmax(0.0f, at[0]);
  const unsigned r = a.r0 + (unsigned)i, s = r / a.step;
  const int w0 = base + (tid - lane);  // the wave's first sample
  const unsigned sA = (a.r0 + (unsigned)w0) / a.step;
  const bool one = w0 + 64 <= (int)a.n && (a.r0 + (unsigned)w0 + 63u) / a.step == sA;  // uniform over the wave
  if (one) {
    mt = tp_wave_max(mt), ms = tp_wave_max(ms);
    if (lane == 0) tp_fold(a.tp + (size_t)(a.step0 + sA) * a.C + ch, mt), tp_fold(a.sp + (size_t)(a.step0 + sA) * a.C + ch, ms);
  } else if (i <= last) {
    tp_fold(a.tp + (size_t)(a.step0 + s) * a.C + ch, mt), tp_fold(a.sp + (size_t)(a.step0 + s) * a.C + ch, ms);
  }
}

// The peaks so far: the maximum over rows [0, rows) of both stores, per channel -> out [2][C] (true peak, sample peak).
// One workgroup per (channel, store); rows are few (ten a second of programme).
__global__ __launch_bounds__(256) void k_true_peak_totals(const unsigned *tp, const unsigned *sp, unsigned long long rows, int C,
                                                          unsigned *out) {
  __shared__ unsigned part[4];
  const int ch = blockIdx.x, which = blockIdx.y, tid = threadIdx.x;
  const unsigned *src = which ? sp : tp;
  unsigned m = 0;
  for (unsigned long long r = (unsigned long long)tid; r < rows; r += 256) m = max(m, src[r * (unsigned long long)C + ch]);
  m = __float_as_uint(tp_wave_max(__uint_as_float(m)));
  if ((tid & 63) == 0) part[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) out[(size_t)which * C + ch] = max(max(part[0], part[1]), max(part[2], part[3]));
}
#endif  // EARHIP_TP_HELPERS_ONLY

}  // namespace earhip
