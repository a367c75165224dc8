// limiter_kernels.h — the device side of the look-ahead limiter (include/earhip.h, group N; the maths: limiter.h, true_peak.h).
//
// Two passes per launch, neither recursive, so both are cut along the time axis into tiles that know nothing of each other:
//   k_lim_detect_*     all channels of a time tile -> one row r[n] of required gains (scratch of the limiter, [max launch]).
//     _4x12   the shape of BS.1770-4's table: k_true_peak_4x12's inner loop (a lane takes a run of 8 samples, reads its 8 + 11
//             inputs once from padded LDS into registers, coefficients in scalar registers).  A workgroup of 4 waves takes ONE
//             tile of 512 samples; wave w takes channels w, w + 4, ... and keeps the running maximum over them in registers; the
//             four waves' maxima meet in LDS and 256 threads write r with whole lines.
//     _any    any table up to 8 x 64 from device memory, a lane per sample (as k_true_peak_any).
//     _sample detect = 0: the largest |x| over the channels, a lane per sample.
//   k_lim_apply        a workgroup takes 1024 output samples: r over [tile start - (M - 1) - L, tile end) into LDS (history from
//             rhist_in), the sliding minimum of width M there by doubling (a[i] = min(a[i], a[i - s]), s = 1, 2, 4 ..: widths
//             1, 2, 4 .. P, then min(a_P[i], a_P[i - (M - P)]); min is exact, so this is the definition's result), the K-term
//             sums in the prescribed order (limiter.h: lim_sum), g = min(s / K, r[n - L]), the statistics (a wave reduces its
//             samples and lane 0 issues one integer atomic max and one 64-bit atomic add, vector memory operations, into one of
//             kLimSlots copies), and then every channel's delayed row of the tile times g, whole lines in and out.
// History: both passes read the samples and gains in front of the launch from xhist_in / rhist_in; k_lim_apply leaves the
// launch's last ones in xhist_out / rhist_out, the OTHER of two buffers (the first tile may still be reading).
#pragma once
#include <hip/hip_runtime.h>

#include "limiter.h"
#define EARHIP_TP_HELPERS_ONLY  // the tile constants, tp_wave_max and tp_sample; not the meter's kernels
#include "true_peak_kernels.h"
#undef EARHIP_TP_HELPERS_ONLY

namespace earhip {

constexpr int kLimDetWaves = 4;
constexpr int kLimAnyTile = 256;
constexpr int kLimTile = 1024, kLimThreads = 256, kLimRun = kLimTile / kLimThreads;
constexpr int kLimMaxWindow = kLimTile + (kLimMaxLookahead + 2 + kLimMaxHold) - 1 + kLimMaxLookahead;  // floats of r of a tile
constexpr int kLimPer = (kLimMaxWindow + kLimThreads - 1) / kLimThreads;
constexpr int kLimSlots = 64;
constexpr unsigned kLimOneBits = 0x3F800000u;  // 1.0f

struct LimArgs {
  const float *in;  // [C][in_stride], samples [0, n) of this launch
  size_t in_stride;
  float *out;  // [C][out_stride]
  size_t out_stride;
  float *gain;  // [n] or nullptr
  unsigned n;
  int C;
  float c;
  int L, M, K, D, HX, HR, phases, taps;
  const float *xhist_in;  // [C][HX]: entry HX + i is sample i < 0 of the launch
  float *xhist_out;
  const float *rhist_in;  // [HR]: entry HR + i is r of sample i < 0
  float *rhist_out;
  float *r;                         // [n]
  unsigned *stat_min;               // [kLimSlots] the largest (bits of 1.0f) - (bits of g)
  unsigned long long *stat_count;   // [kLimSlots] samples with g < 1
  const float *table;               // [phases][taps] in device memory (k_lim_detect_any)
  float h[4][12];                   // (k_lim_detect_4x12)
};

__global__ __launch_bounds__(64 * kLimDetWaves) void k_lim_detect_4x12(LimArgs a) {
  __shared__ float tile[kLimDetWaves][kTpLds];
  __shared__ float emax[kLimDetWaves][kTpWaveTile + kTpWaveTile / kTpRun];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int base = (int)blockIdx.x * kTpWaveTile;  // the workgroup's first sample of the launch
  const int last = (int)a.n - 1;
  float *t = tile[wave];
  const bool inside = base >= kTpHalo && base + kTpWaveTile <= (int)a.n;  // (uniform over the workgroup)
  float e[kTpRun];
#pragma unroll
  for (int j = 0; j < kTpRun; j++) e[j] = 0.0f;
  for (int c0 = 0; c0 < a.C; c0 += kLimDetWaves) {
    const int ch = c0 + wave;  // (uniform over the wave)
    if (ch < a.C) {
      const float *row = a.in + (size_t)ch * a.in_stride;
      const float *hist = a.xhist_in + (size_t)ch * a.HX + (a.HX - kTpHalo);
      // window word w is sample base - 11 + w (k_true_peak_4x12's two ways of loading it)
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
    }
    __syncthreads();
    if (ch < a.C) {
      float x[kTpRun + kTpHalo];  // the lane's run j = 0 .. 7 is x[11 + j]
#pragma unroll
      for (int m = 0; m < kTpRun + kTpHalo; m++) x[m] = t[(kTpRun + 1) * lane + m + m / kTpRun];
      auto y = [&](int j, int p) { return tp_dot_n<12>(a.h[p], [&](int k) { return x[kTpHalo + j - k]; }); };
#pragma unroll
      for (int j = 0; j < kTpRun; j++) {
        float m = tp_absmax(e[j], x[kTpHalo + j - 6]);  // D = 12 / 2
        m = tp_absmax(tp_absmax(m, y(j, 0)), y(j, 1));
        e[j] = tp_absmax(tp_absmax(m, y(j, 2)), y(j, 3));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < kTpRun; j++) emax[wave][(kTpRun + 1) * lane + j] = e[j];
  __syncthreads();
  for (int i = (int)threadIdx.x; i < kTpWaveTile; i += 64 * kLimDetWaves) {
    const int w = i + i / kTpRun;
    const float v = fmaxf(fmaxf(emax[0][w], emax[1][w]), fmaxf(emax[2][w], emax[3][w]));
    if (base + i <= last) a.r[base + i] = lim_required_gain(a.c, v);
  }
}

__global__ __launch_bounds__(kLimAnyTile) void k_lim_detect_any(LimArgs a) {
  __shared__ float xs[kLimAnyTile + kTpHist];
  __shared__ float hs[kTpMaxPhases * kTpMaxTaps];
  const int tid = threadIdx.x;
  const int halo = a.taps - 1;
  const int base = (int)blockIdx.x * kLimAnyTile;
  const int last = (int)a.n - 1;
  for (int i = tid; i < a.phases * a.taps; i += kLimAnyTile) hs[i] = a.table[i];
  float e = 0.0f;
  for (int ch = 0; ch < a.C; ch++) {
    const float *row = a.in + (size_t)ch * a.in_stride;
    const float *hist = a.xhist_in + (size_t)ch * a.HX + (a.HX - halo);
    __syncthreads();  // (the table; the readers of the channel before)
    for (int w = tid; w < kLimAnyTile + halo; w += kLimAnyTile) xs[w] = tp_sample(row, hist, halo, last, base - halo + w);
    __syncthreads();
    const float *at = xs + halo + tid;
    e = tp_absmax(e, at[-a.D]);
    for (int p = 0; p < a.phases; p++) e = tp_absmax(e, tp_dot(hs + p * a.taps, a.taps, [&](int k) { return at[-k]; }));
  }
  if (base + tid <= last) a.r[base + tid] = lim_required_gain(a.c, e);
}

__global__ __launch_bounds__(256) void k_lim_detect_sample(LimArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  float e = 0.0f;
  for (int ch = 0; ch < a.C; ch++) e = tp_absmax(e, a.in[(size_t)ch * a.in_stride + i]);
  a.r[i] = lim_required_gain(a.c, e);
}

__global__ __launch_bounds__(kLimThreads) void k_lim_apply(LimArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lim_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int W = kLimTile + a.HR;  // r of samples [t0 - HR, t0 + tile)
  float *rs = lim_lds, *ms = lim_lds + ((W + 3) & ~3);
  const int t0 = (int)blockIdx.x * kLimTile;
  const int last = (int)a.n - 1;

  // the histories for the next launch
  if (blockIdx.x == 0)
    for (int k = tid; k < a.HR; k += kLimThreads) {
      const int i = (int)a.n - a.HR + k;
      a.rhist_out[k] = i < 0 ? a.rhist_in[a.HR + i] : a.r[i];
    }
  for (int ch = (int)blockIdx.x; ch < a.C; ch += (int)gridDim.x)
    for (int k = tid; k < a.HX; k += kLimThreads) {
      const int i = (int)a.n - a.HX + k;
      a.xhist_out[(size_t)ch * a.HX + k] = i < 0 ? a.xhist_in[(size_t)ch * a.HX + a.HX + i] : a.in[(size_t)ch * a.in_stride + i];
    }

  for (int w = tid; w < W; w += kLimThreads) {
    const int i = t0 - a.HR + w;  // (a value beyond the launch's last sample is never consumed by a sample that is written)
    rs[w] = i < 0 ? a.rhist_in[a.HR + i] : a.r[min(i, last)];
  }
  __syncthreads();
  float rdel[kLimRun];  // r[n - L] of the thread's samples n = t0 + tid + 256 k
#pragma unroll
  for (int k = 0; k < kLimRun; k++) rdel[k] = rs[a.M - 1 + tid + kLimThreads * k];
  // sliding minimum, in place: after a round rs[w] is the minimum over the 2 s values up to w (for w >= 2 s - 1)
  const int per = (W + kLimThreads - 1) / kLimThreads;
  int P = 1;
  for (; 2 * P <= a.M; P *= 2) {
    float v[kLimPer];
#pragma unroll
    for (int k = 0; k < kLimPer; k++) {
      const int w = tid + kLimThreads * k;
      if (k < per && w < W && w >= P) v[k] = rs[w - P];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kLimPer; k++) {
      const int w = tid + kLimThreads * k;
      if (k < per && w < W && w >= P) rs[w] = fminf(rs[w], v[k]);
    }
    __syncthreads();
  }
  // m of samples [t0 - L, t0 + tile): sample t0 - L + j is window word M - 1 + j
  for (int j = tid; j < kLimTile + a.L; j += kLimThreads) ms[j] = fminf(rs[a.M - 1 + j], rs[P - 1 + j]);
  __syncthreads();
  float s[kLimRun];
  lim_sum(a.K, s, [&](int k, int q) { return ms[a.L + tid + kLimThreads * k - q]; });
  float *gs = rs;  // (every read of rs lies before the barrier above)
  unsigned worst = 0, count = 0;
#pragma unroll
  for (int k = 0; k < kLimRun; k++) {
    const int i = tid + kLimThreads * k;
    const float g = lim_gain(s[k], a.K, rdel[k]);
    gs[i] = g;
    if (t0 + i <= last) {
      if (a.gain) a.gain[t0 + i] = g;
      if (g < 1.0f) worst = max(worst, kLimOneBits - __float_as_uint(g)), count++;
    }
  }
  // (non-negative floats order like their bit patterns: the smallest g is the largest difference from the bits of 1)
  worst = __float_as_uint(tp_wave_max(__uint_as_float(worst)));
  for (int sh = 32; sh >= 1; sh >>= 1) count += (unsigned)__shfl_xor((int)count, sh, 64);
  if (lane == 0 && count) {
    const int slot = (int)(blockIdx.x % kLimSlots);
    atomicMax(&a.stat_min[slot], worst);
    atomicAdd(&a.stat_count[slot], (unsigned long long)count);
  }
  __syncthreads();
  for (int ch = 0; ch < a.C; ch++) {
    const float *__restrict__ row = a.in + (size_t)ch * a.in_stride;
    const float *__restrict__ hist = a.xhist_in + (size_t)ch * a.HX;
    float *__restrict__ o = a.out + (size_t)ch * a.out_stride;
    float x[kLimRun];
#pragma unroll
    for (int k = 0; k < kLimRun; k++) x[k] = tp_sample(row, hist, a.HX, last, t0 + tid + kLimThreads * k - a.D - a.L);
#pragma unroll
    for (int k = 0; k < kLimRun; k++) {
      const int i = tid + kLimThreads * k;
      if (t0 + i <= last) o[t0 + i] = x[k] * gs[i];
    }
  }
}

}  // namespace earhip
