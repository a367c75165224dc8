// src_kernels.h — the device side of the polyphase sample-rate converter (include/earhip.h, group P; the maths: src.h).
//
//   k_src<TAB, WIN>  a workgroup of 256 threads takes `tiles_per_wg` consecutive tiles of kSrcTile = 1024 outputs of one channel
//             (blockIdx.y).  TAB: the table c[L][pitch] is copied into LDS once per workgroup (pitch odd, so the rows of
//             neighbouring lanes, M mod L rows apart, start on different banks whenever L is a multiple of 32 or the lanes'
//             phases do not wrap); otherwise the lanes read it through the caches.  WIN: a tile's input window — the
//             floor(((tile - 1) M + L - 1) / L) + T samples from i_first - (T - 1) on — is brought into LDS with coalesced
//             loads, the part in front of the call from the history, one idle word after every 32 (src_pad: at a step of two
//             inputs per output the lanes of a half-wave then fall on 32 different banks); otherwise (M / L beyond about 11) the
//             lanes read the rows directly.  A thread takes outputs tid, tid + 256, tid + 512, tid + 768 of the tile: four
//             independent fmaf chains in the header's order, and every store instruction of a wave is 64 consecutive floats.
//             Per multiply-add: two LDS reads of 4 bytes (the coefficient and the sample).  The other assignment — a lane keeps one
//             phase's T coefficients in registers over outputs j, j + L, .. — needs one, but T = 48 .. 96 registers of
//             coefficients, a tile of at least 64 L outputs (10,240 at 160 / 147: a 40 KB transpose buffer beside the window) and
//             a second pass through LDS before the store; it was not built.
//   k_src_history    behind it on the stream: the last T - 1 inputs of every channel into the OTHER history buffer
//             (src_history_entry), so a call shorter than T - 1 keeps the tail of the old history.
// No atomics, no scratch; nothing is read behind a row's n samples or written behind its n_out outputs.
#pragma once
#include <hip/hip_runtime.h>

#include "src.h"

namespace earhip {

struct SrcArgs {
  const float *in;  // [C][in_stride], samples [0, n) of this launch
  size_t in_stride;
  float *out;  // [C][out_stride], outputs [0, n_out) of this launch
  size_t out_stride;
  unsigned n, n_out;
  unsigned r0;  // the launch's lead (src.h)
  int L, M, T, H, pitch;
  int window_lds, table_lds, window;  // src_shape
  int tiles_per_wg;
  const float *table;    // [L][pitch]
  const float *hist_in;  // [C][H]: entry H + i is sample i < 0 of the launch
  float *hist_out;
};

template <bool TAB, bool WIN>
__global__ __launch_bounds__(kSrcThreads) void k_src(SrcArgs a) {
  extern __shared__ __attribute__((aligned(16))) float src_lds[];
  const int tid = threadIdx.x;
  const float *__restrict__ row = a.in + (size_t)blockIdx.y * a.in_stride;
  const float *__restrict__ hist = a.hist_in + (size_t)blockIdx.y * a.H;
  float *__restrict__ o = a.out + (size_t)blockIdx.y * a.out_stride;
  float *tab = src_lds, *win = src_lds + (TAB ? a.table_lds : 0);
  const int H = a.H, T = a.T;
  const long n = (long)a.n;
  // sample i of the launch: history in front of it, nothing behind it (no output that is written reads there)
  auto sample = [&](long i) { return i < 0 ? hist[H + i] : (i < n ? row[i] : 0.0f); };
  if (TAB)
    for (int i = tid; i < a.table_lds; i += kSrcThreads) tab[i] = a.table[i];
  const float *__restrict__ coeffs = TAB ? tab : a.table;
  for (int tt = 0; tt < a.tiles_per_wg; tt++) {
    const unsigned q0 = (blockIdx.x * (unsigned)a.tiles_per_wg + (unsigned)tt) * (unsigned)kSrcTile;
    if (q0 >= a.n_out) break;  // (uniform over the workgroup)
    uint64_t ib;
    int pb;
    src_index(a.r0, q0, a.L, a.M, &ib, &pb);
    const long first = (long)ib - (T - 1);  // the window's first sample
    if (WIN) {
      __syncthreads();  // the readers of the tile before
      for (int w = tid; w < a.window; w += kSrcThreads) win[src_pad(w)] = sample(first + w);
    }
    if (WIN || (TAB && tt == 0)) __syncthreads();
    const unsigned left = a.n_out - q0;  // >= 1
    int at[kSrcRun];                     // the thread's outputs: window word of x[i], and their coefficient rows
    const float *c[kSrcRun];
    float acc[kSrcRun];
#pragma unroll
    for (int r = 0; r < kSrcRun; r++) {
      const unsigned t = min((unsigned)(tid + kSrcThreads * r), left - 1);  // (a lane beyond the last output repeats it)
      const unsigned v = (unsigned)pb + t * (unsigned)a.M;                  // < 2^10 + 2^20
      at[r] = (int)(v / (unsigned)a.L) + (T - 1);
      c[r] = coeffs + (size_t)(v % (unsigned)a.L) * a.pitch;
      acc[r] = 0.0f;
    }
    for (int k = 0; k < T; k++) {
#pragma unroll
      for (int r = 0; r < kSrcRun; r++) {
        const float x = WIN ? win[src_pad(at[r] - k)] : sample(first + at[r] - k);
        acc[r] = fmaf(c[r][k], x, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kSrcRun; r++) {
      const unsigned t = (unsigned)(tid + kSrcThreads * r);
      if (t < left) o[(size_t)q0 + t] = acc[r];
    }
  }
}

__global__ __launch_bounds__(kSrcThreads) void k_src_history(SrcArgs a) {
  const float *row = a.in + (size_t)blockIdx.x * a.in_stride;
  const float *old = a.hist_in + (size_t)blockIdx.x * a.H;
  float *next = a.hist_out + (size_t)blockIdx.x * a.H;
  for (int k = (int)threadIdx.x; k < a.H; k += kSrcThreads)
    next[k] = src_history_entry(a.H, a.n, k, [&](int e) { return old[e]; }, [&](uint64_t i) { return row[i]; });
}

}  // namespace earhip
