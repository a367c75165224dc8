// delaymix_kernels.h — the device side of the delay matrix (include/earhip.h, group S; the maths: delaymix.h).
//
//   k_delaymix  a workgroup of 256 threads takes one tile of kDelaymixTile = 1024 outputs of one output row (blockIdx.y) and
//             loops over that row's routes in list order.  The tiles lie on the 16-byte grid of the OUTPUT row (a row whose
//             base is `ao` floats behind a 16-byte boundary has its tile t start at sample 1024 t - ao), so a thread's four
//             consecutive outputs are one 16-byte store wherever all four exist.  Per route the tile's input window — its
//             1024 samples and the T - 1 in front of them, D samples back in the input row — is brought into LDS with
//             16-byte loads on the 16-byte grid of the INPUT row (the window starts `a` = 0 .. 3 floats early; D is arbitrary,
//             so a differs from route to route), the part in front of the call from the history, one idle word after every 32
//             (delaymix_pad: lanes four words apart then fall on different banks).  The thread then runs the header's chain
//             for its four outputs with a sliding register window: T + 3 LDS reads for 4 T multiply-adds.  A route of ONE tap
//             shares no sample between neighbouring outputs and goes round the LDS and its barriers: the thread loads its four
//             samples as one 16-byte load at a float's alignment.  (What else was measured: NOTES.md.)
//   k_delaymix_history  behind it on the stream: the last H inputs of every row that is read into the OTHER history buffer
//             (src_history_entry), so a call shorter than H keeps the tail of the old history.
// No atomics, no scratch; nothing is read outside a row's n samples or written outside them; a row no route reads is not read.
#pragma once
#include <hip/hip_runtime.h>

#include "delaymix.h"

namespace earhip {

struct DelaymixArgs {
  const float *in;  // [n_in][in_stride], samples [0, n) of this launch
  size_t in_stride;
  float *out;  // [n_out][out_stride]
  size_t out_stride;
  int n, H;
  const DelaymixEntry *entries;
  const int *row_start;
  const float *taps;
  const float *hist_in;  // [n_in][H]: entry H + i is sample i < 0 of the launch
  float *hist_out;
  uint64_t reads;
};

// four floats at a float's alignment: one 16-byte load wherever they lie (global loads need no more than 4-byte alignment)
struct __attribute__((packed, aligned(4))) DelaymixQuad {
  float x[kDelaymixRun];
};

__global__ __launch_bounds__(kDelaymixThreads) void k_delaymix(DelaymixArgs a) {
  __shared__ __attribute__((aligned(16))) float win[kDelaymixLds];
  const int tid = threadIdx.x, k = blockIdx.y, n = a.n, H = a.H;
  float *__restrict__ o = a.out + (size_t)k * a.out_stride;
  const int ao = (int)(((uintptr_t)o >> 2) & 3);
  const int n0 = (int)blockIdx.x * kDelaymixTile - ao;  // the tile's first output; -3 .. -1: those do not exist
  if (n0 >= n) return;                                  // (uniform over the workgroup)
  const int len = min(kDelaymixTile, n - n0);
  float acc[kDelaymixRun];
#pragma unroll
  for (int i = 0; i < kDelaymixRun; i++) acc[i] = 0.0f;
  for (int e = a.row_start[k]; e < a.row_start[k + 1]; e++) {
    const DelaymixEntry q = a.entries[e];
    const int T = q.n_taps;
    const float *__restrict__ row = a.in + (size_t)q.in * a.in_stride;
    const float *__restrict__ hist = a.hist_in + (size_t)q.in * (size_t)H;
    const float *__restrict__ h = a.taps + q.tap_at;
    // sample i of the launch: history in front of it; nothing beyond either end (no output that is written reads there)
    auto sample = [&](int i) { return i < -H ? 0.0f : i < 0 ? hist[H + i] : i < n ? row[i] : 0.0f; };
    if (T == 1) {  // (uniform) no neighbour shares a sample: the thread's four, straight from the row
      const int i0 = n0 + 4 * tid - q.delay;
      DelaymixQuad v;
      if (i0 >= 0 && i0 + 3 < n) {
        v = *reinterpret_cast<const DelaymixQuad *>(row + i0);
      } else {
#pragma unroll
        for (int i = 0; i < kDelaymixRun; i++) v.x[i] = sample(i0 + i);
      }
      const float h0 = h[0];
#pragma unroll
      for (int i = 0; i < kDelaymixRun; i++) acc[i] = fmaf(h0, v.x[i], acc[i]);
      continue;
    }
    const int g0 = n0 - q.delay - (T - 1);  // the first sample the tile reads
    const int lead = (int)(((long)((uintptr_t)row >> 2) + g0) & 3);
    const int first = g0 - lead, words = lead + T - 1 + len;  // window word w is sample first + w; row + first is 16-byte aligned
    __syncthreads();                                          // the readers of the route before
    for (int w = 4 * tid; w < words; w += 4 * kDelaymixThreads) {
      const int i = first + w;
      float4 v;
      if (i >= 0 && i + 3 < n)
        v = *reinterpret_cast<const float4 *>(row + i);
      else
        v = make_float4(sample(i), sample(i + 1), sample(i + 2), sample(i + 3));
      win[delaymix_pad(w)] = v.x, win[delaymix_pad(w + 1)] = v.y, win[delaymix_pad(w + 2)] = v.z, win[delaymix_pad(w + 3)] = v.w;
    }
    __syncthreads();
    // output 4 tid + i, tap j reads word lead + (T - 1 - j) + 4 tid + i: x[i] holds it for the current j
    const int base = lead + 4 * tid;
    float x[kDelaymixRun];
#pragma unroll
    for (int i = 0; i < kDelaymixRun; i++) x[i] = win[delaymix_pad(base + T - 1 + i)];
    for (int j = 0; j < T; j++) {
      const float hj = h[j];
#pragma unroll
      for (int i = 0; i < kDelaymixRun; i++) acc[i] = fmaf(hj, x[i], acc[i]);
      if (j + 1 < T) {
#pragma unroll
        for (int i = kDelaymixRun - 1; i > 0; i--) x[i] = x[i - 1];
        x[0] = win[delaymix_pad(base + T - 2 - j)];
      }
    }
  }
  const int at = n0 + 4 * tid;
  if (at >= 0 && at + 3 < n) {
    *reinterpret_cast<float4 *>(o + at) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int i = 0; i < kDelaymixRun; i++)
      if (at + i >= 0 && at + i < n) o[at + i] = acc[i];
  }
}

__global__ __launch_bounds__(kDelaymixThreads) void k_delaymix_history(DelaymixArgs a) {
  const int c = blockIdx.y;
  if (!(a.reads >> c & 1)) return;
  const float *row = a.in + (size_t)c * a.in_stride;
  const float *old = a.hist_in + (size_t)c * (size_t)a.H;
  float *next = a.hist_out + (size_t)c * (size_t)a.H;
  const int k = (int)(blockIdx.x * kDelaymixThreads + threadIdx.x);
  if (k < a.H) next[k] = src_history_entry(a.H, (uint64_t)a.n, k, [&](int e) { return old[e]; }, [&](uint64_t i) { return row[i]; });
}

}  // namespace earhip
