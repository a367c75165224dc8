// firmix_kernels.h — the two passes of the FIR filter matrix (include/earhip.h, group M; the plan: firmix.h).
//
//   k_firmix_spectra      grid (blocks, ring rows): the forward transform of ONE 2B window [x_{t-1} | x_t] of one input
//                         channel, taken once and kept in the channel's ring for the P - 1 blocks that follow.  The window is
//                         real, so bins 0 .. B - 1 are kept (bin B, real like bin 0, rides in bin 0's imaginary part): B
//                         complex numbers per window.  The same kernel makes the filters' spectra at create ([h_p | 0]).
//   k_firmix_mac_inverse  grid (blocks, groups of two outputs): sum over the group's input channels c (ascending) and the
//                         partitions p (ascending) of H[k][c][p] X[c][t - p], per bin, in registers: an inner sum over p, added
//                         to the running sum over c (the order is fixed: no atomics).  The two outputs' Hermitian sums go
//                         through ONE inverse transform as Y0 + i Y1; its second half (overlap-save) is the output block:
//                         real part output 2g, imaginary part output 2g + 1.  K / 2 inverses per block, not K C P.
//
// Every block is its own transform (no two-blocks-per-transform pairing as in K2: the pairing there depends on where a call
// starts), so a window's spectrum does not depend on how the stream is cut into calls.
// Transforms: fft_lds.h (Stockham passes in LDS), twiddles in LDS up to L = 2048 as in K2.
#pragma once

#include <hip/hip_runtime.h>

#include "fft_lds.h"
#include "firmix.h"

namespace earhip {

constexpr int kFirmixThreads = 256;

struct FirmixSpectraArgs {
  const float *in;      // rows [.][in_stride]
  size_t in_stride;
  const int *rows;      // [ring rows] input channel of each ring row (nullptr for the filters: row r is row r)
  const float *prev_in; // [ring rows][B] the block before the call
  float *prev_out;      // written by the workgroups of the call's last block
  cf *X;                // ring [ring rows][R][B], or the filters' spectra [pairs][P][B]
  const cf *tw;         // [L]
  int n;                // blocks of the call (partitions of a filter)
  int slot0, R;
};

struct FirmixMacArgs {
  const cf *X;          // ring
  const cf *H;          // [pairs][P][B]
  const cf *tw;
  const FirmixEntry *entries;
  const int *group_start;
  float *out;           // [K][out_stride]
  size_t out_stride;
  int K, P, slot0, R;
  unsigned long long blocks_before;
};

// acc += h x; bin 0 carries two real bins (0 and B), multiplied each by its own
__device__ __forceinline__ cf firmix_mac(cf acc, cf h, cf x, bool packed) {
  const float re = fmaf(h.x, x.x, fmaf(packed ? 0.0f : -h.y, x.y, acc.x));
  const float im = packed ? fmaf(h.y, x.y, acc.y) : fmaf(h.x, x.y, fmaf(h.y, x.x, acc.y));
  return cf_make(re, im);
}

template <int L>
__device__ __forceinline__ const cf *firmix_twiddles(cf *lds_tw, const cf *tw, int tid) {
  if (L > 2048) return tw;
  for (int i = tid; i < L; i += kFirmixThreads) lds_tw[i] = tw[i];
  return lds_tw;  // visible after the first barrier of the passes
}

template <int L, bool TAPS>
__global__ void __launch_bounds__(kFirmixThreads) k_firmix_spectra(FirmixSpectraArgs A) {
  constexpr int B = L / 2, NT = kFirmixThreads;
  __shared__ __attribute__((aligned(16))) cf lds[2 * L + (L <= 2048 ? L : 1)];
  cf *a = lds, *b = lds + L;
  const int tid = threadIdx.x;
  const int t = blockIdx.x, r = blockIdx.y;
  const cf *tw = firmix_twiddles<L>(lds + 2 * L, A.tw, tid);
  const float *lo, *hi;
  cf *dst;
  if (TAPS) {
    lo = A.in + (size_t)r * A.in_stride + (size_t)t * B;
    hi = nullptr;
    dst = A.X + ((size_t)r * (size_t)A.n + (size_t)t) * B;
  } else {
    const float *row = A.in + (size_t)A.rows[r] * A.in_stride;
    hi = row + (size_t)t * B;
    lo = t > 0 ? hi - B : A.prev_in + (size_t)r * B;
    dst = A.X + ((size_t)r * (size_t)A.R + (size_t)firmix_ring_slot(A.slot0, t, 0, A.R)) * B;
  }
  for (int i = tid; i < B; i += NT) {
    const float h = TAPS ? 0.0f : hi[i];
    a[i] = cf_make(lo[i], 0.0f);
    a[i + B] = cf_make(h, 0.0f);
    if (!TAPS && t == A.n - 1) A.prev_out[(size_t)r * B + i] = h;
  }
  const cf *z = fft_run_passes<L, -1, NT>(a, b, tw, 0, tid);
  __syncthreads();
  for (int i = tid; i < B; i += NT) dst[i] = i == 0 ? cf_make(z[0].x, z[B].x) : z[i];
}

template <int L>
__global__ void __launch_bounds__(kFirmixThreads) k_firmix_mac_inverse(FirmixMacArgs A) {
  constexpr int B = L / 2, NT = kFirmixThreads;
  __shared__ __attribute__((aligned(16))) cf lds[2 * L + (L <= 2048 ? L : 1)];
  cf *a = lds, *b = lds + L;
  const int tid = threadIdx.x;
  const int t = blockIdx.x, g = blockIdx.y;
  const int k0 = 2 * g, k1 = 2 * g + 1;
  float *out0 = A.out + (size_t)k0 * A.out_stride + (size_t)t * B;
  float *out1 = k1 < A.K ? A.out + (size_t)k1 * A.out_stride + (size_t)t * B : nullptr;
  const int e0 = A.group_start[g], e1 = A.group_start[g + 1];
  if (e0 == e1) {  // no pair: +0.0
    for (int i = tid; i < B; i += NT) {
      out0[i] = 0.0f;
      if (out1) out1[i] = 0.0f;
    }
    return;
  }
  const cf *tw = firmix_twiddles<L>(lds + 2 * L, A.tw, tid);
  const int live = firmix_live_partitions(A.P, t, A.blocks_before);
  const size_t RB = (size_t)A.R * B, PB = (size_t)A.P * B;
  bool has0 = false, has1 = false;  // an output without a pair is +0.0, not the rounding of the other's transform
  for (int e = e0; e < e1; e++) {
    has0 = has0 || A.entries[e].h0 >= 0;
    has1 = has1 || A.entries[e].h1 >= 0;
  }
  for (int j = tid; j < B; j += NT) {
    const bool packed = j == 0;
    cf s0 = cf_make(0.0f, 0.0f), s1 = s0;
    for (int e = e0; e < e1; e++) {
      const FirmixEntry ent = A.entries[e];
      const cf *Xr = A.X + (size_t)ent.row * RB + j;
      const cf *H0 = A.H + (size_t)(ent.h0 >= 0 ? ent.h0 : 0) * PB + j;
      const cf *H1 = A.H + (size_t)(ent.h1 >= 0 ? ent.h1 : 0) * PB + j;
      cf c0 = cf_make(0.0f, 0.0f), c1 = c0;
      int slot = firmix_ring_slot(A.slot0, t, 0, A.R);
      if (ent.h0 >= 0 && ent.h1 >= 0) {
#pragma unroll 4
        for (int p = 0; p < live; p++) {
          const cf x = Xr[(size_t)slot * B];
          c0 = firmix_mac(c0, H0[(size_t)p * B], x, packed);
          c1 = firmix_mac(c1, H1[(size_t)p * B], x, packed);
          slot = slot == 0 ? A.R - 1 : slot - 1;
        }
      } else {
        const cf *Hs = ent.h0 >= 0 ? H0 : H1;
        cf c = cf_make(0.0f, 0.0f);
#pragma unroll 4
        for (int p = 0; p < live; p++) {
          c = firmix_mac(c, Hs[(size_t)p * B], Xr[(size_t)slot * B], packed);
          slot = slot == 0 ? A.R - 1 : slot - 1;
        }
        if (ent.h0 >= 0) c0 = c;
        else c1 = c;
      }
      if (ent.h0 >= 0) s0 = cf_add(s0, c0);
      if (ent.h1 >= 0) s1 = cf_add(s1, c1);
    }
    // Y = Y0 + i Y1 with both Hermitian: Y[j] = s0 + i s1, Y[L - j] = conj(s0) + i conj(s1)
    if (packed) {
      a[0] = cf_make(s0.x, s1.x);
      a[B] = cf_make(s0.y, s1.y);
    } else {
      a[j] = cf_make(s0.x - s1.y, s0.y + s1.x);
      a[L - j] = cf_make(s0.x + s1.y, s1.x - s0.y);
    }
  }
  const cf *y = fft_run_passes<L, +1, NT>(a, b, tw, 0, tid);
  __syncthreads();
  const float norm = 1.0f / (float)L;
  for (int i = tid; i < B; i += NT) {
    const cf v = y[B + i];
    out0[i] = has0 ? v.x * norm : 0.0f;
    if (out1) out1[i] = has1 ? v.y * norm : 0.0f;
  }
}

}  // namespace earhip
