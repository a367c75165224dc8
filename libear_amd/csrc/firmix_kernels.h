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

// ---- fade blocks (earhip_firmix_select with fade_blocks > 0) ----------------------------------------------------------------
//   k_firmix_fade  grid (fade blocks of the call, groups of two outputs): the blocks in which TWO filter sets are applied to
//                  the same ring of input spectra and blended, y = (1 - a) y_from + a y_to, a = firmix_fade_gain.  Per bin the
//                  merged ascending channel lists of both sets are walked once: each X[c][t - p] is read once and multiplied
//                  into the sums of up to four pairs, each in the steady kernel's order (inner sum over p from zero, added to
//                  the running sum over c).  Two inverse transforms, one after the other through the SAME two LDS buffers
//                  (at L = 8192 they take 128 KB of the 160): the target's sums wait in registers (4 floats per bin of the
//                  thread) and the first transform's output block does too (2 floats per sample), all indexed by unrolled
//                  loops so that nothing goes to scratch.
struct FirmixFadeArgs {
  const cf *X;                      // ring
  const cf *Ha, *Hb;                // the spectra slices of the set faded from / to
  const cf *tw;
  const FirmixEntry *ea, *eb;       // their lists
  const int *ga, *gb;               // their group_start
  float *out;
  size_t out_stride;
  int K, P, slot0, R;
  unsigned long long blocks_before;
  int q0, F;                        // fade block of the call's first block, blocks of the fade
};

template <int L>
__global__ void __launch_bounds__(kFirmixThreads) k_firmix_fade(FirmixFadeArgs A) {
  constexpr int B = L / 2, NT = kFirmixThreads, NJ = (B + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) cf lds[2 * L + (L <= 2048 ? L : 1)];
  cf *a = lds, *b = lds + L;
  const int tid = threadIdx.x;
  const int t = blockIdx.x, g = blockIdx.y;
  const int k0 = 2 * g, k1 = 2 * g + 1;
  float *out0 = A.out + (size_t)k0 * A.out_stride + (size_t)t * B;
  float *out1 = k1 < A.K ? A.out + (size_t)k1 * A.out_stride + (size_t)t * B : nullptr;
  const int a_begin = A.ga[g], a_end = A.ga[g + 1], b_begin = A.gb[g], b_end = A.gb[g + 1];
  if (a_begin == a_end && b_begin == b_end) {  // no pair in either set: +0.0
    for (int i = tid; i < B; i += NT) {
      out0[i] = 0.0f;
      if (out1) out1[i] = 0.0f;
    }
    return;
  }
  const cf *tw = firmix_twiddles<L>(lds + 2 * L, A.tw, tid);
  const int live = firmix_live_partitions(A.P, t, A.blocks_before);
  const int slot_t = firmix_ring_slot(A.slot0, t, 0, A.R);
  const size_t RB = (size_t)A.R * B, PB = (size_t)A.P * B;
  bool has_a0 = false, has_a1 = false, has_b0 = false, has_b1 = false;
  for (int e = a_begin; e < a_end; e++) {
    has_a0 = has_a0 || A.ea[e].h0 >= 0;
    has_a1 = has_a1 || A.ea[e].h1 >= 0;
  }
  for (int e = b_begin; e < b_end; e++) {
    has_b0 = has_b0 || A.eb[e].h0 >= 0;
    has_b1 = has_b1 || A.eb[e].h1 >= 0;
  }
  cf tb0[NJ], tb1[NJ];  // the target's sums, kept while the first inverse runs
#pragma unroll
  for (int u = 0; u < NJ; u++) {
    const int j = tid + u * NT;
    tb0[u] = tb1[u] = cf_make(0.0f, 0.0f);
    if (j >= B) continue;
    const bool packed = j == 0;
    cf sa0 = cf_make(0.0f, 0.0f), sa1 = sa0, sb0 = sa0, sb1 = sa0;
    int ia = a_begin, ib = b_begin;
    while (ia < a_end || ib < b_end) {
      const FirmixMerged m = firmix_merge_step(A.ea, ia, a_end, A.eb, ib, b_end);
      const cf *Xr = A.X + (size_t)m.row * RB + j;
      const cf *Ha0 = A.Ha + (size_t)(m.a0 >= 0 ? m.a0 : 0) * PB + j, *Ha1 = A.Ha + (size_t)(m.a1 >= 0 ? m.a1 : 0) * PB + j;
      const cf *Hb0 = A.Hb + (size_t)(m.b0 >= 0 ? m.b0 : 0) * PB + j, *Hb1 = A.Hb + (size_t)(m.b1 >= 0 ? m.b1 : 0) * PB + j;
      cf ca0 = cf_make(0.0f, 0.0f), ca1 = ca0, cb0 = ca0, cb1 = ca0;
      int slot = slot_t;
      for (int p = 0; p < live; p++) {
        const cf x = Xr[(size_t)slot * B];
        if (m.a0 >= 0) ca0 = firmix_mac(ca0, Ha0[(size_t)p * B], x, packed);
        if (m.a1 >= 0) ca1 = firmix_mac(ca1, Ha1[(size_t)p * B], x, packed);
        if (m.b0 >= 0) cb0 = firmix_mac(cb0, Hb0[(size_t)p * B], x, packed);
        if (m.b1 >= 0) cb1 = firmix_mac(cb1, Hb1[(size_t)p * B], x, packed);
        slot = slot == 0 ? A.R - 1 : slot - 1;
      }
      if (m.a0 >= 0) sa0 = cf_add(sa0, ca0);
      if (m.a1 >= 0) sa1 = cf_add(sa1, ca1);
      if (m.b0 >= 0) sb0 = cf_add(sb0, cb0);
      if (m.b1 >= 0) sb1 = cf_add(sb1, cb1);
    }
    tb0[u] = sb0, tb1[u] = sb1;
    if (packed) {
      a[0] = cf_make(sa0.x, sa1.x);
      a[B] = cf_make(sa0.y, sa1.y);
    } else {
      a[j] = cf_make(sa0.x - sa1.y, sa0.y + sa1.x);
      a[L - j] = cf_make(sa0.x + sa1.y, sa1.x - sa0.y);
    }
  }
  const float norm = 1.0f / (float)L;
  float ya0[NJ], ya1[NJ];  // the output block under the set faded from
  {
    const cf *y = fft_run_passes<L, +1, NT>(a, b, tw, 0, tid);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NJ; u++) {
      const int i = tid + u * NT;
      const cf v = i < B ? y[B + i] : cf_make(0.0f, 0.0f);
      ya0[u] = has_a0 ? v.x * norm : 0.0f;
      ya1[u] = has_a1 ? v.y * norm : 0.0f;
    }
    __syncthreads();  // the result is read before `a` is written again
  }
#pragma unroll
  for (int u = 0; u < NJ; u++) {
    const int j = tid + u * NT;
    if (j >= B) continue;
    const cf s0 = tb0[u], s1 = tb1[u];
    if (j == 0) {
      a[0] = cf_make(s0.x, s1.x);
      a[B] = cf_make(s0.y, s1.y);
    } else {
      a[j] = cf_make(s0.x - s1.y, s0.y + s1.x);
      a[L - j] = cf_make(s0.x + s1.y, s1.x - s0.y);
    }
  }
  const cf *y = fft_run_passes<L, +1, NT>(a, b, tw, 0, tid);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NJ; u++) {
    const int i = tid + u * NT;
    if (i >= B) continue;
    const cf v = y[B + i];
    const float w = firmix_fade_gain(A.q0 + t, i, A.F, B);
    // (1 - w) y_from + w y_to, each operation rounded on its own: what a caller's float32 code gives
    const float yb0 = has_b0 ? v.x * norm : 0.0f, yb1 = has_b1 ? v.y * norm : 0.0f;
    out0[i] = __fadd_rn(__fmul_rn(1.0f - w, ya0[u]), __fmul_rn(w, yb0));
    if (out1) out1[i] = __fadd_rn(__fmul_rn(1.0f - w, ya1[u]), __fmul_rn(w, yb1));
  }
}

}  // namespace earhip
