// gain_split.h — what the split-operand ("f16x2") gain kernels have in common: the grid kernel (gain_h2.h, gain_h2_t1.h),
// the piece-list kernel (gain_p2.h: the helpers only, it keeps its own copies of the blocks) and the hinge kernel (gain_hg.h).
// The method is described at the top of gain_h2.h.
//   * the f16 helpers of the operand split and the tile constants;
//   * probed_input_scale: the input scale of a call from the level K0 probed;
//   * split_inputs: a chunk's inputs as f16 high / low pieces (the A fragments);
//   * exact_segments: one object inside a wave's 64 samples on the exact f32 MFMA;
//   * totals_not_finite: the test that sends a wave's tile to the exact redo;
//   * write_tile: a wave's totals, scaled, transposed through LDS, to whole 256-byte rows of the output.
// All of them are inlined into kernels that are hand-scheduled and sit at the register limit: they take what they need as
// arguments and keep no state (NOTES.md, "The gain kernels' shared blocks", has the per-kernel register counts).
#pragma once

#include <hip/hip_runtime.h>

#include "gain_kernels.h"
#include "gain_mfma.h"

namespace earhip {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kSplitTile = 256;   // samples per workgroup tile of the 4-wave kernel (descriptor tile)
constexpr int kSplitChunk = 32;   // objects per MFMA (k)
constexpr int kSplitRowTiles = 4; // row tiles of a wave: sample 4 i + r of its 64 is row i of row tile r
constexpr int kSplitOutPitch = 16 * kSplitRowTiles + 4;  // floats between two columns of a wave's output tile in LDS (+ 4: bank spread)

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

// two floats -> packed f16 pair, round to nearest even (v_cvt_pk_f16_f32)
__device__ __forceinline__ uint32_t pack_f16(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_t));
}
// v - (the low / high half of u as a float): the exact residual of a split in ONE instruction (v_fma_mix_f32 converts its
// f16 operand on the way in; the conversion alone, v_cvt_f32_f16, issues at the same 4.3 cycles, and the subtraction came on
// top — profiles/r05_valu_issue_rates.txt)
// (written out: the compiler turns fma(half, -1, v) back into a conversion and a subtraction)
__device__ __forceinline__ float sub_f16_lo(float v, uint32_t u) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(u), "v"(v));
  return r;
}
__device__ __forceinline__ float sub_f16_hi(float v, uint32_t u) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(u), "v"(v));
  return r;
}

// Wide mode: the low piece of an input is kept as (residual x 2^11) and multiplied with (h x 2^-11) of the gain —
// both exact scalings, the same product — so that it is a normal f16 over 21 binades below the level the prescale
// aims at instead of 11 (measured relative RMS of the products: 6.5e-8 down to 2^-18, 1.4e-7 at 2^-20, 5e-7 at
// 2^-22; with the plain residual 2.5e-7 at 2^-10 and 1e-6 at 2^-12).
constexpr float kLowPieceScale = 2048.0f;
__device__ __forceinline__ uint32_t scale_f16x2_down(uint32_t h) {  // both halves x 2^-11 (exact unless subnormal)
  const f16x2_t k = {(_Float16)0.00048828125f, (_Float16)0.00048828125f};
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2_t, h) * k);
}

__device__ __forceinline__ f32x4 mfma_f16(const u32x4 &a, const u32x4 &b, const f32x4 &c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c,
                                                0, 0, 0);
}

// Input scale of THIS call from the level K0 probed (*level_cur: the bits of the largest magnitude seen): that magnitude,
// in [2^E, 2^(E+1)), goes to [2^7, 2^8) — peaks up to 256x the probed maximum stay inside the f16 range (beyond: the exact
// redo), and samples down to 2^-11 of it keep a normal low piece (2^-22 relative; below that 2^-33 of the maximum,
// absolute).  Nothing seen (silence): the launch's x_scale; absurd or non-finite levels: clamped.
__device__ __forceinline__ float probed_input_scale(const unsigned *level_cur, float x_scale) {
  const unsigned lv = *level_cur;
  if (lv) {
    const int E = max(-60, min(20, (int)(lv >> 23) - 127));
    x_scale = __uint_as_float((unsigned)(127 + 7 - E) << 23);
  }
  return x_scale;
}

// A fragments of a chunk: row tile r = sample 4*li + r of the 8 objects of this lane (xc[q]: the lane's four samples of
// object q).  2 x 2 blocks: an f16 pair packs two OBJECTS (q, q+1) of one row tile, the scaling and the exact residual
// subtractions pair two SAMPLES (r, r+1) of one object (neighbours in the loaded float4: packed arithmetic without operand
// moves).  WIDE: the residuals are scaled by 2^11 before they are rounded to f16 (kLowPieceScale).
template <bool WIDE>
__device__ __forceinline__ void split_inputs(const f32x4 (&xc)[8], float x_scale, u32x4 (&ah)[kSplitRowTiles],
                                             u32x4 (&al)[kSplitRowTiles]) {
#pragma unroll
  for (int qp = 0; qp < 4; qp++)
#pragma unroll
    for (int rp = 0; rp < kSplitRowTiles; rp += 2) {
      const f32x2 s0 = f32x2{xc[2 * qp][rp], xc[2 * qp][rp + 1]} * x_scale;          // object 2qp
      const f32x2 s1 = f32x2{xc[2 * qp + 1][rp], xc[2 * qp + 1][rp + 1]} * x_scale;  // object 2qp+1
      const uint32_t H0 = pack_f16(s0[0], s1[0]), H1 = pack_f16(s0[1], s1[1]);
      constexpr float LOW = WIDE ? kLowPieceScale : 1.0f;
      const f32x2 r0 = f32x2{sub_f16_lo(s0[0], H0), sub_f16_lo(s0[1], H1)} * LOW;  // residuals (exact)
      const f32x2 r1 = f32x2{sub_f16_hi(s1[0], H0), sub_f16_hi(s1[1], H1)} * LOW;
      ah[rp][qp] = H0;
      ah[rp + 1][qp] = H1;
      al[rp][qp] = pack_f16(r0[0], r1[0]);
      al[rp + 1][qp] = pack_f16(r0[1], r1[1]);
    }
}

// The exact path: ONE object (points base .. base + n - 1 of the curve store, k = the segment the tile starts in), all its
// pieces inside a wave's tile [tile_t0, tile_t1) of tile_len samples, on the f32 MFMA with k = {a, b} of that object (k
// slots 2, 3 idle: same arithmetic as gain_mfma.h), accumulated into tot in units of 1 / (sx gsc).  The two scales are
// applied to the two operands (their product may not be a float): sx to the inputs (row: the object's input at the tile's
// first sample), gsc[c] to the gains of the lane's column (li) in column tile c.
template <int NCT>
__device__ __forceinline__ void exact_segments(const PointStore &ps, int base, int n, int k, const float *row, int64_t tile_t0,
                                               int64_t tile_t1, int tile_len, int li, int kg, const float (&gsc)[NCT], float sx,
                                               int col0, f32x4 (&tot)[kSplitRowTiles][NCT]) {
  constexpr int NRT = kSplitRowTiles;
  const float *__restrict__ gain = ps.gain;
  const unsigned rowlen = (unsigned)ps.row;
  const bool is_b = kg & 1;
  const bool slot0 = kg < 2;
  int cur = 0;
  while (cur < tile_len) {
    const SegDesc dk = describe_segment(ps, base, n, k, tile_t0, tile_t1);
    const int r1 = min(seg_r1(dk.info), tile_len);
    if (r1 > cur) {  // duplicate times make empty segments (steps)
      const bool ramp = dk.info & kSegRamp;
      float a[NRT], gv[NCT];
#pragma unroll
      for (int r = 0; r < NRT; r++) {
        const int s = li * NRT + r;
        const float x = row[min(s, tile_len - 1)];
        const float p = (float)(dk.d0 + s) * dk.scale;  // gain_interpolator.hpp:272
        float coef = ramp ? (is_b ? p : 1.0f - p) : (is_b ? 0.0f : 1.0f);
        coef = (slot0 && s >= cur && s < r1) ? coef : 0.0f;
        a[r] = (x * coef) * sx;
      }
      const int grow = dk.row + ((ramp && is_b && slot0) ? 1 : 0);
      const float *gp = gain + (size_t)grow * rowlen + col0 + li;
#pragma unroll
      for (int c = 0; c < NCT; c++) gv[c] = gp[c * 16] * gsc[c];
#pragma unroll
      for (int r = 0; r < NRT; r++)
#pragma unroll
        for (int c = 0; c < NCT; c++)
          tot[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], gv[c], tot[r][c], 0, 0, 0);
      cur = r1;
    }
    if (!(dk.info & kSegMulti)) break;
    k++;
  }
}

// An operand beyond the f16 range (or not finite) shows as non-finite totals: does this LANE hold one, in either set?  (the wave then
// redoes its tile exactly, unscaled: __ballot of this)
// (| between the two arrays' tests, not ||: as a function the short-circuit form kept a lane mask per element alive — up to
// 250 more spilled SGPRs in k_gain_mix_h2<3,8,2> and k_gain_mix_hg<3,8>, scratch in k_gain_mix_hg<2,*>; the same value)
template <int NCT>
__device__ __forceinline__ bool totals_not_finite(const f32x4 (&tot0)[kSplitRowTiles][NCT], const f32x4 (&tot1)[kSplitRowTiles][NCT]) {
  bool bad = false;
#pragma unroll
  for (int r = 0; r < kSplitRowTiles; r++)
#pragma unroll
    for (int c = 0; c < NCT; c++)
#pragma unroll
      for (int e = 0; e < 4; e++) bad |= !(__builtin_fabsf(tot0[r][c][e]) < INFINITY) | !(__builtin_fabsf(tot1[r][c][e]) < INFINITY);
  return bad;
}

// A wave's tile is done: scale its totals and store them.  bus = tot0 + (s - c) tot1 with (s - c) = wf0 + 4 e + r for the
// lane's rows (wf0: the lane's first row against the point the line is anchored at).
// inv_x: the inverse of the input scale the totals carry (exact: a power of two); inv_gc[c]: the inverse gain scale of the
// lane's column (li) in column tile c (the D fragments' layout: a lane holds column li, rows 4 kg + e = samples 16 kg + 4 e
// + r of row tile r — for fixed e the four row tiles are 4 consecutive samples).  op: the wave's first sample in output row
// 0; ot: 16 x kSplitOutPitch floats of LDS that are the wave's own.
// Whole tiles of aligned rows go through that LDS: written straight from the fragments, one store instruction covers 4
// columns x 64 bytes in 16-byte pieces (64 scattered pieces per instruction: the stores of the 100 MB of buses cost a tenth
// of the grid kernel's time, a quarter at 256 objects); transposed, it covers 4 whole 256-byte rows.  The rows are written
// past the caches (K2 reads them once, much later: headline K1 0.437 -> 0.412 ms).
template <int NCT>
__device__ __forceinline__ void write_tile(const f32x4 (&tot0)[kSplitRowTiles][NCT], const f32x4 (&tot1)[kSplitRowTiles][NCT],
                                           float wf0, float inv_x, const float (&inv_gc)[NCT], float *ot, float *op,
                                           size_t out_stride, int col0, int ncols, int li, int kg, int tile_len, bool vec_ok) {
  constexpr int NRT = kSplitRowTiles, TS = 16 * NRT, OP = kSplitOutPitch;
  auto value = [&](int r, int c, int e) {
    return (__builtin_fmaf(wf0 + (float)(4 * e + r), tot1[r][c][e], tot0[r][c][e]) * inv_x) * inv_gc[c];
  };
  const bool whole = vec_ok && tile_len == TS;  // (wave-uniform)
#pragma unroll
  for (int c = 0; c < NCT; c++) {
    if (whole) {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < NRT; r++) v[r] = value(r, c, e);
        *reinterpret_cast<f32x4 *>(ot + li * OP + kg * 16 + e * 4) = v;
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {  // lane: column 4 j + (lane >> 4), samples 4 (lane & 15) .. + 3
        const int cl = 4 * j + kg, col = col0 + c * 16 + cl;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(ot + cl * OP + li * 4);
        if (col < ncols) __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(op + (size_t)col * out_stride + li * 4));
      }
      continue;
    }
    const int col = col0 + c * 16 + li;
    if (col >= ncols) continue;
    float *o = op + (size_t)col * out_stride;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int s = kg * 16 + e * 4;
      f32x4 v;
#pragma unroll
      for (int r = 0; r < NRT; r++) v[r] = value(r, c, e);
      if (vec_ok && s + 3 < tile_len) {
        *reinterpret_cast<f32x4 *>(o + s) = v;
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (s + i < tile_len) o[s + i] = v[i];
      }
    }
  }
}

}  // namespace earhip
