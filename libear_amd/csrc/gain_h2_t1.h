// gain_h2_t1.h — the f16x2 grid kernel of gain_h2.h in its form with ONE tile per workgroup, kept for the 4-wave
// instantiations with two or three column tiles (256-sample tiles, 17-48 output columns): two such workgroups share a
// CU and cover each other's pipeline ends, and with the tile end inside the chunk loop (gain_h2.h: a workgroup working
// through several tiles) these instantiations no longer fit the register file (0.50 -> 0.55 ms on the headline scene at
// 256-sample tiles).  Same arithmetic, same operands, same results; see gain_h2.h for the method and for the per-chunk code
// (descriptors, gains, B fragments, the MFMA blocks), which both forms call; here: the prologue, the tile, the loop, the tail.
#pragma once

#include "gain_h2.h"

namespace earhip {

// Parameters, NW and the two forms as for k_gain_mix_h2 (gain_h2.h).  WIDE: the form that keeps the inputs' low pieces scaled
// (kLowPieceScale), as two instantiations launched back to back: the level probe decides on the device which one works
// (k_seg_prep sets *wide_cur) and the other returns at once (an empty grid: ~3 us).  Without a probe (wide_cur == NULL) only
// the wide form is launched.
template <int NCT, int NW, bool WIDE>
__global__ void __launch_bounds__(64 * NW, 2)
k_gain_mix_h2_t1(GainMixParams P, int zero_row, float x_scale, const float *__restrict__ gcol, const unsigned *level_cur,
              unsigned *level_next, const unsigned *slow_cur, unsigned *slow_next, const unsigned *wide_cur, unsigned *wide_next) {
  if (wide_cur && ((*wide_cur & 1u) != 0u) != WIDE) return;  // the other form of this kernel works on this call
  constexpr int NRT = 4, TS = 16 * NRT, CH = kSplitChunk;
  constexpr int NQ = CH / NW;         // objects whose gains one wave converts per chunk
  constexpr int NFRAG = 2 * NCT * 3;  // {B0,B1} x column tiles x {h, l, h 2^-11 (wide mode)}
  __shared__ u32x4 bfrag[2][NFRAG + 6][64];  // + 6 never-read fragments: the lanes without a column write there
  // the wave's output tile of one column tile, [16 columns][64 samples (+ 4: bank spread)], on its way from the
  // D fragments (a lane: one column, 16-byte pieces 64 bytes apart) to stores of whole 256-byte rows
  constexpr int OP = kSplitOutPitch;
  __shared__ __attribute__((aligned(16))) float otile[NW][16 * OP];
  __shared__ float inv_gcol[16 * NCT];  // 1 / the gain scale of the workgroup's columns: read at the END of a tile, where a
                                        // round trip to memory would stand in the open
  if (threadIdx.x < 16 * NCT) inv_gcol[threadIdx.x] = 1.0f / gcol[blockIdx.z * 16 * NCT + threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, kg = lane >> 4;
  const int wgtile = xcd_tile(blockIdx.x, gridDim.x);
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
    if (wide_next) *wide_next = 0u;
    record_mode(P, wide_cur != nullptr);
  }
  if (level_cur) {
    x_scale = probed_input_scale(level_cur, x_scale);
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) *level_next = 0;
  }
  // does any object of this tile need the exact path (a curve point inside the tile, a quiet object)?  K0:
  // k_seg_prep leaves a word per tile; this call clears the words of the call after next (they alternate).
  const bool any_slow = !slow_cur || slow_cur[wgtile] != 0u;
  if (slow_next && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) slow_next[wgtile] = 0u;
  const int nparts = gridDim.y;
  const int part = blockIdx.y;
  const int m_lo = (int)(((int64_t)P.M * part) / nparts);
  const int m_hi = (int)(((int64_t)P.M * (part + 1)) / nparts);
  const int col0 = blockIdx.z * 16 * NCT;
  const int tile_s0 = wgtile * (TS * NW) + w * TS;  // first sample of this wave's tile
  const int tile_len = max(0, min(TS, P.nsamples - tile_s0));
  const int64_t tile_t0 = P.t_call + tile_s0;
  const int64_t tile_t1 = tile_t0 + tile_len;
  const SegDesc *__restrict__ dtile = P.desc + (size_t)wgtile * P.M;
  const float *__restrict__ gain = P.ps.gain;
  const unsigned rowlen = (unsigned)P.ps.row;

  // running totals in scaled units: bus = (tot0 + (s - s0) tot1) / (x_scale g_scale)
  f32x4 tot0[NRT][NCT], tot1[NRT][NCT];
  auto clear_totals = [&]() {
#pragma unroll
    for (int r = 0; r < NRT; r++)
#pragma unroll
      for (int c = 0; c < NCT; c++) tot0[r][c] = tot1[r][c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  };
  clear_totals();

  // ---- slow path: one object, all its pieces inside this wave's tile, on the exact f32 MFMA, accumulated into tot0 in units of
  // 1 / (sx sg) (gain_h2.h, single_object: objects with a curve point inside the tile and quiet objects behind the chunk loop,
  // every object when the tile is redone or the rows are unaligned; khint: the segment index K0 found, or -1)
  auto single_object = [&](int m, float sx, bool sg, int khint = -1) {
    if (tile_len <= 0) return;
    float gsc[NCT];
#pragma unroll
    for (int c = 0; c < NCT; c++) gsc[c] = sg ? gcol[col0 + c * 16 + li] : 1.0f;
    const int base = P.ps.off[m], n = P.ps.cnt[m];
    const float *row = P.in + (size_t)m * P.in_stride + tile_s0;
    int k;
    if (khint >= 0) {
      k = min(khint, n);
      while (k < n && P.ps.time[base + k] <= tile_t0) k++;
    } else {
      k = upper_bound_time(P.ps.time + base, n, tile_t0);
    }
    exact_segments<NCT>(P.ps, base, n, k, row, tile_t0, tile_t1, tile_len, li, kg, gsc, sx, col0, tot0);
  };

  const int nobj = m_hi - m_lo;
  const int nch = (P.vec_ok && nobj >= CH) ? (nobj + CH - 1) / CH : 0;
  float inv_x = 1.0f / x_scale;  // exact: a power of two
  bool col_scaled = true;        // the totals are in units of 1 / (x_scale x the column's gain scale)

  if (nch > 0) {
    // lane-constant part of the input address: byte offset of this lane's float4 (lanes past the
    // end of the call re-read the last vector; never stored).  All loads below are (wave-uniform
    // 64-bit base) + (32-bit lane offset).  The last chunk is moved back to end at m_hi (its objects
    // that the previous chunk already covered get the zero row).
    const int nvec = (P.nsamples + 3) & ~3;
    const unsigned xs = (unsigned)min(tile_s0 + li * NRT, nvec - 4);
    const unsigned xlane = ((unsigned)(kg * 8) * (unsigned)P.in_stride + xs) * 4u;
    const unsigned bcol_e = (unsigned)(col0 + min(lane, 16 * NCT - 1));  // the lane's gain column
    const float g_scale = gcol[bcol_e];                                   // ... and that column's scale (a power of two)
    // fragment this lane fills: B0 pieces at bfr, bfr+1, B1 pieces NCT*2 further
    const int blane = (w * NQ / 8) * 16 + (lane & 15);
    const int bfr = lane < 16 * NCT ? (lane >> 4) * 3 : NFRAG;
    const int bfr1 = lane < 16 * NCT ? NCT * 3 : 3;
    auto chunk_base = [&](int c) { return min(m_lo + c * CH, m_hi - CH); };

    // inputs q0 .. q0 + n - 1 of chunk c.  Past the last chunk (the two-chunks-ahead requests of the
    // last two chunks: never used) every lane of every request reads the same 16 bytes instead of 64
    // lines per wave that would occupy the CU's miss slots for nothing (6 % of the input requests).
    auto load_x_part = [&](int c, f32x4 (&x)[8], int q0, int n) {
      const bool live = c < nch;
      const char *bp = reinterpret_cast<const char *>(P.in + (live ? (size_t)chunk_base(c) * P.in_stride : 0));
      const size_t rstride = live ? P.in_stride * sizeof(float) : 0;
      const unsigned xo = live ? xlane : 0u;
#pragma unroll
      for (int q = 0; q < 8; q++)
        if (q >= q0 && q < q0 + n)
          x[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(bp + (size_t)q * rstride + xo));
    };
    auto load_x = [&](int c, f32x4 (&x)[8]) { load_x_part(c, x, 0, 8); };
    // what this WAVE converts for chunk c: objects chunk_base + NQ w + q (past the last chunk: the last one's again)
    auto chunk_desc = [&](int c) { return load_desc<NQ>(dtile, chunk_base(min(c, nch - 1)) + w * NQ); };
    auto chunk_gains = [&](const ChunkDesc<NQ> &R, int c, ChunkCoef<NQ> &D, float (&S)[NQ], float (&E)[NQ]) {
      const int cc = min(c, nch - 1);
      load_gains<NQ, TS * NW>(R, chunk_base(cc) + w * NQ, m_lo + cc * CH, zero_row, gain, rowlen, bcol_e, D, S, E);
    };
    auto convert = [&](const ChunkCoef<NQ> &D, const float (&S)[NQ], const float (&E)[NQ], int buf, int part) {
      store_b<NQ, WIDE>(D, S, E, g_scale, &bfrag[buf][bfr][blane] + (part ? bfr1 * 64 : 0), w, part);
    };

    // Inputs are requested TWO chunks ahead (a chunk is about 1 us of work for the wave, less
    // than the memory latency under load) into the registers the operand split has just
    // freed; the chunk loop is unrolled twice so that the two register sets need no moves.
    // The vector-memory counter is in order (a wait for one load waits for every older one),
    // so per chunk the gain rows of the next chunk are requested BEFORE the inputs and
    // converted while those are in flight.
    f32x4 X0[8], X1[8];
    ChunkDesc<NQ> L;
    {
      float S[NQ], E[NQ];
      ChunkCoef<NQ> D;
      L = chunk_desc(0);
      chunk_gains(L, 0, D, S, E);
      load_x(0, X0);
      load_x(1, X1);
      convert(D, S, E, 0, 0);
      convert(D, S, E, 0, 1);
      L = chunk_desc(1);
    }
    // chunk c: inputs in xc, B fragments in bfrag[buf]
    auto chunk = [&](int c, int buf, f32x4 (&xc)[8]) {
      __syncthreads();  // B fragments of chunk c are in bfrag[buf]; bfrag[buf^1] is free
      float S[NQ], E[NQ];
      ChunkCoef<NQ> D;
      chunk_gains(L, c + 1, D, S, E);  // chunk c+1 (its descriptors were fetched one chunk ago)
      L = chunk_desc(c + 2);
      __builtin_amdgcn_sched_barrier(0);  // every gain row is requested before any input (see above)

      u32x4 ah[NRT], al[NRT];  // A fragments: the inputs' high and low pieces
      split_inputs<WIDE>(xc, x_scale, ah, al);
      __builtin_amdgcn_sched_barrier(0);  // the splitting above stays above
      chunk_mfmas<NCT, WIDE>(bfrag[buf], lane, ah, al, tot0, tot1,
                             [&](int q0, int n) __attribute__((always_inline)) { load_x_part(c + 2, xc, q0, n); },
                             [&](int part) __attribute__((always_inline)) { convert(D, S, E, buf ^ 1, part); });
    };
#pragma unroll 1
    for (int c = 0; c < nch; c += 2) {
      chunk(c, 0, X0);
      if (c + 1 < nch) chunk(c + 1, 1, X1);
    }

    // objects with curve points inside this workgroup tile (zero rows above)
    for (int b0 = 0; any_slow && b0 < nobj; b0 += 64) {
      const SegDesc db = dtile[min(m_lo + b0 + lane, m_hi - 1)];
      unsigned long long multi = __ballot((db.info & (kSegMulti | kSegQuiet)) && b0 + lane < nobj);
      while (multi) {
        const int j = __builtin_ctzll(multi);
        multi &= multi - 1;
        // (the k field of a descriptor is exact for these objects: the piece ends inside the tile)
        single_object(m_lo + b0 + j, x_scale, true, seg_k(__shfl(db.info, j)));
      }
    }
    // an input beyond the f16 range (or not finite) shows as non-finite totals: redo the
    // wave's tile exactly, unscaled
    if (__ballot(totals_not_finite<NCT>(tot0, tot1))) {
      clear_totals();
      inv_x = 1.0f;
      col_scaled = false;
      for (int m = m_lo; m < m_hi; m++) single_object(m, 1.0f, false);
    }
  } else {
    inv_x = 1.0f;
    col_scaled = false;
    for (int m = m_lo; m < m_hi; m++) single_object(m, 1.0f, false);  // unaligned rows
  }

  if (tile_len <= 0) return;
  // (s - c) of the lane's rows, samples 64w + 16kg + 4e + r: the line is anchored at the tile's centre
  const float wf0 = (float)(w * TS + kg * 16 - (TS * NW) / 2);
  float inv_gc[NCT];  // inverse gain scale of the lane's column in each column tile (the D fragments' layout)
#pragma unroll
  for (int c = 0; c < NCT; c++) inv_gc[c] = col_scaled ? inv_gcol[c * 16 + li] : 1.0f;
  float *op = P.out + (size_t)blockIdx.y * P.part_stride + tile_s0;
  write_tile<NCT>(tot0, tot1, wf0, inv_x, inv_gc, otile[w], op, P.out_stride, col0, P.ncols, li, kg, tile_len, P.vec_ok);
}

}  // namespace earhip
