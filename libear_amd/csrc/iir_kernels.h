// iir_kernels.h — the device side of the biquad filter matrix (include/earhip.h, group O; the maths: iir.h).
//
// The technique is the loudness meter's (loudness_kernels.h): the time axis of a launch is cut, per route, into chunks of
// Lc = kIirChunk samples on the stage's own clock grid, and a lane walks one (route, chunk); a wave takes 64 consecutive chunks
// of one route.
//   k_iir_pass1      every (route, chunk) but the launch's last: chunk 0 from the CARRIED state (so its end state is the true
//                    one and no power of Phi for a partial length is ever needed), the others from zero      e [R][cap][16]
//   k_iir_propagate  per route, the true start state of every chunk                                        start [R][cap][16]
//                    A wave scans 64 whole chunks (Hillis-Steele with Phi^(Lc 2^d), d = 0 .. 5), the 4 waves of the workgroup
//                    take the groups side by side, one thread chains the group sums with Phi^(64 Lc), and every lane adds its
//                    group's carry-in times Phi^(Lc (lane + 1)), applied as the product of the Phi^(Lc 2^d) of the set bits
//                    of lane + 1: 7 matrices per route instead of 65.  The matrices are block lower-triangular and used so
//   k_iir_pass2<W>   a workgroup per (output, 64 chunks), W waves: every chunk again from its true start state, the waves taking
//                    the output's routes side by side, W at a time.  Per tile of kIirTile2 samples every wave lays its route's z
//                    down in LDS as doubles; then all threads add  acc = fma(gain_r, z_r, acc)  in ascending list index — the
//                    header's order whatever W is — and after the output's last route the tile leaves as float32 in runs of
//                    consecutive samples.  The lane of the launch's last chunk leaves the state the next launch starts from
//                    in the OTHER of the two state buffers.  With more routes than waves a route's state waits in e[] between
//                    tiles.  An output without a route is written as +0.0 by the same path.
// Rows are read through LDS as the meter reads them: unconditional loads with indices clamped into the launch, a tile ahead.
// Fixed orders everywhere, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "iir.h"

namespace earhip {

constexpr int kIirTile = 32;               // pass 1: samples of a chunk per LDS tile, as the meter
constexpr int kIirPitch = kIirTile + 1;    // odd
constexpr int kIirTile2 = 16;              // pass 2 (its tiles also hold doubles: 12.7 KiB of LDS a wave instead of 25)
constexpr int kIirPitch2 = kIirTile2 + 1;  // odd
constexpr int kIirZPitch = 66;             // doubles between the samples of a z tile: the adders' reads hit 32 different bank pairs

struct IirRouteDev {
  int in, out, S, pad;
  double gain;
  IirCoeffs<double> k;
};

struct IirArgs {
  const float *in;  // [n_in][in_stride], samples [0, n) of this launch
  size_t in_stride;
  float *out;  // [n_out][out_stride]
  size_t out_stride;
  unsigned n, off0, nchunks;  // iir.h: IirPlan
  unsigned cap;               // chunks of e and start per route: nchunks <= cap <= kIirMaxChunks
  const IirRouteDev *routes;  // [R]
  const double *Q;            // [R][kIirPowers][kIirMat]
  double *e;                  // [R][cap][16]
  double *start;              // [R][cap][16]
  const double *state_in;     // [R][16]
  double *state_out;          // [R][16]
  const int *out_first;       // [n_out + 1]: the routes of output o are out_routes[out_first[o] .. out_first[o + 1])
  const int *out_routes;      // [R] in ascending list index per output
};

__device__ inline IirState<double> iir_load_state(const double *p, int n2, bool live) {
  IirState<double> s;
#pragma unroll
  for (int i = 0; i < kIirMaxState; i++) s.s[i] = (live && i < n2) ? p[i] : 0.0;
  return s;
}
__device__ inline void iir_store_state(double *p, int n2, const IirState<double> &s) {
#pragma unroll
  for (int i = 0; i < kIirMaxState; i++)
    if (i < n2) p[i] = s.s[i];
}

__global__ __launch_bounds__(64) void k_iir_pass1(IirArgs a) {
  __shared__ float tile[64 * kIirPitch];
  const int lane = threadIdx.x;
  const int r = blockIdx.y;
  const IirRouteDev &rt = a.routes[r];
  const int S = rt.S, n2 = 2 * S;
  if (S == 0) return;  // (a gain route has no state)
  const unsigned c0 = blockIdx.x * 64u, c = c0 + lane;
  const bool live = c + 1 < a.nchunks;
  // sample j of chunk c (j in [0, Lc)) is sample c * Lc - off0 + j of the launch; this lane's chunk holds j in [jlo, jhi)
  int jlo = 0, jhi = 0;
  if (live) {
    const int b0 = (int)c * kIirChunk - (int)a.off0;
    jlo = max(-b0, 0);
    jhi = min(kIirChunk, (int)a.n - b0);
  }
  const float *row = a.in + (size_t)rt.in * a.in_stride;
  const IirCoeffs<double> k = rt.k;
  IirState<double> st = iir_load_state(a.state_in + (size_t)r * kIirMaxState, n2, c == 0);

  // the wave's fetch of one tile, as k_loudness_pass: load i of the 32 takes chunks (2 i, 2 i + 1) of the 64, lane l sample
  // l % 32 of the tile; unconditional, the index clamped into [0, n): what lies outside a lane's [jlo, jhi) is never consumed
  const int fs = lane & 31, fh = lane >> 5;
  const int pbase = (int)(c0 + fh) * kIirChunk - (int)a.off0 + fs;
  const int plast = (int)a.n - 1;
  float pre[kIirTile];
  auto fetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < kIirTile; i++) {
      const int p = pbase + t * kIirTile + 2 * i * kIirChunk;
      pre[i] = row[min(max(p, 0), plast)];
    }
  };
  constexpr int ntiles = kIirChunk / kIirTile;
  fetch(0);
  for (int t = 0; t < ntiles; t++) {
    __syncthreads();  // (the tile before this one has been read)
#pragma unroll
    for (int i = 0; i < kIirTile; i++) tile[(2 * i + fh) * kIirPitch + fs] = pre[i];
    __syncthreads();
    if (t + 1 < ntiles) fetch(t + 1);  // in flight while this tile is filtered
    const int j0 = t * kIirTile;
    const float *mine = tile + lane * kIirPitch;
    if (j0 >= jlo && j0 + kIirTile <= jhi) {
#pragma unroll
      for (int s = 0; s < kIirTile; s++) (void)iir_step(k, S, st, (double)mine[s]);
    } else {
      for (int s = max(jlo - j0, 0); s < kIirTile && j0 + s < jhi; s++) (void)iir_step(k, S, st, (double)mine[s]);
    }
  }
  if (live) iir_store_state(a.e + ((size_t)r * a.cap + c) * kIirMaxState, n2, st);
}

// launched when the launch has two chunks or more
__global__ __launch_bounds__(64 * kIirScanWaves) void k_iir_propagate(IirArgs a) {
  __shared__ double Qs[kIirPowers * kIirMat];
  __shared__ double gsum[kIirScanGroups][kIirMaxState];   // c of the last lane of every group
  __shared__ double carry[kIirScanGroups][kIirMaxState];  // the state that enters every group
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n2 = 2 * a.routes[r].S;
  if (n2 == 0) return;
  const size_t base = (size_t)r * a.cap * kIirMaxState;
  const double *E = a.e + base;
  double *St = a.start + base;
  const unsigned m = a.nchunks - 2;  // the whole chunks in the middle: chunk 1 + i
  const unsigned groups = (m + 63) / 64;
  for (int i = tid; i < kIirPowers * kIirMat; i += 64 * kIirScanWaves) Qs[i] = a.Q[(size_t)r * kIirPowers * kIirMat + i];
  if (tid < n2) St[kIirMaxState + tid] = E[tid];  // chunk 1 starts where chunk 0 ended: pass 1 ran chunk 0 from the true state
  __syncthreads();
#pragma unroll 1
  for (int rr = 0; rr < kIirGroupsPerWave; rr++) {
    const unsigned g = (unsigned)wave + (unsigned)rr * kIirScanWaves;
    if (g >= groups) continue;  // (uniform over the wave)
    const unsigned i = g * 64 + lane;
    IirState<double> c = iir_load_state(E + (size_t)(1 + i) * kIirMaxState, n2, i < m);
    // inclusive scan: c_i = sum over j <= i of Phi^(Lc (i - j)) e_j
#pragma unroll 1
    for (int d = 0; d < 6; d++) {
      IirState<double> up;
#pragma unroll
      for (int q = 0; q < kIirMaxState; q++) up.s[q] = __shfl_up(c.s[q], 1u << d, 64);
      if (lane >= (1 << d)) c = iir_advance(Qs + d * kIirMat, n2, up, c);
    }
    if (i < m) iir_store_state(St + (size_t)(2 + i) * kIirMaxState, n2, c);  // (finished below)
    if (lane == 63) {
#pragma unroll
      for (int q = 0; q < kIirMaxState; q++) gsum[g][q] = c.s[q];
    }
  }
  __syncthreads();
  if (tid == 0) {
    IirState<double> cr = iir_load_state(E, n2, true);
    for (unsigned g = 0; g < groups; g++) {
      IirState<double> gs;
#pragma unroll
      for (int q = 0; q < kIirMaxState; q++) carry[g][q] = cr.s[q], gs.s[q] = gsum[g][q];
      cr = iir_advance(Qs + 6 * kIirMat, n2, cr, gs);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int rr = 0; rr < kIirGroupsPerWave; rr++) {
    const unsigned g = (unsigned)wave + (unsigned)rr * kIirScanWaves;
    if (g >= groups) continue;
    const unsigned i = g * 64 + lane;
    if (i >= m) continue;
    IirState<double> v;
#pragma unroll
    for (int q = 0; q < kIirMaxState; q++) v.s[q] = carry[g][q];
    const IirState<double> zero = iir_zero_state();
#pragma unroll 1
    for (int d = 0; d < kIirPowers; d++)
      if (((lane + 1) >> d) & 1) v = iir_advance(Qs + d * kIirMat, n2, v, zero);
    double *p = St + (size_t)(2 + i) * kIirMaxState;
    const IirState<double> c = iir_load_state(p, n2, true);
#pragma unroll
    for (int q = 0; q < kIirMaxState; q++) v.s[q] = v.s[q] + c.s[q];
    iir_store_state(p, n2, v);
  }
}

template <int W>
__global__ __launch_bounds__(64 * W) void k_iir_pass2(IirArgs a) {
  constexpr int T = kIirTile2, P = kIirPitch2, ZP = kIirZPitch;
  constexpr int kPer = T / W;  // samples of the tile's 64 x T an adder thread takes
  __shared__ float tile[W][64 * P];
  __shared__ double zt[W][T * ZP];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int o = blockIdx.y;
  const unsigned c0 = blockIdx.x * 64u, c = c0 + lane;
  const int first = a.out_first[o], nr = a.out_first[o + 1] - first;
  const int nb = (nr + W - 1) / W;  // rounds of W routes
  const bool livec = c < a.nchunks;
  int jlo = 0, jhi = 0;
  if (livec) {
    const int b0 = (int)c * kIirChunk - (int)a.off0;
    jlo = max(-b0, 0);
    jhi = min(kIirChunk, (int)a.n - b0);
  }
  const int plast = (int)a.n - 1;
  // the fetch of a tile: load i of the 16 takes chunks 4 i .. 4 i + 3 of the 64, lane l sample l % 16: four runs of 64 bytes
  const int fs = lane & 15, fh = lane >> 4;
  const int pbase = (int)(c0 + fh) * kIirChunk - (int)a.off0 + fs;
  constexpr int ntiles = kIirChunk / T;
  const int iters = ntiles * nb;
  // the route this wave takes in round b (uniform over the wave), -1: none
  auto route_of = [&](int b) {
    const int qi = b * W + wave;
    return qi < nr ? a.out_routes[first + qi] : -1;
  };
  float pre[T];
  auto fetch = [&](int it) {
    const int t = it / nb, r = route_of(it - t * nb);
    const float *row = a.in + (size_t)(r >= 0 ? a.routes[r].in : 0) * a.in_stride;
#pragma unroll
    for (int i = 0; i < T; i++) {
      const int p = pbase + t * T + 4 * i * kIirChunk;
      pre[i] = row[min(max(p, 0), plast)];
    }
  };
  IirState<double> st = iir_zero_state();
  IirCoeffs<double> k;
  int S = 0;
  if (iters > 0) fetch(0);
  for (int t = 0; t < ntiles; t++) {
    double acc[kPer];
#pragma unroll
    for (int i = 0; i < kPer; i++) acc[i] = 0.0;
    for (int b = 0; b < nb; b++) {
      const int it = t * nb + b;
      const int r = route_of(b);
#pragma unroll
      for (int i = 0; i < T; i++) tile[wave][(4 * i + fh) * P + fs] = pre[i];
      __syncthreads();  // (and every z tile of the round before has been added)
      if (it + 1 < iters) fetch(it + 1);  // in flight while this tile is filtered
      if (r >= 0) {
        const IirRouteDev &rt = a.routes[r];
        const size_t slot = ((size_t)r * a.cap + c) * kIirMaxState;
        if (nb > 1 || t == 0) {
          S = rt.S;
          k = rt.k;
          // the launch's first chunk starts from the carried state, the others from the propagated ones; later tiles of a
          // route that shares its wave continue from where they were left
          const double *from = t > 0 ? a.e + slot : (c == 0 ? a.state_in + (size_t)r * kIirMaxState : a.start + slot);
          st = iir_load_state(from, 2 * S, livec);
        }
        const int j0 = t * T;
        const float *mine = tile[wave] + lane * P;
        double *z = zt[wave] + lane;
        if (j0 >= jlo && j0 + T <= jhi) {
#pragma unroll
          for (int s = 0; s < T; s++) z[s * ZP] = iir_step(k, S, st, (double)mine[s]);
        } else {
#pragma unroll
          for (int s = 0; s < T; s++) {
            const bool in = j0 + s >= jlo && j0 + s < jhi;
            double y = 0.0;
            if (in) y = iir_step(k, S, st, (double)mine[s]);
            z[s * ZP] = y;
          }
        }
        if (livec) {
          if (nb > 1 && t + 1 < ntiles) iir_store_state(a.e + slot, 2 * S, st);
          if (t + 1 == ntiles && c + 1 == a.nchunks) iir_store_state(a.state_out + (size_t)r * kIirMaxState, 2 * S, st);
        }
      }
      __syncthreads();
      // the header's sum: ascending list index, one fused multiply-add per route
#pragma unroll
      for (int w = 0; w < W; w++) {
        const int qi = b * W + w;
        if (qi < nr) {
          const double gain = a.routes[a.out_routes[first + qi]].gain;
#pragma unroll
          for (int i = 0; i < kPer; i++) {
            const int idx = tid + i * 64 * W;
            acc[i] = fma(gain, zt[w][(idx & (T - 1)) * ZP + (idx / T)], acc[i]);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kPer; i++) {
      const int idx = tid + i * 64 * W;
      const int p = (int)(c0 + (unsigned)(idx / T)) * kIirChunk - (int)a.off0 + t * T + (idx & (T - 1));
      if (p >= 0 && p < (int)a.n) a.out[(size_t)o * a.out_stride + p] = (float)acc[i];
    }
  }
}

}  // namespace earhip
