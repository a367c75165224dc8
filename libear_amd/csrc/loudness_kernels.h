// loudness_kernels.h — the device side of the programme loudness meter (include/earhip.h, group L; the maths: loudness.h).
//
// A recursive filter does not fit one-thread-per-output.  The time axis of a call is cut, per channel, into CHUNKS of L samples
// on the meter's own clock grid (L divides the 100 ms step, so a chunk lies inside one step; the first and the last chunk of a
// call may be partial), and a lane walks one chunk:
//   k_loudness_pass<false>  every (channel, chunk) from the ZERO state; keeps the end state e        [C][cap][4]
//   k_loudness_propagate    S[k+1] = Phi^len(k) S[k] + e[k] per channel: the true start state of every chunk [C][cap][4], and
//                           the state the next call starts from.  The chain over the whole chunks in the middle is a scan: a
//                           wave takes 64 chunks (Hillis-Steele with Phi^(L 2^d)), the waves of a workgroup take the groups of
//                           64 side by side, one thread chains the group sums with Phi^(64 L), and every lane finishes with
//                           Phi^(L (i + 1)) times its group's carry-in.  Fixed order: no atomics anywhere
//   k_loudness_pass<true>   every chunk again from its true start state; the sum of y^2 of the chunk   [C][cap]
//   k_loudness_steps        one thread per (channel, step the call touches): the sum so far of the open step, then the chunks of
//                           the step in ascending order; a step that the call completes goes to the step store as a mean, the
//                           sum of one it leaves open goes to the OTHER of two `open` words (read [par], written [par ^ 1])
// The rows are read through LDS: the 64 lanes of a wave walk 64 consecutive chunks of one row, L * 4 bytes apart, so a tile of
// kLoudTile samples of each chunk is fetched by the wave with two coalesced 128-byte runs per load (scalar loads: a row may
// start at any float), kept in registers while the tile before it is filtered, and then laid down in LDS rows of an odd pitch
// (lane l reads row l: different banks).
#pragma once
#include <hip/hip_runtime.h>

#include "loudness.h"

namespace earhip {

constexpr int kLoudTile = 32;                // samples of a chunk per LDS tile
constexpr int kLoudPitch = kLoudTile + 1;    // odd
constexpr int kLoudPropThreads = 1024;       // 16 waves chain the groups of 64 chunks of a channel side by side
constexpr int kLoudQPitch = 17;              // doubles between the 4x4 matrices of the propagation's table in LDS
constexpr int kLoudGroupsPerWave = 4;        // ... so a launch takes at most 16 * 4 * 64 whole chunks + 2
constexpr int kLoudMaxChunks = (kLoudPropThreads / 64) * kLoudGroupsPerWave * 64;  // chunks of one launch (cap of the scratch)

struct LoudArgs {
  const float *rows;     // [C][stride], samples [0, n) of this launch
  size_t stride;
  unsigned n;            // samples of this launch (<= (kLoudMaxChunks - 1) * L)
  unsigned off0;         // clock of sample 0 modulo L: chunk 0 of the launch starts off0 samples BEFORE sample 0
  unsigned nchunks;
  int L, C;
  KCoeffs<double> k;
  double *e;             // [C][kLoudMaxChunks][4]
  double *start;         // [C][kLoudMaxChunks][4]
  double *q;             // [C][kLoudMaxChunks]
  double *state;         // [C][4]
  const double *P;       // [L + 1][16]  Phi^j
  const double *Q;       // [65][16]     Phi^(L j)
  // steps
  double *open;          // [2][C]
  int par;
  unsigned cps;          // chunks per step
  unsigned chunk0_in_step;  // index within its step of chunk 0 of the launch
  unsigned long long step0; // the step chunk 0 lies in
  double *steps;         // [max_steps][C]
  double step_samples;   // samples of a step
};

// samples [lo, lo + len) of the launch are chunk c's (a launch is at most kLoudMaxChunks * L samples: int arithmetic)
__device__ inline void loud_chunk_range(const LoudArgs &a, unsigned c, unsigned &lo, unsigned &len) {
  const int b0 = (int)c * a.L - (int)a.off0;
  const int l = max(b0, 0), h = min(b0 + a.L, (int)a.n);
  lo = (unsigned)l;
  len = (unsigned)(h - l);
}

template <bool kSecond>
__global__ __launch_bounds__(64) void k_loudness_pass(LoudArgs a) {
  __shared__ float tile[64 * kLoudPitch];
  const int lane = threadIdx.x;
  const int ch = blockIdx.y;
  const unsigned c0 = blockIdx.x * 64u, c = c0 + lane;
  const bool live = c < a.nchunks;
  // sample j of chunk c (j in [0, L)) is sample c * L - off0 + j of the launch; this lane's chunk holds j in [jlo, jhi)
  int jlo = 0, jhi = 0;
  if (live) {
    const int b0 = (int)c * a.L - (int)a.off0;
    jlo = max(-b0, 0);
    jhi = min(a.L, (int)a.n - b0);
  }
  const float *row = a.rows + (size_t)ch * a.stride;
  KState<double> st{{0.0, 0.0, 0.0, 0.0}};
  if (kSecond && live) {
    const double *s = a.start + ((size_t)ch * kLoudMaxChunks + c) * 4;
    for (int i = 0; i < 4; i++) st.s[i] = s[i];
  }
  double acc = 0.0;

  // The wave's fetch of one tile: load i of the 32 takes chunks (2 i, 2 i + 1) of the 64, lane l sample l % 32 of the tile:
  // two runs of 128 bytes per load.  The loads are UNCONDITIONAL, their index clamped into the launch's samples [0, n): a
  // sample outside the launch (before the first chunk's first, behind the last chunk's last, beyond L in the last tile) reads
  // a neighbour that no lane consumes (the filter loop below stays inside [jlo, jhi)).  A load under a condition is a branch
  // and a wait of its own: 32 latencies in a row per tile instead of one, 40 us per pass instead of 16.
  const int fs = lane & 31, fh = lane >> 5;
  const int pbase = (int)(c0 + fh) * a.L - (int)a.off0 + fs;  // launch sample of (chunk c0 + fh, j = fs)
  const int plast = (int)a.n - 1;
  float pre[kLoudTile];
  auto fetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < kLoudTile; i++) {
      const int p = pbase + t * kLoudTile + 2 * i * a.L;
      pre[i] = row[min(max(p, 0), plast)];
    }
  };
  const int ntiles = (a.L + kLoudTile - 1) / kLoudTile;
  fetch(0);
  for (int t = 0; t < ntiles; t++) {
    __syncthreads();  // (the tile before this one has been read)
#pragma unroll
    for (int i = 0; i < kLoudTile; i++) tile[(2 * i + fh) * kLoudPitch + fs] = pre[i];
    __syncthreads();
    if (t + 1 < ntiles) fetch(t + 1);  // in flight while this tile is filtered
    const int j0 = t * kLoudTile;
    const float *mine = tile + lane * kLoudPitch;
    if (j0 >= jlo && j0 + kLoudTile <= jhi) {
#pragma unroll
      for (int s = 0; s < kLoudTile; s++) {
        const double y = k_weight_step(a.k, st, (double)mine[s]);
        if (kSecond) acc = fma(y, y, acc);
      }
    } else {
      for (int s = max(jlo - j0, 0); s < kLoudTile && j0 + s < jhi; s++) {
        const double y = k_weight_step(a.k, st, (double)mine[s]);
        if (kSecond) acc = fma(y, y, acc);
      }
    }
  }
  if (live) {
    if (kSecond) {
      a.q[(size_t)ch * kLoudMaxChunks + c] = acc;
    } else {
      double *e = a.e + ((size_t)ch * kLoudMaxChunks + c) * 4;
      for (int i = 0; i < 4; i++) e[i] = st.s[i];
    }
  }
}

__device__ inline KState<double> loud_load4(const double *p) {
  KState<double> s;
  for (int i = 0; i < 4; i++) s.s[i] = p[i];
  return s;
}

__global__ __launch_bounds__(kLoudPropThreads) void k_loudness_propagate(LoudArgs a) {
  __shared__ double gsum[kLoudMaxChunks / 64][4];   // c of the last lane of every group
  __shared__ double carry[kLoudMaxChunks / 64][4];  // the state that enters every group
  __shared__ double Qs[65 * kLoudQPitch];           // Phi^(L j), j = 0 .. 64, rows of an odd pitch (lane l reads matrix l + 1)
  const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)ch * kLoudMaxChunks;
  const double *E = a.e + base * 4;
  double *S = a.start + base * 4;
  const KState<double> zero{{0.0, 0.0, 0.0, 0.0}};
  // the whole chunks in the middle: m of them, chunk 1 + i.  Their end states are fetched first: everything below waits for
  // global memory once, not once per step of the chain
  const unsigned m = a.nchunks >= 2 ? a.nchunks - 2 : 0;
  const unsigned groups = (m + 63) / 64;
  KState<double> cs[kLoudGroupsPerWave];
#pragma unroll
  for (int r = 0; r < kLoudGroupsPerWave; r++) {
    const unsigned i = ((unsigned)wave + (unsigned)r * (kLoudPropThreads / 64)) * 64 + lane;
    cs[r] = i < m ? loud_load4(E + 4 * (size_t)(1 + i)) : zero;
  }
  const KState<double> e_last = loud_load4(E + 4 * (size_t)(a.nchunks - 1));
  // ... and the powers of Phi^L go to LDS in the same round trip (one number per thread): read from global memory where they
  // are used, each of the scan's steps waited for a miss of its own (the passes have just swept the caches): 27 us, not 9
  for (int i = tid; i < 65 * 16; i += kLoudPropThreads) Qs[(i >> 4) * kLoudQPitch + (i & 15)] = a.Q[i];
  const KState<double> s0 = loud_load4(a.state + 4 * ch);
  unsigned lo, len0, len_last;
  loud_chunk_range(a, 0, lo, len0);
  loud_chunk_range(a, a.nchunks - 1, lo, len_last);
  double Plast[16];
  for (int i = 0; i < 16; i++) Plast[i] = a.P[16 * (size_t)len_last + i];
  // the first chunk (it may be partial)
  const KState<double> s1 = k_state_advance(a.P + 16 * (size_t)len0, s0, loud_load4(E));
  __syncthreads();  // (every thread has read the state before anyone writes it)
  if (a.nchunks == 1) {
    if (tid == 0) {
      for (int i = 0; i < 4; i++) S[i] = s0.s[i], a.state[4 * ch + i] = s1.s[i];
    }
    return;
  }
  if (tid == 0)
    for (int i = 0; i < 4; i++) S[i] = s0.s[i], S[4 + i] = s1.s[i];
  // S[2 + i] = the state that leaves chunk 1 + i
#pragma unroll
  for (int r = 0; r < kLoudGroupsPerWave; r++) {
    const unsigned g = (unsigned)wave + (unsigned)r * (kLoudPropThreads / 64);
    if (g >= groups) continue;  // (uniform over the wave)
    KState<double> c = cs[r];
    // inclusive scan: c_i = sum over j <= i of Phi^(L (i - j)) e_j
    for (int d = 0; d < 6; d++) {
      KState<double> up;
      for (int k = 0; k < 4; k++) up.s[k] = __shfl_up(c.s[k], 1u << d, 64);
      if (lane >= (1 << d)) c = k_state_advance(Qs + kLoudQPitch * (1 << d), up, c);
    }
    cs[r] = c;
    if (lane == 63)
      for (int k = 0; k < 4; k++) gsum[g][k] = c.s[k];
  }
  __syncthreads();
  if (tid == 0) {
    KState<double> cr = s1;
    double q64[16];  // (in registers: the loop's stores to LDS would have it read again every round)
    for (int i = 0; i < 16; i++) q64[i] = Qs[kLoudQPitch * 64 + i];
    for (unsigned g = 0; g < groups; g++) {
      for (int k = 0; k < 4; k++) carry[g][k] = cr.s[k];
      KState<double> gs;
      for (int k = 0; k < 4; k++) gs.s[k] = gsum[g][k];
      cr = k_state_advance(q64, cr, gs);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kLoudGroupsPerWave; r++) {
    const unsigned g = (unsigned)wave + (unsigned)r * (kLoudPropThreads / 64);
    if (g >= groups) continue;
    const unsigned i = g * 64 + lane;
    if (i >= m) continue;
    KState<double> cin;
    for (int k = 0; k < 4; k++) cin.s[k] = carry[g][k];
    const KState<double> out = k_state_advance(Qs + kLoudQPitch * (lane + 1), cin, cs[r]);
    for (int k = 0; k < 4; k++) S[4 * (size_t)(2 + i) + k] = out.s[k];
    if (i == m - 1) {
      // ... which enters the last chunk (it may be partial): the state the next call starts from
      const KState<double> fin = k_state_advance(Plast, out, e_last);
      for (int k = 0; k < 4; k++) a.state[4 * ch + k] = fin.s[k];
    }
  }
  if (m == 0 && tid == 0) {
    const KState<double> fin = k_state_advance(Plast, s1, e_last);
    for (int k = 0; k < 4; k++) a.state[4 * ch + k] = fin.s[k];
  }
}

// nsteps_touched: the steps chunk 0 .. nchunks - 1 of the launch lie in
__global__ __launch_bounds__(64) void k_loudness_steps(LoudArgs a, unsigned nsteps_touched) {
  const unsigned idx = blockIdx.x * 64u + threadIdx.x;
  if (idx >= nsteps_touched * (unsigned)a.C) return;
  const unsigned s = idx / (unsigned)a.C;
  const int ch = (int)(idx - s * (unsigned)a.C);
  // chunks of the launch in step step0 + s: launch chunk index = s * cps - chunk0_in_step + (0 .. cps)
  const long long first = (long long)s * a.cps - (long long)a.chunk0_in_step;
  const long long b = first > 0 ? first : 0;
  const long long e_ = first + a.cps < (long long)a.nchunks ? first + a.cps : (long long)a.nchunks;
  double acc = s == 0 ? a.open[(size_t)a.par * a.C + ch] : 0.0;
  const double *q = a.q + (size_t)ch * kLoudMaxChunks;
  for (long long c = b; c < e_; c++) acc += q[c];
  // the step is complete when the launch reaches its last sample
  const long long step_end = (first + a.cps) * a.L - (long long)a.off0;  // launch sample index one past the step
  if (step_end <= (long long)a.n) {
    a.steps[(size_t)(a.step0 + s) * a.C + ch] = acc / a.step_samples;
    if (s == nsteps_touched - 1) a.open[(size_t)(a.par ^ 1) * a.C + ch] = 0.0;
  } else {
    a.open[(size_t)(a.par ^ 1) * a.C + ch] = acc;  // (only the last step of a launch can stay open)
  }
}

}  // namespace earhip
