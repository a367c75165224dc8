// extent_kernels.h — libear's polar extent panner (src/object_based/polar_extent.cpp:12-302, core:
// src/object_based/polar_extent_scalar.cpp:25-108 / polar_extent_simd.hpp:28-134) as a batch kernel: ONE WAVE
// per (object, metadata block), over the point source panner of panner.h.
//
// libear spreads an object with width / height / depth over 1652 points on the sphere (37 rows, 5 degrees
// apart), each with the point source panner's gains precomputed: a weight per point (1 inside a "stadium"
// of width x height around the object's direction, fading to 0 over 10 degrees), the weighted sum of the
// points' gain vectors, normalised, blended by power with the point-source gains for extents under 10
// degrees, and for depth != 0 the rms of a near and a far rendering.  The weighting and the sum are the
// reference's one SIMD kernel (float, xsimd batches of 4-16 points); everything before it is scalar double
// set-up per call.
//
// Here the work is split between two kernels.  k_pan_objects (a thread per position, panner_kernels.h) does what
// is scalar in libear — extentMod, the share of the spread part, the basis at the object's direction, the
// stadium's parameters, the point source panner's gains for extents under 10 degrees — and leaves a JOB record
// per position that needs spreading.  k_pan_objects_extent takes ONE WAVE per job:
//   * the 1652 points are stored in 26 spatially compact chunks of 64 (bands of 8 rows cut along the azimuth)
//     with, per chunk, its mean direction, its angular radius and the float sum of its points' gain vectors;
//   * lane c classifies chunk c against the extent with one dot product: entirely outside (further from the
//     object than half the larger dimension + fade: every weight is 0), entirely inside (closer than half the
//     smaller dimension: every weight is 1 — the chunk's precomputed sum is added, like libear's all-ones
//     batches, polar_extent_simd.hpp:108-121), or on the boundary;
//   * only boundary chunks are evaluated: a lane per point (positions and gains read as whole 256-byte rows),
//     the per-lane partial sums meet in a butterfly of lane exchanges;
//   * from there lane s carries loudspeaker s: normalisation, the blend with the point-source gains, depth's
//     rms of two renderings, gain, LFE mask, the direct / diffuse split.
// Arithmetic types follow the reference: float weights and sums (extent_float_t), double around them.  The
// order of the float additions differs from the scalar core's (as it does between the reference's scalar and
// SIMD cores, which its tests hold to 1e-5: tests/extent_tests.cpp:140-169).
//
// The set-up per position, the weight of a point, the classification of a chunk and the grid's geometry are
// extent.h (plain C++, also compiled on the CPU); here are the tables' device form, the job record and the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "extent.h"
#include "panner.h"

namespace earhip {

struct ExtentTable {
  int n_points;  // 1652
  int n_padded;  // multiple of 64; padded points carry zero gains
  int n_chunks;  // n_padded / 64 (26)
  int n_pv;      // panner outputs: loudspeakers without LFE, or 2 for 0+2+0
  const float *xs, *ys, *zs;  // [n_padded], chunk after chunk
  const float *gains;         // [n_pv][n_padded]
  const float *chunk_dir;     // [3][kExtentMaxChunks]: unit mean direction of a chunk's points
  const float *chunk_rad;     // [kExtentMaxChunks]: largest angle between it and a point of the chunk (radians)
  const float *chunk_sum;     // [kExtentMaxChunks][kMaxPanOut]: float sum of the chunk's gain vectors
};

constexpr int kExtentWaves = 4;          // positions per workgroup

// what k_pan_objects leaves for k_pan_objects_extent
struct ExtentJob {
  int pos;                 // index of the position in the call's arrays
  int n_pass;              // renderings: 1, or 2 with depth
  double spread[2];        // share of the spread part per rendering (:263-266)
  ExtentWeighting W[2];
  float dir[3];            // the object's direction (unit; +y for the origin, :52-60)
  double psq[kMaxPanOut];  // the point source panner's gains squared (zero when no rendering needs them)
};

// One job rendered by a wave: what lane s (< E.n_pv) returns is the panner's output s of PolarExtent::handle
// (:290-302), lanes past E.n_pv return 0.  Every lane of the wave calls it.
__device__ inline double extent_render(const ExtentTable &E, const ExtentJob &J, int lane) {
  const int S = E.n_pv;
  const int n_pass = J.n_pass;
  // lane c looks at chunk c: the angle between its mean direction and the object's
  float chunk_angle = 0.0f, chunk_rad = 0.0f;
  if (lane < E.n_chunks) {
    const float cd = E.chunk_dir[lane] * J.dir[0] + E.chunk_dir[kExtentMaxChunks + lane] * J.dir[1] +
                     E.chunk_dir[2 * kExtentMaxChunks + lane] * J.dir[2];
    chunk_angle = acosf(fminf(fmaxf(cd, -1.0f), 1.0f));
    chunk_rad = E.chunk_rad[lane];
  }
  // From here on lane s (< S) carries the panner's output s.
  const double psq = lane < S ? J.psq[lane] : 0.0;
  double fin = 0.0;
  for (int k = 0; k < n_pass; k++) {  // calc_pv_spread (:257-288)
    const double amount_spread = J.spread[k], amount_point = 1.0 - amount_spread;
    double out = amount_point > 1e-10 ? amount_point * psq : 0.0;
    if (amount_spread > 1e-10) {
      const ExtentWeighting &W = J.W[k];
      const bool is_chunk = lane < E.n_chunks;
      const ExtentChunkClass chunk_class = extent_chunk_class(W, chunk_angle, chunk_rad);
      const bool outside = is_chunk && chunk_class == kExtentChunkOutside;
      const bool inside = is_chunk && chunk_class == kExtentChunkInside;
      unsigned long long m_inside = __ballot(inside);
      unsigned long long m_edge = __ballot(is_chunk && !outside && !inside);
      // chunks entirely inside: their precomputed sums (lane s adds loudspeaker s)
      float total = 0.0f;
      while (m_inside) {
        const int c = __ffsll((long long)m_inside) - 1;
        m_inside &= m_inside - 1;
        if (lane < S) total += E.chunk_sum[c * kMaxPanOut + lane];
      }
      // chunks on the boundary: a lane per point
      float acc[kMaxPanOut];
#pragma unroll
      for (int s = 0; s < kMaxPanOut; s++) acc[s] = 0.0f;
      const bool any_edge = m_edge != 0;
      while (m_edge) {
        const int c = __ffsll((long long)m_edge) - 1;
        m_edge &= m_edge - 1;
        const int q = c * 64 + lane;
        const float w = extent_weight(W, E.xs[q], E.ys[q], E.zs[q]);
        if (__ballot(w != 0.0f) == 0) continue;
        const float *g = E.gains + q;
#pragma unroll
        for (int s = 0; s < kMaxPanOut; s++)
          if (s < S) acc[s] += w * g[(size_t)s * E.n_padded];
      }
      if (any_edge) {
#pragma unroll
        for (int s = 0; s < kMaxPanOut; s++)
          if (s < S) {
            float v = acc[s];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if (lane == s) total += v;
          }
      }
      float n2 = total * total;  // (lanes >= S hold 0)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) n2 += __shfl_xor(n2, off);
      const float scale = (float)(1.0 / (double)sqrtf(n2));  // (:281: float norm, double reciprocal, float scaling)
      const float r = total * scale;
      out += amount_spread * (double)(r * r);
    }
    const double v = sqrt(out);
    fin = n_pass == 2 ? fin + v * v : v;
  }
  if (n_pass == 2) fin = sqrt(fin / 2.0);  // (:297-299)
  return fin;
}

// lane c writes channel c of the full layout for position i: the panner output that feeds it (none: an LFE
// channel) out of the lanes' fin, gain, sqrt(1 - diffuse) / sqrt(diffuse) (gain_calculator_objects.cpp:47-56).
// Every lane of the wave calls it.
__device__ inline void extent_write(const PanParams &P, double fin, size_t i, int lane, const double *gain,
                                    const double *diffuse, float *direct, float *diff) {
  const int src = lane < P.n_full ? P.real_of_full[lane] : -1;
  const double got = __shfl(fin, src < 0 ? 0 : src);
  if (lane < P.n_full) {
    const double g = gain ? gain[i] : 1.0, df = diffuse ? diffuse[i] : 0.0;
    const double v = src < 0 ? 0.0 : got * g;
    direct[i * P.n_full + lane] = (float)(v * sqrt(1.0 - df));
    diff[i * P.n_full + lane] = (float)(v * sqrt(df));
  }
}

// direct / diffuse [npos][n_full] float for the jobs k_pan_objects left.  Wave w of the launch takes jobs[w];
// waves past *job_count leave at once.
static __global__ void __launch_bounds__(64 * kExtentWaves)
k_pan_objects_extent(PanParams P, ExtentTable E, const ExtentJob *jobs, const unsigned *job_count, const double *gain,
                     const double *diffuse, float *direct, float *diff) {
  const int lane = threadIdx.x & 63;
  const unsigned wi = __builtin_amdgcn_readfirstlane(blockIdx.x * kExtentWaves + (threadIdx.x >> 6));
  if (wi >= *job_count) return;  // (whole waves)
  const ExtentJob &J = jobs[wi];
  extent_write(P, extent_render(E, J, lane), (size_t)J.pos, lane, gain, diffuse, direct, diff);
}

}  // namespace earhip
