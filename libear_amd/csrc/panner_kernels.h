// panner_kernels.h — the Objects gain producer's batch kernels over the core of panner.h: libear's GainCalculatorObjects
// (src/object_based/gain_calculator_objects.cpp:24-57) for point sources — the point source panner, the LFE mask and the
// sqrt(1 - diffuse) / sqrt(diffuse) split — one thread per (object, metadata block), and the panner sampled at unit
// vectors in double for set-up (the extent grid, the HOA design, the self check).
//
// At 10^4 x real time a scene of 1024 objects with an ADM block every 20 ms needs 5 * 10^8 gain vectors per wall-clock
// second; the reference computes them one at a time on the host (virtual dispatch over region objects, Eigen
// temporaries).  Results are identical after the cast to float in all but rounding-boundary cases.
#pragma once
#include <hip/hip_runtime.h>

#include "extent_kernels.h"
#include "panner.h"

namespace earhip {

// The scalar part of one position (everything that is scalar double work in libear): the renderings of
// PolarExtent::handle with the share of the spread part in each (may_spread false: a distance of 1 and no extent,
// nothing is spread), and, where a rendering needs them, the point source panner's outputs pv[0 .. n_pv).
// false: no region took the position.
__device__ inline bool pan_prepare(const PanParams &P, Vec3 p, bool may_spread, double width, double height, double depth,
                                   ExtentPasses &X, bool &spread_any, double (&pv)[kMaxPanOut], int &n_pv) {
  X.n_pass = 1;
  X.spread[0] = X.spread[1] = 0.0;
  if (may_spread) extent_passes(p, width, height, depth, X);
  spread_any = false;
  bool need_point = false;
  for (int k = 0; k < X.n_pass; k++) {
    spread_any = spread_any || X.spread[k] > 1e-10;
    need_point = need_point || (1.0 - X.spread[k]) > 1e-10;
  }
  n_pv = 0;
  if (need_point) {
    double real[kMaxPanOut];
    if (!pan_full(P.table, p, real)) return false;
    n_pv = pan_outputs(P, real, pv);
  }
  return true;
}

// what a wave needs to render position `pos` at p (extent_render)
__device__ inline void extent_job_fill(ExtentJob &J, int pos, Vec3 p, const ExtentPasses &X, const double (&pv)[kMaxPanOut],
                                       int n_pv) {
  J.pos = pos;
  J.n_pass = X.n_pass;
  for (int k = 0; k < 2; k++) {
    J.spread[k] = X.spread[k];
    // (:270-272: at least half the fade width in each dimension)
    if (k < X.n_pass && X.spread[k] > 1e-10)
      extent_setup(p, fmax(X.w[k], kExtentFade / 2.0), fmax(X.h[k], kExtentFade / 2.0), J.W[k]);
  }
  const double n = sqrt(p.x * p.x + p.y * p.y + p.z * p.z);
  J.dir[0] = n < 1e-10 ? 0.0f : (float)(p.x / n);
  J.dir[1] = n < 1e-10 ? 1.0f : (float)(p.y / n);
  J.dir[2] = n < 1e-10 ? 0.0f : (float)(p.z / n);
  for (int c = 0; c < kMaxPanOut; c++) J.psq[c] = c < n_pv ? pv[c] * pv[c] : 0.0;
}

// Position i at p by one thread: rows i of direct / diffuse [npos][n_full] float; *missed counts positions no region
// took.  Positions that libear spreads over the sphere — an extent, or a distance under 1, which widens even a
// zero extent (polar_extent.cpp:62-70) — are prepared here and left as a job for k_pan_objects_extent (a wave each).
// jobs == NULL: every distance is 1 and there is no extent.
__device__ inline void pan_object(const PanParams &P, size_t i, Vec3 p, double width, double height, double depth,
                                  const double *gain, const double *diffuse, float *direct, float *diff, unsigned *missed,
                                  ExtentJob *jobs, unsigned *job_count) {
  ExtentPasses X;
  bool spread_any;
  double pv[kMaxPanOut];
  int n_pv;
  float *d = direct + i * P.n_full, *f = diff + i * P.n_full;
  if (!pan_prepare(P, p, jobs != nullptr, width, height, depth, X, spread_any, pv, n_pv)) {
    for (int c = 0; c < P.n_full; c++) d[c] = f[c] = 0.0f;
    atomicAdd(missed, 1u);
    return;
  }
  if (spread_any) {
    extent_job_fill(jobs[atomicAdd(job_count, 1u)], (int)i, p, X, pv, n_pv);
    return;
  }
  for (int c = 0; c < P.n_full; c++) d[c] = f[c] = 0.0f;
  const double g = gain ? gain[i] : 1.0, df = diffuse ? diffuse[i] : 0.0;
  const double sd = sqrt(1.0 - df), sf = sqrt(df);
  for (int c = 0; c < n_pv; c++) {
    // PolarExtent without spread: sqrt(amount_point pv^2), with depth the rms of two of them
    // (src/object_based/polar_extent.cpp:257-302); gain; split (gain_calculator_objects.cpp:47-56)
    double v = sqrt((1.0 - X.spread[0]) * (pv[c] * pv[c]));
    if (X.n_pass == 2) {
      const double v2 = sqrt((1.0 - X.spread[1]) * (pv[c] * pv[c]));
      v = sqrt((v * v + v2 * v2) / 2.0);
    }
    v *= g;
    const int o = P.stereo ? P.stereo_index[c] : P.full_index[c];
    d[o] = (float)(v * sd);
    f[o] = (float)(v * sf);
  }
}

// One thread per position (pan_object).
static __global__ void __launch_bounds__(128)
k_pan_objects(PanParams P, size_t npos, const double *az, const double *el, const double *dist, const double *width,
              const double *height, const double *depth, const double *gain, const double *diffuse, float *direct,
              float *diff, unsigned *missed, ExtentJob *jobs, unsigned *job_count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npos) return;
  const Vec3 p = polar_to_cart(az[i], el[i], dist ? dist[i] : 1.0);
  pan_object(P, i, p, width ? width[i] : 0.0, height ? height[i] : 0.0, depth ? depth[i] : 0.0, gain, diffuse, direct, diff,
             missed, jobs, job_count);
}

// HOA decoder design and the extent panner's point grid: panning values of unit vectors in double,
// [npos][n_pv] (2 for 0+2+0)
static __global__ void __launch_bounds__(128)
k_pan_points(PanParams P, size_t npos, const double *xyz, double *pv_out, unsigned *missed) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npos) return;
  const Vec3 p = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  double real[kMaxPanOut], pv[kMaxPanOut];
  const int n_pv = P.stereo ? 2 : P.table.n_real;
  if (!pan_full(P.table, p, real)) {
    atomicAdd(missed, 1u);
    for (int c = 0; c < n_pv; c++) pv_out[i * n_pv + c] = 0.0;
    return;
  }
  pan_outputs(P, real, pv);
  for (int c = 0; c < n_pv; c++) pv_out[i * n_pv + c] = pv[c];
}

// earhip_panner_self_check: what a workgroup found over its directions
struct SelfCheckPartial {
  unsigned missed;         // directions no region took
  double max_power_error;  // max |sum pv^2 - 1| over the others
  double min_own_gain;     // min over the loudspeaker directions of the loudspeaker's own gain (2.0: none in this workgroup)
};
constexpr int kSelfCheckThreads = 256;

// One thread per direction: the first n_design rows of xyz are the t-design, row n_design + k is the real direction of
// panner output k.  Each direction goes through pan_full / pan_outputs as in k_pan_points; the three results are reduced
// over the wave with shuffles, over the workgroup through LDS, and written as partial[blockIdx.x] — no atomics, so the
// host's pass over the partials in index order gives the same bits for the same panner.
static __global__ void __launch_bounds__(kSelfCheckThreads)
k_pan_self_check(PanParams P, int n_dirs, int n_design, const double *xyz, SelfCheckPartial *partial) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  unsigned missed = 0;
  double err = 0.0, own = 2.0;
  if (i < n_dirs) {
    const Vec3 p = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    double real[kMaxPanOut], pv[kMaxPanOut];
    if (!pan_full(P.table, p, real)) {
      missed = 1;
    } else {
      const int n_pv = pan_outputs(P, real, pv);
      double power = 0.0;
      for (int c = 0; c < n_pv; c++) power += pv[c] * pv[c];
      err = fabs(power - 1.0);
      // (a NaN would be dropped by fmax: let it through as an error no bound accepts)
      if (!(err == err)) err = 1e300;
      const int k = i - n_design;
      if (k >= 0 && k < n_pv) own = pv[k] == pv[k] ? pv[k] : -1e300;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    missed += __shfl_xor(missed, off);
    err = fmax(err, __shfl_xor(err, off));
    own = fmin(own, __shfl_xor(own, off));
  }
  constexpr int kWaves = kSelfCheckThreads / 64;
  __shared__ unsigned s_missed[kWaves];
  __shared__ double s_err[kWaves], s_own[kWaves];
  const int wave = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) s_missed[wave] = missed, s_err[wave] = err, s_own[wave] = own;
  __syncthreads();
  if (threadIdx.x == 0) {
    SelfCheckPartial r = {s_missed[0], s_err[0], s_own[0]};
    for (int w = 1; w < kWaves; w++) {
      r.missed += s_missed[w];
      r.max_power_error = fmax(r.max_power_error, s_err[w]);
      r.min_own_gain = fmin(r.min_own_gain, s_own[w]);
    }
    partial[blockIdx.x] = r;
  }
}

}  // namespace earhip
