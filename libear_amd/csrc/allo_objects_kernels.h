// allo_objects_kernels.h — the device form of earhip group U (api_allo.hip): the allocentric panner with channelLock,
// divergence and extent.  Lanes over (object, loudspeaker): a workgroup of 256 threads holds 256 / W objects, W the power of
// two at or above the channel count (2 .. 32), and lane (o, c) computes loudspeaker c of object o with allo_objects.h's
// channel_terms — c's neighbours under the object's mask from the by-value table (so a masked object takes the same path as
// an unmasked one and no table of grid weights is kept anywhere), then the at most 60 terms of its three axis sums.  The 60-term
// sums of an object's loudspeakers so run side by side.  Steps 1 and 2 (lock, divergence) are per object and every lane of
// the object repeats them: their loops over the table are uniform, their reads scalar.  The normalisation is a fixed-order
// sum: the lanes leave G_c in LDS and each adds its object's W entries in channel order, as the host form does.  Rows leave
// through two LDS tiles, which are the workgroup's contiguous runs of direct and diffuse_out, as full-width stores.
#pragma once

#include <hip/hip_runtime.h>

#include "allo_objects.h"

namespace earhip {
namespace allo {

constexpr int kObjectsThreads = 256;
// log2 of W, the lanes an object takes
inline int objects_log2_width(int n_channels) {
  int l = 1;
  while ((1 << l) < n_channels) l++;
  return l;
}
inline int objects_per_workgroup(int n_channels) { return kObjectsThreads >> objects_log2_width(n_channels); }

__global__ void __launch_bounds__(kObjectsThreads)
    k_allo_objects(Table t, Extras e, int log2_width, size_t n, const double *__restrict__ x, const double *__restrict__ y,
                   const double *__restrict__ z, const double *__restrict__ width, const double *__restrict__ height,
                   const double *__restrict__ depth, const double *__restrict__ gain, const double *__restrict__ diffuse,
                   const unsigned char *__restrict__ channel_lock, const double *__restrict__ lock_max_distance,
                   const double *__restrict__ divergence, const double *__restrict__ position_range,
                   const uint32_t *__restrict__ excluded, float *__restrict__ direct, float *__restrict__ diffuse_out,
                   int *__restrict__ status) {
  __shared__ double G_all[3][kObjectsThreads];
  __shared__ float tile[2][kObjectsThreads];  // [direct, diffuse][object * n_channels + channel]
  const int tid = threadIdx.x, local = tid >> log2_width, c = tid & ((1 << log2_width) - 1);
  const int per_wg = kObjectsThreads >> log2_width;
  const size_t first = (size_t)blockIdx.x * per_wg;  // the workgroup's first object (first < n: the grid is sized so)
  const size_t i = first + local;
  const bool live = i < n;
  const double px = live ? x[i] : 0.0, py = live ? y[i] : 0.0, pz = live ? z[i] : 0.0;
  const double sw = live && width ? width[i] : 0.0, sh = live && height ? height[i] : 0.0, sd = live && depth ? depth[i] : 0.0;
  const double g = live && gain ? gain[i] : 1.0, d = live && diffuse ? diffuse[i] : 0.0;
  const bool lock = live && channel_lock ? channel_lock[i] != 0 : false;
  const double maxd = live && lock_max_distance ? lock_max_distance[i] : HUGE_VAL;
  const double v = live && divergence ? divergence[i] : 0.0, r = live && position_range ? position_range[i] : 0.0;
  const uint32_t mask = live && excluded ? excluded[i] : 0u;
  const bool ok = position_valid(px, py, pz, g, d) && objects_valid(sw, sh, sd, maxd, v, r);
  if (live && status && c == 0) status[i] = ok ? 0 : 1;

  Object o;
  prepare_object(t, e, ok ? px : 0.0, ok ? py : 0.0, ok ? pz : 0.0, ok ? sw : 0.0, ok ? sh : 0.0, ok ? sd : 0.0, ok && lock,
                 ok ? maxd : 0.0, ok ? v : 0.0, ok ? r : 0.0, mask, o);
  double w[3], G[3];
  channel_terms(t, e, o, c, w, G);  // (zeros for c at or beyond the channel count)
  for (int k = 0; k < 3; k++) G_all[k][tid] = G[k];
  __syncthreads();
  double norm[3] = {1.0, 1.0, 1.0};
  if (o.extent) {
    const int base = local << log2_width;
    for (int k = 0; k < 3; k++) {
      if (k >= o.n_pos) continue;
      double sum = 0.0;
      for (int cc = 0; cc < t.n; cc++) sum += G_all[k][base + cc] * G_all[k][base + cc];
      norm[k] = sqrt(sum);
    }
  }
  if (c < t.n) {
    const double gc = combine(o, w, G, norm);
    const float nan = __int_as_float(0x7fc00000);
    tile[0][local * t.n + c] = ok ? row_value(gc, g, direct_factor(d)) : nan;
    tile[1][local * t.n + c] = ok ? row_value(gc, g, diffuse_factor(d)) : nan;
  }
  __syncthreads();
  const size_t left = n - first;
  const unsigned rows = left < (size_t)per_wg ? (unsigned)left : (unsigned)per_wg;
  const unsigned count = rows * (unsigned)t.n;  // at most 256: one store per thread and output
  if ((unsigned)tid < count) {
    direct[first * (size_t)t.n + tid] = tile[0][tid];
    if (diffuse_out) diffuse_out[first * (size_t)t.n + tid] = tile[1][tid];
  }
}

}  // namespace allo
}  // namespace earhip
