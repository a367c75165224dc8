// objects_kernels.h — channelLock, objectDivergence and zoneExclusion of an Objects audioBlockFormat (ITU-R BS.2127-0
// 7.3.6, 7.3.7, 7.3.12, in the form include/earhip.h group I specifies: libear refuses all three) around the point
// source and polar extent panners (panner_kernels.h, extent_kernels.h).
//
// Per object: the position may be replaced by the nearest loudspeaker's (lock), then becomes one or three positions
// with power weights (divergence); each goes through the extent panner as it stands; the weighted powers are summed
// and the power of excluded loudspeakers is handed to their nearest remaining neighbours (zone exclusion).
//
// Two kernels.  k_pan_objects_front (a thread per object) does the lock and the divergence positions.  An object that
// has none of the three takes pan_object there and then, the path of k_pan_objects, with the same bits.  Any other
// is left as an ObjectsJob for k_pan_objects_meta, ONE WAVE each: lanes 0 .. 2 prepare the one or three positions
// side by side (pan_prepare, extent_job_fill: libear's scalar double work) into the wave's LDS, then the wave renders
// them in turn (extent_render, lane s carrying panner output s), accumulates w_k fin^2, applies the downmix of the
// object's excluded set and writes the rows (extent_write).
#pragma once
#include <cmath>
#include <cstdint>

#include "panner_kernels.h"

namespace earhip {

constexpr int kObjMaxOut = 22;  // panner outputs of a layout: n_full <= 24 with two LFE channels in the largest

// the candidates of a channel lock: the panner's outputs at the positions it was created with, on the unit sphere,
// and each one's place in the layout's priority order (exact ties go to the lowest)
struct LockTable {
  int n;
  int rank[kObjMaxOut];
  double pos[kObjMaxOut][3];
};

// zone exclusion: groups[i][g] is the set (bits: panner outputs) of the g-th nearest group of loudspeakers of output
// i, itself first; unused entries are 0
struct ZoneTable {
  int n;
  unsigned groups[kObjMaxOut][kObjMaxOut];
};

// what k_pan_objects_front leaves for k_pan_objects_meta
struct ObjectsJob {
  int pos;            // index of the object in the call's arrays
  int n_k;            // positions: 1, or 3 with divergence
  unsigned excluded;  // panner outputs excluded (never all of them: that set excludes nothing)
  double w[3];        // power weights
  double p[3][3];     // positions
};

// jobs / job_count[0]: for k_pan_objects_extent; ojobs / job_count[1]: for k_pan_objects_meta.  The _device entry
// point cannot look at the values: a divergence is clamped to [0, 1] (NaN: 0), a NaN maxDistance lets no loudspeaker
// qualify.
static __global__ void __launch_bounds__(128)
k_pan_objects_front(PanParams P, LockTable L, size_t npos, const double *az, const double *el, const double *dist,
                    const double *width, const double *height, const double *depth, const double *gain, const double *diffuse,
                    const unsigned char *lock, const double *lock_max, const double *divergence, const double *az_range,
                    const uint32_t *excluded, bool may_spread, float *direct, float *diff, unsigned *missed, ExtentJob *jobs,
                    unsigned *job_count, ObjectsJob *ojobs) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npos) return;
  Vec3 p = polar_to_cart(az[i], el[i], dist ? dist[i] : 1.0);
  const bool locked = lock && lock[i];
  double v = divergence ? divergence[i] : 0.0;
  v = v > 0.0 ? fmin(v, 1.0) : 0.0;
  unsigned em = 0, all = 0;
  const uint32_t mask = excluded ? excluded[i] : 0u;
  for (int c = 0; c < P.n_full; c++) {
    const int s = P.real_of_full[c];
    if (s < 0) continue;
    all |= 1u << s;
    if (mask >> c & 1u) em |= 1u << s;
  }
  if (em == all) em = 0;
  if (!locked && v == 0.0 && em == 0) {
    pan_object(P, i, p, width ? width[i] : 0.0, height ? height[i] : 0.0, depth ? depth[i] : 0.0, gain, diffuse, direct, diff,
               missed, may_spread ? jobs : nullptr, job_count);
    return;
  }
  if (locked) {
    const double limit = (lock_max ? lock_max[i] : (double)INFINITY) + 1e-10;
    auto distance = [&](int c) {
      const double dx = p.x - L.pos[c][0], dy = p.y - L.pos[c][1], dz = p.z - L.pos[c][2];
      return sqrt(dx * dx + dy * dy + dz * dz);
    };
    double nearest = (double)INFINITY;
    for (int c = 0; c < L.n; c++) {
      const double d = distance(c);
      if (d < limit) nearest = fmin(nearest, d);
    }
    int pick = -1;
    for (int c = 0; c < L.n; c++) {
      const double d = distance(c);
      if (d < limit && d < nearest + 1e-10 && (pick < 0 || L.rank[c] < L.rank[pick])) pick = c;
    }
    if (pick >= 0) p = {L.pos[pick][0], L.pos[pick][1], L.pos[pick][2]};
  }
  ObjectsJob &O = ojobs[atomicAdd(job_count + 1, 1u)];
  O.pos = (int)i;
  O.excluded = em;
  if (v == 0.0) {
    O.n_k = 1;
    O.w[0] = 1.0;
    O.p[0][0] = p.x, O.p[0][1] = p.y, O.p[0][2] = p.z;
    return;
  }
  // the object's polar coordinates and the axes of its own frame: +y' at the object, x' to its right, z' above
  const double r = az_range ? az_range[i] : 45.0;
  const double a = -ext_degrees(atan2(p.x, p.y)), e = ext_degrees(atan2(p.z, hypot(p.x, p.y)));
  const double d = sqrt(p.x * p.x + p.y * p.y + p.z * p.z);
  const Vec3 ax = polar_to_cart(a - 90.0, 0.0, 1.0), ay = polar_to_cart(a, e, 1.0), az_ = polar_to_cart(a, e + 90.0, 1.0);
  const Vec3 q[3] = {polar_to_cart(0.0, 0.0, d), polar_to_cart(r, 0.0, d), polar_to_cart(-r, 0.0, d)};
  O.n_k = 3;
  O.w[0] = (1.0 - v) / (1.0 + v);
  O.w[1] = O.w[2] = v / (1.0 + v);
  for (int k = 0; k < 3; k++) {
    O.p[k][0] = q[k].x * ax.x + q[k].y * ay.x + q[k].z * az_.x;
    O.p[k][1] = q[k].x * ax.y + q[k].y * ay.y + q[k].z * az_.y;
    O.p[k][2] = q[k].x * ax.z + q[k].y * ay.z + q[k].z * az_.z;
  }
}

// Wave w of the launch takes ojobs[w]; waves past *ojob_count only keep the workgroup's barrier company.
static __global__ void __launch_bounds__(64 * kExtentWaves)
k_pan_objects_meta(PanParams P, ExtentTable E, ZoneTable Z, const ObjectsJob *ojobs, const unsigned *ojob_count,
                   const double *width, const double *height, const double *depth, const double *gain, const double *diffuse,
                   bool may_spread, float *direct, float *diff, unsigned *missed) {
  __shared__ ExtentJob sub[kExtentWaves][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned wi = __builtin_amdgcn_readfirstlane(blockIdx.x * kExtentWaves + wave);
  const bool active = wi < *ojob_count;  // (whole waves)
  const ObjectsJob &O = ojobs[active ? wi : 0];
  size_t i = 0;
  int n_k = 0;
  bool miss = false;
  if (active) {
    i = (size_t)O.pos;
    n_k = O.n_k;
    if (lane < n_k) {
      const Vec3 p = {O.p[lane][0], O.p[lane][1], O.p[lane][2]};
      ExtentPasses X;
      bool spread_any;
      double pv[kMaxPanOut];
      int n_pv;
      if (pan_prepare(P, p, may_spread, width ? width[i] : 0.0, height ? height[i] : 0.0, depth ? depth[i] : 0.0, X, spread_any,
                      pv, n_pv))
        extent_job_fill(sub[wave][lane], (int)i, p, X, pv, n_pv);
      else
        miss = true;
    }
  }
  __syncthreads();
  if (!active) return;
  if (__ballot(miss) != 0) {  // a position no region took: the object's rows are zero and it counts once
    if (lane < P.n_full) direct[i * P.n_full + lane] = diff[i * P.n_full + lane] = 0.0f;
    if (lane == 0) atomicAdd(missed, 1u);
    return;
  }
  double power = 0.0;
  for (int k = 0; k < n_k; k++) {
    const double fin = extent_render(E, sub[wave][k], lane);
    power += O.w[k] * (fin * fin);
  }
  // the power of an excluded output goes, in equal parts, to what is left of its nearest group that has anything left
  const unsigned em = O.excluded;
  double out = lane < kObjMaxOut && (em >> lane & 1u) ? 0.0 : power;
  for (unsigned m = em; m; m &= m - 1) {
    const int c = __ffs((int)m) - 1;
    unsigned to = 0;
    for (int g = 0; g < Z.n && to == 0; g++) to = Z.groups[c][g] & ~em;
    const double share = __shfl(power, c) / (double)__popc(to);
    if (lane < kObjMaxOut && (to >> lane & 1u)) out += share;
  }
  extent_write(P, sqrt(out), i, lane, gain, diffuse, direct, diff);
}

}  // namespace earhip
