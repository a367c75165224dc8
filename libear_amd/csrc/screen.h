// screen.h — screenRef scaling and screenEdgeLock of an Objects position (earhip group R; ITU-R BS.2127-0 sections 7.3.3 and
// 7.3.4; libear refuses both), as __host__ __device__ double-precision code shared by the host form and the device kernel of
// api_screen.hip.  Per element there is an exact fmod, comparisons, one subtraction and one explicit fma: no other libm call
// and (the Makefile builds with -ffp-contract=off) no contraction the code does not spell out, so the host form and the kernel
// give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace earhip {
namespace screen {

constexpr double kMaxAzimuth = 1099511627776.0;  // 2^40, the bound of group K

// one piece of a piecewise-linear map: y = fma(slope, x - x0, y0) for x from x0 up to the next piece's x0
struct Segment {
  double x0, y0, slope;
};

// What one call applies to every element: the azimuth map through (-180, ref.right, ref.left, 180) -> (-180, rep.right,
// rep.left, 180), the elevation map through (-90, ref.bottom, ref.top, 90) -> (-90, rep.bottom, rep.top, 90), and the
// reproduction screen's edges for the lock.  identity: no reproduction screen, every element is copied.
struct Map {
  Segment az[3], el[3];
  double left, right, bottom, top;
  int identity;
};

// the three segments through (x[0], y[0]) .. (x[3], y[3]); x strictly increasing
__host__ __device__ inline void fill_segments(const double x[4], const double y[4], Segment s[3]) {
  for (int k = 0; k < 3; k++) s[k] = Segment{x[k], y[k], (y[k + 1] - y[k]) / (x[k + 1] - x[k])};
}

// edges: left azimuth, right azimuth, bottom elevation, top elevation (earhip_screen_edges), each checked by the caller
__host__ __device__ inline Map make_map(const double ref[4], const double rep[4]) {
  Map m;
  const double ax[4] = {-180.0, ref[1], ref[0], 180.0}, ay[4] = {-180.0, rep[1], rep[0], 180.0};
  const double ex[4] = {-90.0, ref[2], ref[3], 90.0}, ey[4] = {-90.0, rep[2], rep[3], 90.0};
  fill_segments(ax, ay, m.az);
  fill_segments(ex, ey, m.el);
  m.left = rep[0], m.right = rep[1], m.bottom = rep[2], m.top = rep[3];
  m.identity = 0;
  return m;
}

__host__ __device__ inline Map identity_map() {
  Map m = Map();
  m.identity = 1;
  return m;
}

// the segment whose x0 is the largest breakpoint <= x (x at or above the first breakpoint)
__host__ __device__ inline int segment_of(const Segment s[3], double x) { return x >= s[2].x0 ? 2 : (x >= s[1].x0 ? 1 : 0); }

// the map's value at x in [s[0].x0, hi]; x >= hi gives exactly hi (the seam and the poles map to themselves)
__host__ __device__ inline double map_value(const Segment s[3], double hi, double x) {
  if (x >= hi) return hi;
  const Segment &g = s[segment_of(s, x)];
  return fma(g.slope, x - g.x0, g.y0);
}

// azimuth moved by whole turns into [-180, 180]: fmod is exact, and so is the one step that follows it
__host__ __device__ inline double reduce_azimuth(double az) {
  double a = fmod(az, 360.0);
  if (a > 180.0) a -= 360.0;
  if (a < -180.0) a += 360.0;
  return a;
}

// One element.  Returns 0 and the new position, or 1 for an element that is refused (a non-finite azimuth or elevation,
// |azimuth| > 2^40, |elevation| > 90, a lock code above 2), whose outputs are then the inputs.  An element with no flag set
// is not looked at: its bits pass through, whatever they are.
__host__ __device__ inline int apply_one(const Map &m, double az, double el, unsigned screen_ref, unsigned lock_h,
                                         unsigned lock_v, double &az_out, double &el_out) {
  az_out = az, el_out = el;
  if (m.identity || (screen_ref == 0 && lock_h == 0 && lock_v == 0)) return 0;
  // (the comparisons are false for a NaN)
  if (!(fabs(az) <= kMaxAzimuth) || !(fabs(el) <= 90.0) || lock_h > 2 || lock_v > 2) return 1;
  if (screen_ref != 0) {
    az_out = map_value(m.az, 180.0, reduce_azimuth(az));
    el_out = map_value(m.el, 90.0, el);
  }
  if (lock_h != 0) az_out = lock_h == 1 ? m.left : m.right;
  if (lock_v != 0) el_out = lock_v == 1 ? m.bottom : m.top;
  return 0;
}

}  // namespace screen
}  // namespace earhip
