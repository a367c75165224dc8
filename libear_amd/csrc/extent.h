// extent.h — the plain part of libear's polar extent panner (src/object_based/polar_extent.cpp:12-302, core:
// src/object_based/polar_extent_scalar.cpp:25-108): what is scalar set-up per position in libear, the weight of a grid
// point, the classification of a chunk of grid points against an extent, and the geometry of the point grid.  Plain
// C++: hipcc compiles it for the host and the device (the kernels are extent_kernels.h, the grid's gains
// api_panner.hip), g++ for the host alone (tests/cpp/extent_host.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "panner.h"

namespace earhip {

constexpr int kExtentMaxChunks = 32;
constexpr int kExtentRows = 37;          // polar_extent.cpp:14
constexpr double kExtentFade = 10.0;     // :13

// eigen_helpers.hpp:26-48 for 2, 3 and 4 points
EARHIP_PAN_HD inline double ext_interp(double x, const double *xp, const double *yp, int n) {
  if (x <= xp[0]) return yp[0];
  for (int i = 0; i + 1 < n; i++)
    if (xp[i + 1] > x) return yp[i] + (yp[i + 1] - yp[i]) / (xp[i + 1] - xp[i]) * (x - xp[i]);
  return yp[n - 1];
}
EARHIP_PAN_HD inline double ext_degrees(double r) { return r * 180.0 / 3.14159265358979323846264338327950288; }
EARHIP_PAN_HD inline double ext_radians(double d) { return d * 3.14159265358979323846264338327950288 / 180.0; }

// polar_extent.cpp:62-70
EARHIP_PAN_HD inline double extent_mod(double extent, double distance) {
  const double x2[2] = {0.0, 360.0}, y2[2] = {0.2, 1.0};
  const double size = ext_interp(extent, x2, y2, 2);
  const double extent1 = 4.0 * ext_degrees(atan2(size, 1.0));
  const double x3[3] = {0.0, extent1, 360.0}, y3[3] = {0.0, extent, 360.0};
  return ext_interp(4.0 * ext_degrees(atan2(size, distance)), x3, y3, 3);
}

// PolarExtent::handle's renderings (:290-302): one, or with depth a near and a far one; per rendering the
// distance-modified width and height and the share of the spread part (:263-266)
struct ExtentPasses {
  int n_pass;
  double w[2], h[2], spread[2];
};
EARHIP_PAN_HD inline void extent_passes(Vec3 p, double w0, double h0, double dp, ExtentPasses &X) {
  const double distance = sqrt(p.x * p.x + p.y * p.y + p.z * p.z);
  X.n_pass = dp != 0.0 ? 2 : 1;
  for (int k = 0; k < 2; k++) {
    double d = distance;
    if (X.n_pass == 2) d = fmax(k == 0 ? distance - dp / 2.0 : distance + dp / 2.0, 0.0);
    X.w[k] = extent_mod(w0, d);
    X.h[k] = extent_mod(h0, d);
    const double x2[2] = {0.0, kExtentFade}, y2[2] = {0.0, 1.0};
    X.spread[k] = ext_interp(fmax(X.w[k], X.h[k]), x2, y2, 2);
  }
}

// what the core needs per call (PolarExtentCoreContext, polar_extent_core.hpp:30-42)
struct ExtentWeighting {
  bool is_circular;
  float basis[9], circle_test[2], right_circle_centre[2];
  float cos_start, cos_end, sin_start, sin_end, m, c;
  // every point further than r_out from the object's direction weighs 0, every point closer than r_in weighs 1
  // (radians; r_out = half the larger dimension after its modification + fade, r_in = half the smaller one)
  float r_in, r_out;
};

// setup_weighting_function + setup_angle_to_weight (polar_extent.cpp:186-255); calcBasis (:80-91)
EARHIP_PAN_HD inline void extent_setup(Vec3 position, double width, double height, ExtentWeighting &W) {
  const double pi = 3.14159265358979323846264338327950288;
  width = ext_radians(width) / 2;
  height = ext_radians(height) / 2;
  const double n = sqrt(position.x * position.x + position.y * position.y + position.z * position.z);
  const Vec3 u = n < 1e-10 ? Vec3{0.0, 1.0, 0.0} : Vec3{position.x / n, position.y / n, position.z / n};
  double az = -ext_degrees(atan2(u.x, u.y));
  const double el = ext_degrees(atan2(u.z, hypot(u.x, u.y)));
  if (fabs(el) > 90.0 - 1e-5) az = 0.0;  // near the poles the azimuth is indeterminate
  // rows along x, y, z of a frame whose +y points at the object (geom.hpp:91-98)
  Vec3 r0 = polar_to_cart(az - 90.0, 0.0, 1.0), r1 = polar_to_cart(az, el, 1.0), r2 = polar_to_cart(az, el + 90.0, 1.0);
  if (height > width) {  // wider than high from here on: the frame rotated about the object's direction
    const double t = height;
    height = width;
    width = t;
    const Vec3 old0 = r0;
    r0 = r2;
    r2 = {-old0.x, -old0.y, -old0.z};
  }
  W.basis[0] = (float)r0.x, W.basis[1] = (float)r0.y, W.basis[2] = (float)r0.z;
  W.basis[3] = (float)r1.x, W.basis[4] = (float)r1.y, W.basis[5] = (float)r1.z;
  W.basis[6] = (float)r2.x, W.basis[7] = (float)r2.y, W.basis[8] = (float)r2.z;
  // the ends of a wide extent meet at the back (:236-242)
  const double width_full = pi + height;
  const double x3[3] = {0.0, pi / 2.0, pi}, y3[3] = {0.0, pi / 2.0, width_full};
  const double width_mod = ext_interp(width, x3, y3, 3);
  const double x4[4] = {0.0, pi / 4.0, pi / 2.0, pi}, y4[4] = {width_mod, width_mod, width, width};
  width = ext_interp(height, x4, y4, 4);
  W.is_circular = (width - height) < 1e-6;
  const double circle_pos = width - height;
  W.right_circle_centre[0] = (float)sin(circle_pos);
  W.right_circle_centre[1] = (float)cos(circle_pos);
  W.circle_test[0] = (float)-cos(circle_pos);
  W.circle_test[1] = (float)sin(circle_pos);
  const double start_angle = height, end_angle = height + ext_radians(kExtentFade);
  W.cos_start = (float)(start_angle < pi ? cos(start_angle) : -1.0);
  W.cos_end = (float)(end_angle < pi ? cos(end_angle) : -(1.0 + 1e-6));
  W.sin_start = (float)(start_angle < pi / 2 ? sin(start_angle) : 1.0);
  W.sin_end = (float)(end_angle < pi / 2 ? sin(end_angle) : 1.0 + 1e-6);
  W.m = (float)(1.0 / (start_angle - end_angle));
  W.c = (float)(-W.m * end_angle);
  W.r_in = (float)start_angle;
  W.r_out = (float)(width + ext_radians(kExtentFade));
}

// polar_extent_scalar.cpp:34-76 (float)
EARHIP_PAN_HD inline float extent_weight(const ExtentWeighting &W, float x, float y, float z) {
  auto from_cos = [&](float ca) { return ca >= W.cos_start ? 1.0f : ca <= W.cos_end ? 0.0f : W.m * acosf(ca) + W.c; };
  auto from_sin = [&](float sa) { return sa <= W.sin_start ? 1.0f : sa >= W.sin_end ? 0.0f : W.m * asinf(sa) + W.c; };
  const float ty = x * W.basis[3] + y * W.basis[4] + z * W.basis[5];
  if (W.is_circular) return from_cos(ty);
  const float tx = x * W.basis[0] + y * W.basis[1] + z * W.basis[2];
  const float tz = x * W.basis[6] + y * W.basis[7] + z * W.basis[8];
  const float rx = fabsf(tx);
  if (rx * W.circle_test[0] + ty * W.circle_test[1] >= 0.0f) return from_sin(fabsf(tz));
  return from_cos(rx * W.right_circle_centre[0] + ty * W.right_circle_centre[1]);
}

// A chunk of grid points — all within chunk_rad of a direction at chunk_angle from the object's (radians) — against
// an extent: every point weighs 0, every point weighs 1, or neither is known and the points are weighed one by one.
enum ExtentChunkClass { kExtentChunkEdge = 0, kExtentChunkOutside = 1, kExtentChunkInside = 2 };
constexpr float kExtentChunkMargin = 1e-3f;  // (radians: float rounding of the angles and of the weights' own thresholds)
EARHIP_PAN_HD inline ExtentChunkClass extent_chunk_class(const ExtentWeighting &W, float chunk_angle, float chunk_rad) {
  if (chunk_angle - chunk_rad > W.r_out + kExtentChunkMargin) return kExtentChunkOutside;
  if (chunk_angle + chunk_rad + kExtentChunkMargin < W.r_in) return kExtentChunkInside;
  return kExtentChunkEdge;
}

// PolarExtent's point grid (polar_extent.cpp:16-50): 37 rows of points, 5 degrees apart, stored in spatially compact
// chunks of 64 with, per chunk, the unit mean direction of its points (float) and the largest angle between that and a
// point of the chunk
struct ExtentGrid {
  std::vector<Vec3> points;      // [n_points], chunk after chunk
  size_t n_padded, n_chunks;     // n_points rounded up to whole chunks
  std::vector<float> chunk_dir;  // [3][n_chunks]
  std::vector<float> chunk_rad;  // [n_chunks] (radians)
};
inline ExtentGrid extent_grid() {
  const double pi = 3.14159265358979323846264338327950288;
  struct GridPoint {
    Vec3 v;
    int band;
    double az;
    int row;
  };
  std::vector<GridPoint> grid;
  for (int r = 0; r < kExtentRows; r++) {
    const double el = -90.0 + r * (180.0 / (kExtentRows - 1));
    const double radius = std::cos(el * pi / 180.0);
    int n_points = (int)std::round(((2 * pi * radius) / (2 * pi)) * 2 * (kExtentRows - 1));
    if (n_points == 0) n_points = 1;
    for (int i = 0; i < n_points; i++) {
      const double az = i * (360.0 / n_points);
      grid.push_back({polar_to_cart(az, el, 1.0), r / 8, az, r});
    }
  }
  // The device kernel classifies CHUNKS of 64 points against an extent, so a chunk should be a compact patch:
  // bands of 8 rows (40 degrees), each walked along the azimuth.  (The order of the points only changes the
  // order of the float additions; libear's is row by row.)
  std::stable_sort(grid.begin(), grid.end(), [](const GridPoint &a, const GridPoint &b) {
    if (a.band != b.band) return a.band < b.band;
    if (a.az != b.az) return a.az < b.az;
    return a.row < b.row;
  });
  ExtentGrid G;
  const size_t np = grid.size();
  G.n_padded = (np + 63) / 64 * 64;
  G.n_chunks = G.n_padded / 64;
  for (const GridPoint &g : grid) G.points.push_back(g.v);
  G.chunk_dir.assign(3 * G.n_chunks, 0.0f);
  G.chunk_rad.assign(G.n_chunks, 0.0f);
  for (size_t c = 0; c < G.n_chunks; c++) {
    const size_t lo = 64 * c, hi = std::min(lo + 64, np);
    Vec3 m = {0.0, 0.0, 0.0};
    for (size_t q = lo; q < hi; q++) m = vadd(m, G.points[q]);
    double n = std::sqrt(vdot(m, m));
    if (n < 1e-6) m = G.points[lo], n = 1.0;
    // (the kernel works with the float direction: measure the radius around that)
    const float fx = (float)(m.x / n), fy = (float)(m.y / n), fz = (float)(m.z / n);
    const double fn = std::sqrt((double)fx * fx + (double)fy * fy + (double)fz * fz);
    double worst = 0.0;
    for (size_t q = lo; q < hi; q++) {
      const double cs = (G.points[q].x * fx + G.points[q].y * fy + G.points[q].z * fz) / fn;
      worst = std::max(worst, std::acos(std::min(1.0, std::max(-1.0, cs))));
    }
    G.chunk_dir[c] = fx, G.chunk_dir[G.n_chunks + c] = fy, G.chunk_dir[2 * G.n_chunks + c] = fz;
    G.chunk_rad[c] = (float)(worst + 1e-4);
  }
  return G;
}

}  // namespace earhip
