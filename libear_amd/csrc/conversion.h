// conversion.h — the ITU-R BS.2127 §10 conversion of Objects positions and extents between polar and Cartesian
// (earhip group K; libear src/conversion.cpp:14-281 with src/common/geom.{hpp,cpp}), as __host__ __device__
// double-precision code shared by the host forms and the device kernel of api_conversion.hip.  Arithmetic and
// operation order are libear's; the Makefile builds with -ffp-contract=off, so no FMA is formed.
//
// One difference from libear, in the angle reductions of insideAngleRange / relativeAngle: libear subtracts or
// adds 360 in while loops, which never end for an infinite azimuth and in practice not for a huge one.  Here
// the reduction starts from fmod(x, 360), which is exact, and finishes with at most a few steps of 360.  Every
// step of libear's loops is exact wherever they end, so the two give the same value there (the sign of a zero
// included).  A polar azimuth that is infinite or beyond +-2^40 is refused with EARHIP_INVALID_ARGUMENT.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/earhip.h"

namespace earhip {
namespace conv {

// boost::math::constants::pi<double>() and the constants libear derives from it (src/common/geom.hpp:12-20)
constexpr double kPi = 3.141592653589793238462643383279502884;
constexpr double kRad = kPi / 180.0;
constexpr double kDeg = 180.0 / kPi;
constexpr double kElTop = 30.0, kElTopTilde = 45.0;  // conversion.cpp:80-81
constexpr double kMaxAzimuth = 1099511627776.0;      // 2^40: larger polar azimuths are refused

// One sector of the azimuth mapping (conversion.cpp:27-39), from the mapping points 0, -30, -110, 110, 30
// degrees at (0, 1), (1, 1), (1, -1), (-1, -1), (-1, 1).  cart_*_az is libear's azimuth() of the Cartesian
// points, m the inverse of the matrix whose rows are the two points: every entry is exact (0, +-0.5, +-1; the
// signs of the zeros are those of Eigen's 2x2 inverse).
struct Sector {
  double polar_start_az, polar_end_az, cart_start_az, cart_end_az;
  double cart_start[2], cart_end[2];
  double m[2][2];
};

#define EARHIP_CONV_SECTORS                                                    \
  {{0.0, -30.0, -0.0, -45.0, {0.0, 1.0}, {1.0, 1.0}, {{-1.0, 1.0}, {1.0, -0.0}}},   \
   {-30.0, -110.0, -45.0, -135.0, {1.0, 1.0}, {1.0, -1.0}, {{0.5, 0.5}, {0.5, -0.5}}}, \
   {-110.0, 110.0, -135.0, 135.0, {1.0, -1.0}, {-1.0, -1.0}, {{0.5, -0.5}, {-0.5, -0.5}}}, \
   {110.0, 30.0, 135.0, 45.0, {-1.0, -1.0}, {-1.0, 1.0}, {{-0.5, -0.5}, {-0.5, 0.5}}},  \
   {30.0, 0.0, 45.0, -0.0, {-1.0, 1.0}, {0.0, 1.0}, {{-1.0, 1.0}, {0.0, 1.0}}}}

constexpr int kNumSectors = 5;
static __constant__ Sector d_sectors[kNumSectors] = EARHIP_CONV_SECTORS;  // (static: one per unit that includes this)
static const Sector h_sectors[kNumSectors] = EARHIP_CONV_SECTORS;

__host__ __device__ inline const Sector &sector(int i) {
#ifdef __HIP_DEVICE_COMPILE__
  return d_sectors[i];
#else
  return h_sectors[i];
#endif
}

__host__ __device__ inline double radians(double d) { return d * kRad; }
__host__ __device__ inline double degrees(double r) { return r * kDeg; }
__host__ __device__ inline double sign(double x) { return x < 0.0 ? -1.0 : (x > 0.0 ? 1.0 : 0.0); }
// std::max(a, b) and std::max({a, b, c}): the first argument wins ties and NaN comparisons
__host__ __device__ inline double max2(double a, double b) { return a < b ? b : a; }
__host__ __device__ inline double max3(double a, double b, double c) { return max2(max2(a, b), c); }

// The value libear's loops `while (x - 360 >= lo) x -= 360; while (x < lo) x += 360;` reach, for |lo| <= 360:
// x - 360k in [lo, lo + 360).  fmod is exact, and the steps after it are the last of libear's steps.  A zero
// that libear reaches by a step is +0.
__host__ __device__ inline double reduce_angle(double x, double lo) {
  double r = fmod(x, 360.0);
  if (r == 0.0 && x != 0.0) r = 0.0;
  for (int i = 0; i < 2 && r - 360.0 >= lo; i++) r -= 360.0;
  for (int i = 0; i < 2 && r < lo; i++) r += 360.0;
  return r;
}

// y moved by whole turns to [x, x + 360) (src/common/geom.hpp:31-39)
__host__ __device__ inline double relative_angle(double x, double y) { return reduce_angle(y, x); }

// is x within [start, end], end clockwise from start, tolerance 0 (src/common/geom.cpp:7-28).  end is reduced
// to (start, start + 360] as libear's `while (end - 360 > start)` / `while (end < start)` leave it.
__host__ __device__ inline bool inside_angle_range(double x, double start, double end) {
  for (int i = 0; i < 2 && end - 360.0 > start; i++) end -= 360.0;
  for (int i = 0; i < 2 && end < start; i++) end += 360.0;
  return reduce_angle(x, start) <= end;
}

// azimuth of (x, y, .) (src/common/geom.cpp:71-73)
__host__ __device__ inline double azimuth(double x, double y) { return -degrees(atan2(x, y)); }

// cart(az, el, 1) (src/common/geom.cpp:82-87): a row of libear's localCoordinateSystem
__host__ __device__ inline void cart1(double az, double el, double v[3]) {
  v[0] = sin(radians(-az)) * cos(radians(el)) * 1.0;
  v[1] = cos(radians(-az)) * cos(radians(el)) * 1.0;
  v[2] = sin(radians(el)) * 1.0;
}

// localCoordinateSystem(az, el) (src/common/geom.hpp:91-98): rows az - 90 / el 0, az / el, az / el + 90
__host__ __device__ inline void local_coordinate_system(double az, double el, double lcs[3][3]) {
  cart1(az - 90.0, 0.0, lcs[0]);
  cart1(az, el, lcs[1]);
  cart1(az, el + 90.0, lcs[2]);
}

__host__ __device__ inline double norm3(double a, double b, double c) { return sqrt(a * a + b * b + c * c); }

// conversion.cpp:94-119
__host__ __device__ inline double map_az_to_linear(double left_az, double right_az, double az) {
  const double mid_az = (left_az + right_az) / 2.0;
  const double az_range = right_az - mid_az;
  const double rel_az = az - mid_az;
  const double gain_r = 0.5 + 0.5 * tan(radians(rel_az)) / tan(radians(az_range));
  return atan2(gain_r, 1.0 - gain_r) * (2.0 / kPi);
}

__host__ __device__ inline double map_linear_to_az(double left_az, double right_az, double x) {
  const double mid_az = (left_az + right_az) / 2.0;
  const double az_range = right_az - mid_az;
  const double gain_l_ = cos(x * (kPi / 2.0));
  const double gain_r_ = sin(x * (kPi / 2.0));
  const double gain_r = gain_r_ / (gain_l_ + gain_r_);
  const double rel_az = degrees(atan(2.0 * (gain_r - 0.5) * tan(radians(az_range))));
  return mid_az + rel_az;
}

// pointPolarToCart (conversion.cpp:123-153).  Returns EARHIP_OK, EARHIP_INVALID_ARGUMENT (an infinite azimuth
// or one beyond +-2^40: libear does not return), or EARHIP_INTERNAL_ERROR (no sector, e.g. a NaN azimuth:
// libear throws internal_error; p outside [-1e-6, 1 + 1e-6]: libear's ear_assert fails).
__host__ __device__ inline int point_polar_to_cart(double az, double el, double dist, double out[3]) {
  if (fabs(az) > kMaxAzimuth) return EARHIP_INVALID_ARGUMENT;  // +-inf included, NaN not
  double r_xy, z;
  if (fabs(el) > kElTop) {
    const double el_tilde = kElTopTilde + (90.0 - kElTopTilde) * (fabs(el) - kElTop) / (90.0 - kElTop);
    z = dist * sign(el);
    r_xy = dist * tan(radians(90.0 - el_tilde));
  } else {
    const double el_tilde = kElTopTilde * el / kElTop;
    z = tan(radians(el_tilde)) * dist;
    r_xy = dist;
  }
  int s = 0;
  while (s < kNumSectors && !inside_angle_range(az, sector(s).polar_end_az, sector(s).polar_start_az)) s++;
  if (s == kNumSectors) return EARHIP_INTERNAL_ERROR;
  const Sector &sec = sector(s);
  const double rel_az = relative_angle(sec.polar_end_az, az);
  const double rel_left_az = relative_angle(sec.polar_end_az, sec.polar_start_az);
  const double p = map_az_to_linear(rel_left_az, sec.polar_end_az, rel_az);
  if (!(-1e-6 <= p && p <= 1.0 + 1e-6)) return EARHIP_INTERNAL_ERROR;
  for (int i = 0; i < 2; i++) out[i] = r_xy * (sec.cart_start[i] + (sec.cart_end[i] - sec.cart_start[i]) * p);
  out[2] = z;
  return EARHIP_OK;
}

// pointCartToPolar (conversion.cpp:155-193).  EARHIP_INTERNAL_ERROR: no sector (a NaN coordinate).
__host__ __device__ inline int point_cart_to_polar(double x, double y, double z, double out[3]) {
  const double eps = 1e-10;
  if (fabs(x) < eps && fabs(y) < eps) {
    if (fabs(z) < eps) {
      out[0] = 0.0, out[1] = 0.0, out[2] = 0.0;
    } else {
      out[0] = 0.0, out[1] = sign(z) * 90.0, out[2] = fabs(z);
    }
    return EARHIP_OK;
  }
  const double cart_az = azimuth(x, y);
  int s = 0;
  while (s < kNumSectors && !inside_angle_range(cart_az, sector(s).cart_end_az, sector(s).cart_start_az)) s++;
  if (s == kNumSectors) return EARHIP_INTERNAL_ERROR;
  const Sector &sec = sector(s);
  // RowVector2d{x, y} * m
  const double g_l = x * sec.m[0][0] + y * sec.m[1][0];
  const double g_r = x * sec.m[0][1] + y * sec.m[1][1];
  const double r_xy = g_l + g_r;
  const double rel_left_az = relative_angle(sec.polar_end_az, sec.polar_start_az);
  double az = map_linear_to_az(rel_left_az, sec.polar_end_az, g_r / r_xy);
  az = relative_angle(-180.0, az);
  const double el_tilde = degrees(atan(z / r_xy));
  double d, el;
  if (fabs(el_tilde) > kElTopTilde) {
    const double abs_el = kElTop + (90.0 - kElTop) * (fabs(el_tilde) - kElTopTilde) / (90.0 - kElTopTilde);
    el = sign(el_tilde) * abs_el;
    d = fabs(z);
  } else {
    el = kElTop * el_tilde / kElTopTilde;
    d = r_xy;
  }
  out[0] = az, out[1] = el, out[2] = d;
  return EARHIP_OK;
}

// whd2xyz (conversion.cpp:197-213): polar width, height, depth -> x, y, z sizes in the source's frame
__host__ __device__ inline void whd2xyz(double width, double height, double depth, double xyz[3]) {
  const double x_size_width = width < 180.0 ? sin(radians(width / 2.0)) : 1.0;
  const double y_size_width = (1.0 - cos(radians(width / 2.0))) / 2.0;
  const double z_size_height = height < 180.0 ? sin(radians(height / 2.0)) : 1.0;
  const double y_size_height = (1.0 - cos(radians(height / 2.0))) / 2.0;
  xyz[0] = x_size_width;
  xyz[1] = max3(y_size_width, y_size_height, depth);
  xyz[2] = z_size_height;
}

// xyz2whd (conversion.cpp:215-236)
__host__ __device__ inline void xyz2whd(double s_x, double s_y, double s_z, double whd[3]) {
  const double width_from_sx = 2.0 * degrees(asin(s_x));
  const double width_from_sy = 2.0 * degrees(acos(1.0 - 2.0 * s_y));
  const double width = width_from_sx + s_x * max2(width_from_sy - width_from_sx, 0.0);
  const double height_from_sz = 2.0 * degrees(asin(s_z));
  const double height_from_sy = 2.0 * degrees(acos(1.0 - 2.0 * s_y));
  const double height = height_from_sz + s_z * max2(height_from_sy - height_from_sz, 0.0);
  double equiv[3];
  whd2xyz(width, height, 0.0, equiv);
  whd[0] = width, whd[1] = height, whd[2] = max2(0.0, s_y - equiv[1]);
}

// the extent half of extentPolarToCart (conversion.cpp:254-266): polar (width, height, depth) at (az, el) ->
// Cartesian (width, height, depth)
__host__ __device__ inline void extent_polar_to_cart(double az, double el, const double whd[3], double out[3]) {
  double front[3], lcs[3][3];
  whd2xyz(whd[0], whd[1], whd[2], front);
  local_coordinate_system(az, el, lcs);
  // M = LCS.colwise() * front_size; size = M.colwise().norm()
  double size[3];
  for (int j = 0; j < 3; j++) size[j] = norm3(lcs[0][j] * front[0], lcs[1][j] * front[1], lcs[2][j] * front[2]);
  out[0] = size[0], out[1] = size[2], out[2] = size[1];
}

// the extent half of extentCartToPolar (conversion.cpp:238-252), at the converted polar position (az, el)
__host__ __device__ inline void extent_cart_to_polar(double az, double el, const double whd[3], double out[3]) {
  const double e[3] = {whd[0], whd[2], whd[1]};  // (width, depth, height): x, y, z sizes
  double lcs[3][3];
  local_coordinate_system(az, el, lcs);
  // M = LCS.transpose().colwise() * extent_vec; column j of M is row j of LCS scaled per component
  double s[3];
  for (int j = 0; j < 3; j++) s[j] = norm3(lcs[j][0] * e[0], lcs[j][1] * e[1], lcs[j][2] * e[2]);
  xyz2whd(s[0], s[1], s[2], out);
}

}  // namespace conv
}  // namespace earhip
