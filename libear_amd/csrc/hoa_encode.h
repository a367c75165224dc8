// hoa_encode.h — real spherical harmonics in libear's conventions (src/hoa/hoa.hpp:16-112: associated Legendre functions
// without the Condon-Shortley phase, N3D / SN3D / FuMa norms, sqrt2 cos / -sqrt2 sin azimuth factors) as __host__ __device__
// double-precision code: the decoder's harmonics (earhip_hoa_decode_matrix, api_hoa.hip) and the encoder of earhip group Q (api_hoa.hip), whose host
// form and device kernel run the one core below.  The Makefile builds with -ffp-contract=off, so no FMA is formed and the two
// differ only in the math library behind sin, cos, sqrt and fmod.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"

namespace earhip {
namespace hoa {

constexpr int kMaxCoef = 64;  // channels of an encoder call
constexpr int kMaxOrder = 7;
constexpr double kPi = 3.141592653589793238462643383279502884;
constexpr double kRad = kPi / 180.0;
constexpr double kSqrt2 = 1.41421356237309504880168872420969808;  // == std::sqrt(2.0)

__host__ __device__ inline double factorial_d(int n) {
  double f = 1.0;
  for (int i = 2; i <= n; i++) f *= i;
  return f;
}

// associated Legendre function P_n^m(x) without the Condon-Shortley phase, upward recurrence in n
__host__ __device__ inline double legendre_nm(int n, int m, double x) {
  const double root = sqrt((1.0 - x) * (1.0 + x));
  double p0 = 1.0;
  for (int i = 1; i <= m; i++) p0 *= (2.0 * i - 1.0) * root;  // P_m^m
  if (n == m) return p0;
  double p1 = x * (2.0 * m + 1.0) * p0;                         // P_(m+1)^m
  for (int l = m + 2; l <= n; l++) {
    const double p2 = (x * (2.0 * l - 1.0) * p1 - (l + m - 1.0) * p0) / (l - m);
    p0 = p1;
    p1 = p2;
  }
  return p1;
}

enum HoaNorm { kN3D, kSN3D, kFuMa };
inline double hoa_norm(HoaNorm t, int n, int am) {
  const double sn3d = std::sqrt(factorial_d(n - am) / factorial_d(n + am));
  if (t == kSN3D) return sn3d;
  if (t == kN3D) return std::sqrt(2.0 * n + 1.0) * sn3d;
  // FuMa: defined up to order 3 (hoa.hpp:56-72)
  static const double f[4][4] = {{0.70710678118654752440, 0, 0, 0},
                                 {1.0, 1.0, 0, 0},
                                 {1.0, 1.15470053837925152902, 1.15470053837925152902, 0},
                                 {1.0, 1.18585412256314232322, 1.34164078649987381784, 1.26491106406735172760}};
  if (n > 3) fail_invalid("FuMa normalisation is defined up to order 3");
  return f[n][am] * sn3d;
}

// ---- the encoder (include/earhip.h group Q): out[c] = (float)(gain * K * P_n^|m|(x) * T_m(r)), left to right
struct Channel {
  double k;           // K(n, |m|) of the call's normalization
  signed char n, m;
};
// a call's channels, prepared on the host and passed to the kernel by value.  walk: the channel indices sorted by (|m|, n),
// the order in which encode_position's recurrences reach them.
struct Table {
  int n_coef;
  Channel ch[kMaxCoef];
  unsigned char walk[kMaxCoef];
};

// the table of a checked channel list (host; no allocation)
inline void fill_table(Table &t, int n_coef, const int *orders, const int *degrees, HoaNorm norm) {
  std::memset(&t, 0, sizeof t);
  t.n_coef = n_coef;
  for (int c = 0; c < n_coef; c++) {
    t.ch[c].k = hoa_norm(norm, orders[c], std::abs(degrees[c]));  // (refuses FuMa above order 3)
    t.ch[c].n = (signed char)orders[c];
    t.ch[c].m = (signed char)degrees[c];
    t.walk[c] = (unsigned char)c;
  }
  std::stable_sort(t.walk, t.walk + n_coef, [&](unsigned char a, unsigned char b) {
    return std::abs((int)t.ch[a].m) * 8 + t.ch[a].n < std::abs((int)t.ch[b].m) * 8 + t.ch[b].n;
  });
}

// what the host form refuses and the device form marks
__host__ __device__ inline bool encode_valid(double az, double el, double gain) {
  const double big = 1.7976931348623157e308;  // (a comparison is false for NaN)
  return fabs(az) <= big && fabs(gain) <= big && fabs(el) <= 90.0;
}

__host__ __device__ inline double azimuth_factor(int m, double cos_mr, double sin_mr) {
  return m > 0 ? kSqrt2 * cos_mr : (m < 0 ? -kSqrt2 * sin_mr : 1.0);
}

// One position, every channel of the table: emit(c, value) once per channel, in walk order.  x = sin(elevation), r = the
// azimuth in radians.  Per |m| the sectoral term P_m^m grows by one factor, cos(m r) and sin(-m r) are taken once, and the
// recurrence in n runs once, as far as the table's highest order of that |m|: every value is the one legendre_nm and the
// factors above give for that channel alone, operation for operation.
template <typename Emit>
__host__ __device__ inline void encode_position_rad(const Table &t, double r, double x, double gain, Emit emit) {
  const double root = sqrt((1.0 - x) * (1.0 + x));
  double pmm = 1.0;
  int w = 0;
  for (int am = 0; am <= kMaxOrder && w < t.n_coef; am++) {
    if (am > 0) pmm *= (2.0 * am - 1.0) * root;  // P_am^am
    if (abs((int)t.ch[t.walk[w]].m) != am) continue;
    const double cos_mr = am ? cos((double)am * r) : 1.0;
    const double sin_mr = am ? sin((double)(-am) * r) : 0.0;  // of m r for the negative m
    double p0 = pmm, p1 = pmm;
    for (int n = am; n <= kMaxOrder; n++) {
      if (n == am + 1) {
        p1 = x * (2.0 * am + 1.0) * p0;
      } else if (n > am + 1) {
        const double p2 = (x * (2.0 * n - 1.0) * p1 - (n + am - 1.0) * p0) / (n - am);
        p0 = p1;
        p1 = p2;
      }
      while (w < t.n_coef && t.ch[t.walk[w]].n == n && abs((int)t.ch[t.walk[w]].m) == am) {
        const int c = t.walk[w++];
        emit(c, gain * t.ch[c].k * p1 * azimuth_factor(t.ch[c].m, cos_mr, sin_mr));
      }
      if (w == t.n_coef || abs((int)t.ch[t.walk[w]].m) != am) break;
    }
  }
}

// degrees in: the azimuth reduced by an exact fmod before the conversion to radians
template <typename Emit>
__host__ __device__ inline void encode_position(const Table &t, double az, double el, double gain, Emit emit) {
  encode_position_rad(t, fmod(az, 360.0) * kRad, sin(el * kRad), gain, emit);
}

// one channel of one position, on its own: the same value, bit for bit (tests/cpp/test_hoa_core.cpp)
__host__ __device__ inline double encode_one(const Channel &c, double az, double el, double gain) {
  const double r = fmod(az, 360.0) * kRad, x = sin(el * kRad);
  const int m = c.m, am = m < 0 ? -m : m;
  const double mr = (double)m * r;
  return gain * c.k * legendre_nm(c.n, am, x) * azimuth_factor(m, m > 0 ? cos(mr) : 1.0, m < 0 ? sin(mr) : 0.0);
}

}  // namespace hoa
}  // namespace earhip
