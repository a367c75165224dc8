// allo.h — the allocentric (Cartesian) point-source panner of earhip group T (include/earhip.h, where the gains are
// specified): the loudspeakers stand on a cube and a position is panned along z, then y, then x.  One plain C++ core in
// double, shared by the host form (api_allo.hip) and the kernel (allo_kernels.h); it compiles without HIP
// (tests/cpp/test_allo_core.cpp builds it with g++).  The Makefile builds with -ffp-contract=off, so no FMA is formed and
// the two forms differ only in the math library behind cos, sin and sqrt.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EARHIP_ALLO_HD __host__ __device__
#else
#define EARHIP_ALLO_HD
#endif

namespace earhip {
namespace allo {

constexpr int kMaxChannels = 32;                          // channels of a layout, LFE included (the 32-bit masks)
constexpr double kHalfPi = 1.57079632679489661923132169;  // the double nearest to pi/2
constexpr double kSnap = 1e-6;                            // coordinates this close are one plane, row or column

// A handle's loudspeakers after snapping, per channel of the full layout; passed to the kernel by value.  real: bit c set =
// channel c is a loudspeaker (not an LFE); the coordinates of the other channels are not read.
struct Table {
  int n;
  uint32_t real;
  double x[kMaxChannels], y[kMaxChannels], z[kMaxChannels];
};

// bracket(V, v) of the specification over V = {coord[c] : c in set}: n = 0 (empty set), 1 or 2 entries, each with its
// weight and the members of the set that stand at its value.
struct Bracket {
  int n;
  double w[2];
  uint32_t at[2];
};

EARHIP_ALLO_HD inline Bracket bracket(const double *coord, int n_channels, uint32_t set, double v) {
  const double inf = HUGE_VAL;
  double lo = -inf, hi = inf;
  uint32_t at_lo = 0, at_hi = 0;
  for (int c = 0; c < n_channels; c++) {
    if (!((set >> c) & 1u)) continue;
    const double p = coord[c];
    const uint32_t bit = 1u << c;
    if (p <= v) {
      if (p > lo) lo = p, at_lo = bit;
      else if (p == lo) at_lo |= bit;
    }
    if (p >= v) {
      if (p < hi) hi = p, at_hi = bit;
      else if (p == hi) at_hi |= bit;
    }
  }
  Bracket b = {0, {0.0, 0.0}, {0u, 0u}};
  if (!at_lo && !at_hi) return b;
  if (!at_lo || !at_hi || lo == hi) {
    b.n = 1, b.w[0] = 1.0, b.at[0] = at_lo ? at_lo : at_hi;
    return b;
  }
  const double f = (v - lo) / (hi - lo);
  const double a = f * kHalfPi;
  b.n = 2, b.w[0] = cos(a), b.w[1] = sin(a), b.at[0] = at_lo, b.at[1] = at_hi;
  return b;
}

// The gains of one position: at most 8 loudspeakers.  Slot 4 kz + 2 ky + kx is the (kz, ky, kx) entry of the three
// brackets; c < 0: the slot is unused.  The loops have constant bounds, so every index below is static and the slots
// live in registers.
struct Gains {
  int c[8];
  double w[8];
};

// excluded: bit c set = channel c of the full layout is excluded; bits of LFE channels and beyond the layout are ignored
EARHIP_ALLO_HD inline void pan_position(const Table &t, double x, double y, double z, uint32_t excluded, Gains &g) {
  uint32_t active = t.real & ~excluded;
  if (!active) active = t.real;
  const Bracket bz = bracket(t.z, t.n, active, z);
  for (int kz = 0; kz < 2; kz++) {
    const Bracket by = bracket(t.y, t.n, kz < bz.n ? bz.at[kz] : 0u, y);
    for (int ky = 0; ky < 2; ky++) {
      const Bracket bx = bracket(t.x, t.n, ky < by.n ? by.at[ky] : 0u, x);
      for (int kx = 0; kx < 2; kx++) {
        const int slot = 4 * kz + 2 * ky + kx;
        const bool used = kx < bx.n;  // (an empty plane or row leaves its brackets empty)
        g.c[slot] = used ? __builtin_ctz(bx.at[kx]) : -1;  // (one loudspeaker: the handle's positions are distinct)
        g.w[slot] = used ? (bz.w[kz] * by.w[ky]) * bx.w[kx] : 0.0;
      }
    }
  }
}

// what the host form refuses and the device form marks (a mask bit beyond the layout is the host form's own check)
EARHIP_ALLO_HD inline bool position_valid(double x, double y, double z, double gain, double diffuse) {
  const double big = 1.7976931348623157e308;  // (a comparison is false for NaN)
  return fabs(x) <= big && fabs(y) <= big && fabs(z) <= big && fabs(gain) <= big && diffuse >= 0.0 && diffuse <= 1.0;
}

// the two factors of a row: direct[c] = (float)(w_c * gain * direct_factor), diffuse_out[c] = (float)(w_c * gain * diffuse_factor)
EARHIP_ALLO_HD inline double direct_factor(double diffuse) { return sqrt(1.0 - diffuse); }
EARHIP_ALLO_HD inline double diffuse_factor(double diffuse) { return sqrt(diffuse); }

// One row of one output: +0 everywhere, then the at most 8 weights.  row: n_channels floats.
EARHIP_ALLO_HD inline void write_row(const Table &t, const Gains &g, double gain, double factor, float *row) {
  for (int c = 0; c < t.n; c++) row[c] = 0.0f;
  for (int s = 0; s < 8; s++)
    if (g.c[s] >= 0) row[g.c[s]] = (float)(g.w[s] * gain * factor);
}

}  // namespace allo
}  // namespace earhip
