// allo_objects.h — the allocentric panner with channelLock, Cartesian objectDivergence and extent (earhip group U,
// include/earhip.h, where the gains are specified), on group T's snapped table (allo.h).  One plain C++ core in double, shared
// by the host form (api_allo.hip) and the kernel (allo_objects_kernels.h); it compiles without HIP
// (tests/cpp/test_allo_objects_core.cpp builds it with g++).
//
// The work is split per loudspeaker.  Group T's weight of a loudspeaker c is a product of one function per coordinate,
// w_c(s) = (wz_c(s.z) * wy_c(s.y)) * wx_c(s.x): wz_c the weight of c's plane among the planes of A, wy_c the weight of c's row
// within that plane, wx_c the weight of c within that row.  Each is fixed by c's own coordinate and its two neighbours in
// that set (Neighbours below), with bracket()'s own arithmetic, so (wz * wy) * wx at the object's position has the bits of
// pan_position.  The extent's sum over the 20^3 grid sources is never formed: the fall-off is a product over the axes too, so
//   G_c^p = sum_s (F_x F_y F_z w_c(s))^p = Pz_c * Py_c * Px_c,   Pk_c = sum_j (F_k(c_j) * wk_c(c_j))^p,
// 60 terms per loudspeaker and position.  Each term is one exp2 of p * (log2 F + log2 w); log2 F needs no exp at all, and
// log2 w is shared by the up to three positions of a diverged object, which differ only in F.
#pragma once

#include "allo.h"

namespace earhip {
namespace allo {

constexpr int kGrid = 20;                        // grid points of a non-flat axis: c_j = (2 j - 19) / 19
constexpr double kLockX = 1.0 / 16.0, kLockY = 4.0, kLockZ = 32.0;  // weights of the squared offsets in the lock distance
constexpr double kLockTol = 1e-10;
constexpr double kFallOff = 5.0625;              // F = 10^(-kFallOff (u^4 - 1))
constexpr double kLog2Of10 = 3.32192809488736234787031942948939;
constexpr double kMinHalfWidth = 0.1;            // of the plateau: at least one grid point lies on it
constexpr double kFullExtent = 0.2;              // s_max from which the extent's gains stand alone (alpha = 1)

// What the handle's table fixes beyond the positions: the lock priority order and the flat axes.  A kernel argument, by value.
struct Extras {
  int n_order;                        // loudspeakers that are not LFE
  unsigned char order[kMaxChannels];  // their channel indices, ascending by (|z|, z, -y, |x|, x)
  int flat[3];                        // axis k (x, y, z): every loudspeaker shares its coordinate
};

inline bool lock_before(const Table &t, int a, int b) {
  const double ka[5] = {fabs(t.z[a]), t.z[a], -t.y[a], fabs(t.x[a]), t.x[a]};
  const double kb[5] = {fabs(t.z[b]), t.z[b], -t.y[b], fabs(t.x[b]), t.x[b]};
  for (int k = 0; k < 5; k++)
    if (ka[k] != kb[k]) return ka[k] < kb[k];
  return false;  // (the handle's positions are distinct)
}

inline Extras make_extras(const Table &t) {
  Extras e;
  e.n_order = 0;
  for (int c = 0; c < kMaxChannels; c++) e.order[c] = 0;
  for (int c = 0; c < t.n; c++) {
    if (!((t.real >> c) & 1u)) continue;
    int k = e.n_order++;
    for (; k > 0 && lock_before(t, c, e.order[k - 1]); k--) e.order[k] = e.order[k - 1];  // insertion sort
    e.order[k] = (unsigned char)c;
  }
  const int first = e.n_order ? e.order[0] : 0;
  e.flat[0] = e.flat[1] = e.flat[2] = 1;
  for (int k = 0; k < e.n_order; k++) {
    const int c = e.order[k];
    if (t.x[c] != t.x[first]) e.flat[0] = 0;
    if (t.y[c] != t.y[first]) e.flat[1] = 0;
    if (t.z[c] != t.z[first]) e.flat[2] = 0;
  }
  return e;
}

// what the host form refuses and the device form marks, beyond position_valid
EARHIP_ALLO_HD inline bool objects_valid(double width, double height, double depth, double max_distance, double divergence,
                                         double position_range) {
  const double big = 1.7976931348623157e308;  // (a comparison is false for NaN)
  return width >= 0.0 && width <= big && height >= 0.0 && height <= big && depth >= 0.0 && depth <= big &&
         max_distance >= 0.0 && divergence >= 0.0 && divergence <= 1.0 && position_range >= 0.0 && position_range <= big;
}

// One object after steps 1 and 2 and the parameters of step 3, the same for all of its loudspeakers.
struct Object {
  uint32_t active;   // A
  int n_pos;         // 1, or 3 with divergence
  double q[3][3];    // [position][x, y, z]
  double weight[3];  // power weights of the positions
  int extent;        // s_max > 0
  double size[3];    // (width, depth, height): on x, y, z
  double p, alpha;
};

EARHIP_ALLO_HD inline double lock_distance(const Table &t, int c, double x, double y, double z) {
  const double dx = x - t.x[c], dy = y - t.y[c], dz = z - t.z[c];
  return sqrt(kLockX * (dx * dx) + kLockY * (dy * dy) + kLockZ * (dz * dz));
}

EARHIP_ALLO_HD inline void prepare_object(const Table &t, const Extras &e, double x, double y, double z, double width,
                                          double height, double depth, bool lock, double max_distance, double divergence,
                                          double position_range, uint32_t excluded, Object &o) {
  o.active = t.real & ~excluded;
  if (!o.active) o.active = t.real;
  if (lock) {  // step 1: every loudspeaker is a candidate, the excluded ones too
    const double limit = max_distance + kLockTol;
    double nearest = HUGE_VAL;
    for (int k = 0; k < e.n_order; k++) {
      const double d = lock_distance(t, e.order[k], x, y, z);
      if (d < limit && d < nearest) nearest = d;
    }
    for (int k = 0; k < e.n_order; k++) {
      const int c = e.order[k];
      const double d = lock_distance(t, c, x, y, z);
      if (d < limit && d < nearest + kLockTol) {
        x = t.x[c], y = t.y[c], z = t.z[c];
        break;
      }
    }
  }
  o.n_pos = divergence == 0.0 ? 1 : 3;  // step 2
  for (int k = 0; k < 3; k++) o.q[k][0] = x, o.q[k][1] = y, o.q[k][2] = z;
  o.q[1][0] = x - position_range, o.q[2][0] = x + position_range;
  o.weight[0] = divergence == 0.0 ? 1.0 : (1.0 - divergence) / (1.0 + divergence);
  o.weight[1] = o.weight[2] = divergence / (1.0 + divergence);
  o.size[0] = width, o.size[1] = depth, o.size[2] = height;  // step 3
  double sum = 0.0, s_max = 0.0;
  int axes = 0;
  for (int k = 0; k < 3; k++) {
    if (e.flat[k]) continue;
    const double s = o.size[k] < 1.0 ? o.size[k] : 1.0;
    sum += s, axes++;
    if (s > s_max) s_max = s;
  }
  const double s_eff = axes ? sum / axes : 0.0;
  o.extent = s_max > 0.0;
  o.p = s_eff <= 0.5 ? 6.0 : 6.0 - 8.0 * (s_eff - 0.5);
  o.alpha = s_max < kFullExtent ? s_max / kFullExtent : 1.0;
}

// a loudspeaker's coordinate on one axis and its neighbours in the set its bracket is taken over (-inf, +inf: none)
struct Neighbours {
  double lo, at, hi;
};

// of loudspeaker c (a member of `active`): [0] x within its row, [1] y within its plane, [2] z among the planes
EARHIP_ALLO_HD inline void neighbours(const Table &t, uint32_t active, int c, Neighbours nb[3]) {
  const double xc = t.x[c], yc = t.y[c], zc = t.z[c];
  double lo[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL}, hi[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL};
  for (int o = 0; o < t.n; o++) {
    if (!((active >> o) & 1u)) continue;
    const double x = t.x[o], y = t.y[o], z = t.z[o];
    if (z < zc && z > lo[2]) lo[2] = z;
    if (z > zc && z < hi[2]) hi[2] = z;
    if (z != zc) continue;
    if (y < yc && y > lo[1]) lo[1] = y;
    if (y > yc && y < hi[1]) hi[1] = y;
    if (y != yc) continue;
    if (x < xc && x > lo[0]) lo[0] = x;
    if (x > xc && x < hi[0]) hi[0] = x;
  }
  nb[0].lo = lo[0], nb[0].at = xc, nb[0].hi = hi[0];
  nb[1].lo = lo[1], nb[1].at = yc, nb[1].hi = hi[1];
  nb[2].lo = lo[2], nb[2].at = zc, nb[2].hi = hi[2];
}

// the weight bracket() gives the value nb.at at v, with bracket()'s operations
EARHIP_ALLO_HD inline double axis_weight(const Neighbours &nb, double v) {
  if (v == nb.at) return 1.0;
  if (v < nb.at) {
    if (nb.lo == -HUGE_VAL) return 1.0;
    if (v <= nb.lo) return 0.0;
    const double f = (v - nb.lo) / (nb.at - nb.lo);
    return sin(f * kHalfPi);
  }
  if (nb.hi == HUGE_VAL) return 1.0;
  if (v >= nb.hi) return 0.0;
  const double f = (v - nb.at) / (nb.hi - nb.at);
  return cos(f * kHalfPi);
}

// log2 of F_k at the grid point c of an object's position coordinate q with size `size`: 0 on the plateau
EARHIP_ALLO_HD inline double log2_fall_off(double c, double q, double size) {
  const double o = q < -1.0 ? -1.0 : (q > 1.0 ? 1.0 : q);
  const double h = size > kMinHalfWidth ? size : kMinHalfWidth;
  const double a = fabs(c - o);
  const double u = (a > h ? a : h) / h;
  const double u2 = u * u;
  return -(kFallOff * kLog2Of10) * (u2 * u2 - 1.0);
}

// One axis of loudspeaker c: log2_G[k] += log2 Pk_c at the position coordinates q[k] (-inf where no term is left).  The
// loops over k have constant bounds, so every index is static and the arrays live in registers.
EARHIP_ALLO_HD inline void add_axis(const Neighbours &nb, int n_pos, double q0, double q1, double q2, double size, double p,
                                    double log2_G[3]) {
  const double q[3] = {q0, q1, q2};
  double P[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < kGrid; j++) {
    const double cj = (2 * j - (kGrid - 1)) / (double)(kGrid - 1);
    const double wj = axis_weight(nb, cj);
    if (wj <= 0.0) continue;
    const double lw = log2(wj);
    for (int k = 0; k < 3; k++)
      if (k < n_pos) P[k] += exp2(p * (log2_fall_off(cj, q[k], size) + lw));
  }
  for (int k = 0; k < 3; k++) log2_G[k] += log2(P[k]);
}

// Loudspeaker c of an object, per position k < o.n_pos: w[k] = w_c(q_k), group T's weight with its bits, and, with extent,
// G[k] = G_c(q_k) before the normalisation over the loudspeakers.  A channel outside A, or an LFE, gets zeros.
EARHIP_ALLO_HD inline void channel_terms(const Table &t, const Extras &e, const Object &o, int c, double w[3], double G[3]) {
  w[0] = w[1] = w[2] = 0.0, G[0] = G[1] = G[2] = 0.0;
  if (c >= t.n || !((o.active >> c) & 1u)) return;
  Neighbours nb[3];
  neighbours(t, o.active, c, nb);
  for (int k = 0; k < 3; k++)
    if (k < o.n_pos) w[k] = (axis_weight(nb[2], o.q[k][2]) * axis_weight(nb[1], o.q[k][1])) * axis_weight(nb[0], o.q[k][0]);
  if (!o.extent) return;
  double log2_G[3] = {0.0, 0.0, 0.0};  // a flat axis has one grid point, F = 1 and weight 1: Pk_c = 1
  if (!e.flat[0]) add_axis(nb[0], o.n_pos, o.q[0][0], o.q[1][0], o.q[2][0], o.size[0], o.p, log2_G);
  double yz[3] = {0.0, 0.0, 0.0};  // the positions of a diverged object differ in x alone
  if (!e.flat[1]) add_axis(nb[1], 1, o.q[0][1], 0.0, 0.0, o.size[1], o.p, yz);
  if (!e.flat[2]) add_axis(nb[2], 1, o.q[0][2], 0.0, 0.0, o.size[2], o.p, yz);
  for (int k = 0; k < 3; k++) log2_G[k] += yz[0];
  for (int k = 0; k < 3; k++)
    if (k < o.n_pos) G[k] = exp2(log2_G[k] / o.p);
}

// Steps 3 (the blend) and 4 for one loudspeaker: norm[k] = sqrt(sum_c G_c(q_k)^2), read only with extent.
EARHIP_ALLO_HD inline double combine(const Object &o, const double w[3], const double G[3], const double norm[3]) {
  double g[3] = {w[0], w[1], w[2]};
  if (o.extent)
    for (int k = 0; k < 3; k++) {
      if (k >= o.n_pos) continue;
      const double ghat = G[k] / norm[k];
      g[k] = sqrt((1.0 - o.alpha) * (w[k] * w[k]) + o.alpha * (ghat * ghat));
    }
  if (o.n_pos == 1) return g[0];
  return sqrt(o.weight[0] * (g[0] * g[0]) + o.weight[1] * (g[1] * g[1]) + o.weight[2] * (g[2] * g[2]));
}

// one output: a loudspeaker without gain, or an LFE, holds +0 whatever the sign of `gain`, as in group T's rows
EARHIP_ALLO_HD inline float row_value(double g_c, double gain, double factor) {
  return g_c == 0.0 ? 0.0f : (float)(g_c * gain * factor);
}

}  // namespace allo
}  // namespace earhip
