// panner.h — the point source panner of the Objects gain producer (include/earhip.h group I) as plain C++ that the device
// kernels (panner_kernels.h, extent_kernels.h, objects_kernels.h), the C ABI (api_panner.hip) and a plain C++ program on
// the CPU (tests/cpp/panner_host.cpp) all compile, as src.h and iir.h are.  No HIP header is needed to include it.
//
// libear's polar point-source panner (src/common/point_source_panner.cpp: triplets, quads, virtual n-gons, the extra
// height loudspeakers and their downmix, the 0+2+0 stereo downmix).  The layout's regions are flattened once, on the host
// and in double precision, into a table of plain records (build_regions: cold); the per-position work — a walk over at
// most ~45 regions with 3x3 products, one or two square roots (pan_full, pan_outputs) — is host-and-device.  The
// arithmetic of a region test follows the reference's operation for operation (:43-51, :86-101, :118-136, :157-190), so
// results agree to the last bits of a double.  Then the small tables of a layout behind channelLock and zoneExclusion.
// What the host set-up refuses it throws as a LayoutFailure (layout_registry.h), which the C ABI turns into earhip::Error.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/earhip.h"
#include "layout_registry.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EARHIP_PAN_HD __host__ __device__
#define EARHIP_PAN_UNROLL _Pragma("unroll")
#else
#define EARHIP_PAN_HD
#define EARHIP_PAN_UNROLL
#endif

namespace earhip {

constexpr int kMaxNgon = 16;   // real loudspeakers around one virtual loudspeaker
constexpr int kMaxPanOut = 32; // loudspeakers of a layout (without LFE)

struct PanRegion {
  int kind;                // 0 triplet, 1 quad, 2 virtual n-gon
  int n;                   // vertices
  int out[kMaxNgon];       // REAL channel (without LFE) each vertex's gain is mixed into (extra height
                           // loudspeakers are mixed into the loudspeaker below / above them)
  // triplet: basis[0]; n-gon: basis[i] of the triplet (tri[i][0], tri[i][1], virtual centre)
  double basis[kMaxNgon][9];
  int tri[kMaxNgon][2];
  double centre_downmix[kMaxNgon];
  // quad
  int order[4];
  double poly_x[9], poly_y[9], pos[4][3];
};

struct PanTable {
  int n_regions;
  int n_real;  // loudspeakers without LFE
  const PanRegion *regions;
};

struct Vec3 {
  double x, y, z;
};
EARHIP_PAN_HD inline Vec3 vsub(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
EARHIP_PAN_HD inline Vec3 vadd(Vec3 a, Vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
EARHIP_PAN_HD inline double vdot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
EARHIP_PAN_HD inline Vec3 vcross(Vec3 a, Vec3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// libear's polar convention (src/common/geom.cpp:82-87): azimuth anticlockwise from the front, degrees
EARHIP_PAN_HD inline Vec3 polar_to_cart(double az, double el, double dist) {
  const double pi = 3.14159265358979323846264338327950288;
  const double a = -az * pi / 180.0, e = el * pi / 180.0;
  return {sin(a) * cos(e) * dist, cos(a) * cos(e) * dist, sin(e) * dist};
}

// position^T * basis of a triplet; true when inside (all coordinates >= -1e-11), pv normalised and
// clamped to [0, 1] (point_source_panner.cpp:43-51)
EARHIP_PAN_HD inline bool triplet_gains(const double *b, Vec3 p, double (&pv)[3]) {
  EARHIP_PAN_UNROLL
  for (int j = 0; j < 3; j++) pv[j] = p.x * b[j] + p.y * b[3 + j] + p.z * b[6 + j];
  const double eps = -1e-11;
  if (!(pv[0] >= eps && pv[1] >= eps && pv[2] >= eps)) return false;
  const double n = sqrt(pv[0] * pv[0] + pv[1] * pv[1] + pv[2] * pv[2]);
  EARHIP_PAN_UNROLL
  for (int j = 0; j < 3; j++) pv[j] = fmin(fmax(pv[j] / n, 0.0), 1.0);
  return true;
}

// first real root in (-1e-10, 1 + 1e-10) of poly . position, clamped (point_source_panner.cpp:157-190)
EARHIP_PAN_HD inline bool quad_pan(const double *poly, Vec3 p, double &out) {
  const double a = poly[0] * p.x + poly[1] * p.y + poly[2] * p.z;
  const double b = poly[3] * p.x + poly[4] * p.y + poly[5] * p.z;
  const double c = poly[6] * p.x + poly[7] * p.y + poly[8] * p.z;
  const double eps = 1e-10;
  double roots[2];
  int nr = 0;
  if (fabs(c) < eps) {
    roots[nr++] = 0.0;
  } else if (fabs(a) < eps) {
    roots[nr++] = -c / b;
  } else {
    const double det = b * b - 4.0 * a * c;
    if (det > eps) {
      roots[nr++] = (-b + sqrt(det)) / (2.0 * a);
      roots[nr++] = (-b - sqrt(det)) / (2.0 * a);
    } else if (det > -eps) {
      roots[nr++] = -b / (2.0 * a);
    }
  }
  for (int i = 0; i < nr; i++)
    if (-eps < roots[i] && roots[i] < 1.0 + eps) {
      out = fmin(fmax(roots[i], 0.0), 1.0);
      return true;
    }
  return false;
}

// One region's answer for a direction: false when the region does not take it, else its gains ADDED into
// real[] (extra loudspeakers already mixed into the real ones).  Triplet :43-51, VirtualNgon :86-101,
// QuadRegion :118-136, :157-190.
EARHIP_PAN_HD inline bool region_try(const PanRegion &R, Vec3 p, double (&real)[kMaxPanOut]) {
  if (R.kind == 0) {
    double pv[3];
    if (!triplet_gains(R.basis[0], p, pv)) return false;
    for (int k = 0; k < 3; k++) real[R.out[k]] += pv[k];
    return true;
  }
  if (R.kind == 1) {
    double x, y;
    if (!(quad_pan(R.poly_x, p, x) && quad_pan(R.poly_y, p, y))) return false;
    double pvs[4];
    pvs[R.order[0]] = (1 - x) * (1 - y);
    pvs[R.order[1]] = x * (1 - y);
    pvs[R.order[2]] = x * y;
    pvs[R.order[3]] = (1 - x) * y;
    Vec3 vel = {0.0, 0.0, 0.0};
    for (int k = 0; k < 4; k++) {
      vel.x += pvs[k] * R.pos[k][0];
      vel.y += pvs[k] * R.pos[k][1];
      vel.z += pvs[k] * R.pos[k][2];
    }
    if (!(vdot(vel, p) > 0)) return false;
    const double n = sqrt(pvs[0] * pvs[0] + pvs[1] * pvs[1] + pvs[2] * pvs[2] + pvs[3] * pvs[3]);
    for (int k = 0; k < 4; k++) real[R.out[k]] += pvs[k] / n;
    return true;
  }
  for (int t = 0; t < R.n; t++) {
    double pv[3];
    if (triplet_gains(R.basis[t], p, pv)) {
      // the virtual centre's gain is distributed to the real loudspeakers, then the n-gon's
      // gains are normalised (:86-101)
      double g[kMaxNgon];
      double n2 = 0.0;
      for (int k = 0; k < R.n; k++) {
        double v = 0.0;
        if (k == R.tri[t][0]) v = pv[0];
        if (k == R.tri[t][1]) v = pv[1];
        g[k] = v + R.centre_downmix[k] * pv[2];
        n2 += g[k] * g[k];
      }
      const double n = sqrt(n2);
      for (int k = 0; k < R.n; k++) real[R.out[k]] += g[k] / n;
      return true;
    }
  }
  return false;
}

// the mix-down of the extra loudspeakers leaves a vector that is normalised again
// (PointSourcePannerDownmix::handle, :239-250)
EARHIP_PAN_HD inline void pan_normalise(const PanTable &T, double (&real)[kMaxPanOut]) {
  double n2 = 0.0;
  for (int c = 0; c < T.n_real; c++) n2 += real[c] * real[c];
  const double n = sqrt(n2);
  for (int c = 0; c < T.n_real; c++) real[c] /= n;
}

// Gains of the real loudspeakers (without LFE) for one direction: the first region that takes the
// position (PolarPointSourcePanner::handle, :208-217).  false: no region took it.
EARHIP_PAN_HD inline bool pan_full(const PanTable &T, Vec3 p, double (&real)[kMaxPanOut]) {
  for (int c = 0; c < T.n_real; c++) real[c] = 0.0;
  bool found = false;
  for (int ri = 0; ri < T.n_regions && !found; ri++) found = region_try(T.regions[ri], p, real);
  if (!found) return false;
  pan_normalise(T, real);
  return true;
}

struct PanParams {
  PanTable table;      // the layout's regions; stereo: those of 0+5+0
  int stereo;          // 0+2+0: pan with 0+5+0, downmix (point_source_panner.cpp:374-398)
  int n_full;          // loudspeakers of the layout incl. LFE
  int full_index[kMaxPanOut];  // real loudspeaker (without LFE) -> index in the full layout
  int stereo_index[2];         // 0+2+0: M+030, M-030
  int real_of_full[kMaxPanOut]; // channel of the full layout -> the panner output that feeds it, -1: LFE
};

// real[] -> the panner's output channels: the layout's loudspeakers without LFE, or the two of 0+2+0
// (StereoPannerDownmix, point_source_panner.cpp:374-398)
EARHIP_PAN_HD inline int pan_outputs(const PanParams &P, const double (&real)[kMaxPanOut], double (&pv)[kMaxPanOut]) {
  if (P.stereo) {
    const double s3 = sqrt(3.0) / 3.0, s5 = sqrt(0.5);
    const double l = real[0] + s3 * real[2] + s5 * real[3];
    const double r = real[1] + s3 * real[2] + s5 * real[4];
    const double n = sqrt(l * l + r * r);
    const double front = fmax(real[0], fmax(real[1], real[2])), back = fmax(real[3], real[4]);
    const double lev = pow(0.5, 0.5 * back / (front + back));  // 0 dB at the front to -3 dB at the back
    pv[0] = l / n * lev;
    pv[1] = r / n * lev;
    return 2;
  }
  for (int c = 0; c < P.table.n_real; c++) pv[c] = real[c];
  return P.table.n_real;
}

// ------------------------------------------------------------------------------------------------
// Set-up (host, double): flatten the regions of a layout
// ------------------------------------------------------------------------------------------------
inline void pan_require(bool ok, const char *m) {
  if (!ok) throw LayoutFailure{EARHIP_INVALID_ARGUMENT, m};
}

inline void invert3(const Vec3 (&rows)[3], double (&inv)[9]) {
  const double m[3][3] = {{rows[0].x, rows[0].y, rows[0].z}, {rows[1].x, rows[1].y, rows[1].z}, {rows[2].x, rows[2].y, rows[2].z}};
  double cof[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      cof[i][j] = m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
    }
  const double inv_det = 1.0 / (m[0][0] * cof[0][0] + m[0][1] * cof[0][1] + m[0][2] * cof[0][2]);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) inv[i * 3 + j] = cof[j][i] * inv_det;  // adjugate / determinant
}

// order of the vertices around their centre (src/common/geom.cpp:37-70)
inline std::vector<int> vertex_order(const std::vector<Vec3> &v) {
  Vec3 c = {0, 0, 0};
  for (auto &p : v) c = vadd(c, p);
  c = {c.x / v.size(), c.y / v.size(), c.z / v.size()};
  const Vec3 a = vsub(v[0], c);
  Vec3 b = {0, 0, 0};
  double best = 1e300;
  for (size_t i = 1; i < v.size(); i++) {
    const Vec3 r = vsub(v[i], c);
    const double col = std::fabs(vdot(r, a));
    if (col < best) best = col, b = r;
  }
  std::vector<double> ang(v.size());
  for (size_t i = 0; i < v.size(); i++) {
    const Vec3 r = vsub(v[i], c);
    ang[i] = std::atan2(vdot(r, a), vdot(r, b));
  }
  std::vector<int> idx(v.size());
  for (size_t i = 0; i < v.size(); i++) idx[i] = (int)i;
  std::sort(idx.begin(), idx.end(), [&](int x, int y) { return ang[x] < ang[y]; });
  return idx;
}

inline void poly_basis(const Vec3 (&q)[4], double (&rows)[9]) {  // point_source_panner.cpp:138-155
  const Vec3 a = q[0], b = q[1], c = q[2], d = q[3];
  const Vec3 r0 = vcross(vsub(b, a), vsub(c, d));
  const Vec3 r1 = vadd(vcross(a, vsub(c, d)), vcross(vsub(b, a), d));
  const Vec3 r2 = vcross(a, d);
  const Vec3 r[3] = {r0, r1, r2};
  for (int i = 0; i < 3; i++) rows[3 * i] = r[i].x, rows[3 * i + 1] = r[i].y, rows[3 * i + 2] = r[i].z;
}

// the regions of a layout with precomputed hull facets (configureFullPolarPanner, :478-561).
// real_az / real_el (optional, one per channel of the full layout): the loudspeakers' real positions; the
// layer logic and the facets follow the nominal ones, the geometry the real ones, as in libear
inline std::vector<PanRegion> build_regions(const LayoutEntry &L, int &n_real, const double *real_az = nullptr,
                                            const double *real_el = nullptr) {
  pan_require(L.facets != nullptr, "layout has no facet table");
  n_real = 0;
  for (int c = 0; c < L.n; c++) n_real += !L.channels[c].is_lfe;
  pan_require(n_real <= kMaxPanOut, "too many loudspeakers");
  // checkScreenSpeakers (:558-577), on the real positions
  for (int c = 0; c < L.n; c++) {
    const LayoutChannel &ch = L.channels[c];
    if (ch.is_lfe || (std::strcmp(ch.name, "M+SC") != 0 && std::strcmp(ch.name, "M-SC") != 0)) continue;
    const double abs_az = std::fabs(real_az ? real_az[c] : ch.azimuth);
    pan_require((5.0 <= abs_az && abs_az < 25.0) || (35.0 <= abs_az && abs_az < 60.0),
                "M+SC or M-SC has azimuth not in the allowed ranges of 5 to 25 and 35 to 60 degrees");
    if (25.0 < abs_az)
      throw LayoutFailure{EARHIP_NOT_IMPLEMENTED, "M+SC and M-SC with azimuths wider than 25 degrees are not currently supported"};
  }
  // the augmented set (layout_registry.h): extra loudspeakers above / below the mid-layer ones where a layer has none
  // in that direction, each mixed into its mid-layer loudspeaker (extraPosVerticalNominal, :256-349), then the
  // virtual loudspeakers below and (unless the layout has one overhead) above (:442-455)
  std::vector<Vec3> verts;
  std::vector<int> mix_to;  // augmented vertex -> real loudspeaker
  std::vector<int> virt;
  for (const AugVertex &v : augment_layout(L, real_az, real_el)) {
    if (v.pole) virt.push_back((int)verts.size());
    verts.push_back(v.pole ? Vec3{0.0, 0.0, (double)v.pole} : polar_to_cart(v.az, v.el, 1.0));
    mix_to.push_back(v.mix_to);
  }
  auto is_virtual = [&](int v) { return std::find(virt.begin(), virt.end(), v) != virt.end(); };
  std::vector<std::vector<int>> facets;
  for (const int *f = L.facets; *f; f += 1 + *f) facets.emplace_back(f + 1, f + 1 + *f);
  std::vector<PanRegion> regions;
  // n-gons around the virtual loudspeakers first (:497-527)
  for (int vv : virt) {
    std::vector<int> ring;  // ascending, like the reference's std::set
    for (auto &f : facets)
      if (std::find(f.begin(), f.end(), vv) != f.end())
        for (int v : f)
          if (v != vv && std::find(ring.begin(), ring.end(), v) == ring.end()) ring.push_back(v);
    std::sort(ring.begin(), ring.end());
    if ((int)ring.size() > kMaxNgon)
      throw LayoutFailure{EARHIP_NOT_IMPLEMENTED, "more than " + std::to_string(kMaxNgon) + " loudspeakers around a virtual loudspeaker"};
    pan_require(ring.size() >= 3, "unsupported n-gon size");
    for (int v : ring) pan_require(!is_virtual(v), "invalid triangulation");
    PanRegion R;
    std::memset(&R, 0, sizeof(R));
    R.kind = 2;
    R.n = (int)ring.size();
    std::vector<Vec3> pos;
    for (int k = 0; k < R.n; k++) {
      R.out[k] = mix_to[ring[k]];
      R.centre_downmix[k] = 1.0 / std::sqrt((double)R.n);
      pos.push_back(verts[ring[k]]);
    }
    const std::vector<int> order = vertex_order(pos);
    for (int t = 0; t < R.n; t++) {
      const int a = order[t], b = order[(t + 1) % R.n];
      R.tri[t][0] = a;
      R.tri[t][1] = b;
      const Vec3 rows[3] = {pos[a], pos[b], verts[vv]};
      invert3(rows, R.basis[t]);
    }
    regions.push_back(R);
  }
  // every other facet: a triplet or a quad (:528-559)
  for (auto &f : facets) {
    bool touches = false;
    for (int v : f) touches = touches || is_virtual(v);
    if (touches) continue;
    PanRegion R;
    std::memset(&R, 0, sizeof(R));
    R.n = (int)f.size();
    if (f.size() != 3 && f.size() != 4)
      throw LayoutFailure{EARHIP_INTERNAL_ERROR, "internal error: facets with more than 4 vertices are not supported"};
    for (int k = 0; k < R.n; k++) R.out[k] = mix_to[f[k]];
    if (f.size() == 3) {
      R.kind = 0;
      const Vec3 rows[3] = {verts[f[0]], verts[f[1]], verts[f[2]]};
      invert3(rows, R.basis[0]);
    } else {
      R.kind = 1;
      std::vector<Vec3> pos;
      for (int k = 0; k < 4; k++) {
        pos.push_back(verts[f[k]]);
        R.pos[k][0] = verts[f[k]].x, R.pos[k][1] = verts[f[k]].y, R.pos[k][2] = verts[f[k]].z;
      }
      const std::vector<int> order = vertex_order(pos);
      Vec3 q[4], qs[4];
      for (int k = 0; k < 4; k++) R.order[k] = order[k], q[k] = pos[order[k]];
      for (int k = 0; k < 4; k++) qs[k] = q[(k + 1) % 4];
      poly_basis(q, R.poly_x);
      poly_basis(qs, R.poly_y);
    }
    regions.push_back(R);
  }
  return regions;
}

// What a panner of layout L pans with: its regions at the real positions (both NULL: nominal) and P, all but
// P.table.regions, which is the caller's copy of what is returned.  0+2+0 pans on the nominal 0+5+0
// (configureStereoPolarPanner, :406-429).
inline std::vector<PanRegion> pan_params(const LayoutEntry &L, const double *azimuth, const double *elevation, PanParams &P) {
  std::memset(&P, 0, sizeof(P));
  P.n_full = L.n;
  int n_real = 0;
  std::vector<PanRegion> regions;
  if (std::strcmp(L.name, "0+2+0") == 0) {
    const LayoutEntry *L050 = nullptr;
    for (int i = 0; i < kNumLayouts; i++)
      if (std::strcmp(kLayouts[i].name, "0+5+0") == 0) L050 = &kLayouts[i];
    regions = build_regions(*L050, n_real);
    P.stereo = 1;
    for (int c = 0; c < L.n; c++) {
      if (std::strcmp(L.channels[c].name, "M+030") == 0) P.stereo_index[0] = c;
      if (std::strcmp(L.channels[c].name, "M-030") == 0) P.stereo_index[1] = c;
    }
  } else {
    regions = build_regions(L, n_real, azimuth, elevation);
    int k = 0;
    for (int c = 0; c < L.n; c++)
      if (!L.channels[c].is_lfe) P.full_index[k++] = c;
  }
  pan_require(L.n <= kMaxPanOut, "too many channels");
  for (int c = 0; c < kMaxPanOut; c++) P.real_of_full[c] = -1;
  const int n_pv = P.stereo ? 2 : n_real;
  for (int k = 0; k < n_pv; k++) P.real_of_full[P.stereo ? P.stereo_index[k] : P.full_index[k]] = k;
  P.table.n_regions = (int)regions.size();
  P.table.n_real = n_real;
  return regions;
}

// ---- channel lock and zone exclusion: the small tables of a layout (include/earhip.h group I, the objects forms)
struct ObjSpeaker {
  int full;       // index in the full layout
  double az, el;  // nominal position
  Vec3 nominal;   // ... on the unit sphere
};
// the non-LFE loudspeakers of a layout, in layout order
inline std::vector<ObjSpeaker> objects_speakers(const LayoutEntry &L) {
  std::vector<ObjSpeaker> sp;
  for (int c = 0; c < L.n; c++)
    if (!L.channels[c].is_lfe)
      sp.push_back({c, L.channels[c].azimuth, L.channels[c].elevation,
                    polar_to_cart(L.channels[c].azimuth, L.channels[c].elevation, 1.0)});
  pan_require((int)sp.size() <= kMaxLayoutSpeakers && L.n <= 32, "too many loudspeakers");
  return sp;
}
// what a create with nominal positions does on the host (earhip_layout_define runs it, so that a layout the region
// builder refuses fails when it is defined)
inline void panner_dry_run(const LayoutEntry &L) {
  int n_real = 0;
  (void)build_regions(L, n_real);
  (void)objects_speakers(L);
}
// rank[s]: the place of loudspeaker s in the lock priority order: ascending (|el|, el, |az|, az), nominal
inline std::vector<int> objects_lock_rank(const std::vector<ObjSpeaker> &sp) {
  std::vector<int> order(sp.size()), rank(sp.size());
  for (size_t s = 0; s < sp.size(); s++) order[s] = (int)s;
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    const double ka[4] = {std::fabs(sp[a].el), sp[a].el, std::fabs(sp[a].az), sp[a].az};
    const double kb[4] = {std::fabs(sp[b].el), sp[b].el, std::fabs(sp[b].az), sp[b].az};
    return std::lexicographical_compare(ka, ka + 4, kb, kb + 4);
  });
  for (size_t r = 0; r < order.size(); r++) rank[order[r]] = (int)r;
  return rank;
}
// groups[i][g]: the g-th nearest group of loudspeakers of loudspeaker i as a set of bits, itself first
inline void objects_zone_groups(const std::vector<ObjSpeaker> &sp, unsigned (&groups)[kMaxLayoutSpeakers][kMaxLayoutSpeakers]) {
  static const int LP[4][4] = {{0, 1, 2, 3}, {3, 0, 1, 2}, {3, 2, 0, 1}, {3, 2, 1, 0}};
  const int n = (int)sp.size();
  std::vector<int> layer(n), fb(n);
  for (int i = 0; i < n; i++) {
    layer[i] = sp[i].el < -10.0 ? 0 : sp[i].el < 10.0 ? 1 : sp[i].el < 60.0 ? 2 : 3;
    fb[i] = sp[i].nominal.y > 1e-6 ? 1 : sp[i].nominal.y < -1e-6 ? -1 : 0;
  }
  std::memset(groups, 0, sizeof(groups));
  struct Key {
    long long k[4];
    int j;
  };
  for (int i = 0; i < n; i++) {
    std::vector<Key> keys;
    for (int j = 0; j < n; j++) {
      const Vec3 d = vsub(sp[i].nominal, sp[j].nominal);
      keys.push_back({{LP[layer[i]][layer[j]], std::abs(fb[i] - fb[j]), std::llround(std::sqrt(vdot(d, d)) * 1e6),
                       std::llround(std::fabs(d.y) * 1e6)}, j});
    }
    std::stable_sort(keys.begin(), keys.end(),
                     [](const Key &a, const Key &b) { return std::lexicographical_compare(a.k, a.k + 4, b.k, b.k + 4); });
    int g = -1;
    for (int q = 0; q < n; q++) {
      if (q == 0 || !std::equal(keys[q].k, keys[q].k + 4, keys[q - 1].k)) g++;
      groups[i][g] |= 1u << keys[q].j;
    }
  }
}
// is azimuth az inside the range that runs anticlockwise from lo to hi (tol 1e-6)
inline bool objects_az_in_range(double az, double lo, double hi) {
  const double tol = 1e-6;
  double d = std::fmod(hi - lo, 360.0);
  if (d < 0.0) d += 360.0;
  if (d == 0.0 && hi > lo) d = 360.0;
  const double start = lo - tol;
  double x = std::fmod(az - start, 360.0);
  if (x < 0.0) x += 360.0;
  return start + x <= lo + d + tol;
}
// mask over the full layout -> set of bits over the non-LFE loudspeakers; the full set excludes nothing
inline unsigned objects_excluded_set(const std::vector<ObjSpeaker> &sp, uint32_t mask) {
  unsigned em = 0;
  for (size_t s = 0; s < sp.size(); s++)
    if (mask >> sp[s].full & 1u) em |= 1u << s;
  return em == (1u << sp.size()) - 1u ? 0u : em;
}
// earhip_objects_excluded_channels: the channels of the full layout whose nominal position lies in one of the zones
inline uint32_t objects_excluded_channels(const std::vector<ObjSpeaker> &sp, int n_zones, const earhip_exclusion_zone *zones) {
  const double tol = 1e-6;
  uint32_t m = 0;
  for (const ObjSpeaker &c : sp)
    for (int k = 0; k < n_zones; k++) {
      const earhip_exclusion_zone &z = zones[k];
      bool inside;
      if (z.cartesian)
        inside = z.min_x - tol < c.nominal.x && c.nominal.x < z.max_x + tol && z.min_y - tol < c.nominal.y &&
                 c.nominal.y < z.max_y + tol && z.min_z - tol < c.nominal.z && c.nominal.z < z.max_z + tol;
      else
        inside = z.min_elevation - tol < c.el && c.el < z.max_elevation + tol &&
                 (std::fabs(c.el) > 90.0 - tol || objects_az_in_range(c.az, z.min_azimuth, z.max_azimuth));
      if (inside) m |= 1u << c.full;
    }
  return m;
}
// earhip_objects_zone_downmix: matrix [N][N] over the full layout (N = L.n), row: from, column: to
inline void objects_zone_downmix(const LayoutEntry &L, uint32_t mask, double *matrix) {
  const std::vector<ObjSpeaker> sp = objects_speakers(L);
  const size_t N = (size_t)L.n;
  if (N < 32 && (mask >> N) != 0)
    throw LayoutFailure{EARHIP_INVALID_ARGUMENT, "mask has a bit set beyond the layout's " + std::to_string(N) + " channels"};
  for (size_t r = 0; r < N; r++)
    for (size_t c = 0; c < N; c++) matrix[r * N + c] = r == c ? 1.0 : 0.0;
  const unsigned em = objects_excluded_set(sp, mask);
  if (em == 0) return;
  unsigned groups[kMaxLayoutSpeakers][kMaxLayoutSpeakers];
  objects_zone_groups(sp, groups);
  for (size_t i = 0; i < sp.size(); i++) {
    if (!(em >> i & 1u)) continue;
    unsigned to = 0;
    for (size_t g = 0; g < sp.size() && to == 0; g++) to = groups[i][g] & ~em;
    matrix[sp[i].full * N + sp[i].full] = 0.0;
    for (size_t j = 0; j < sp.size(); j++)
      if (to >> j & 1u) matrix[sp[i].full * N + sp[j].full] = 1.0 / __builtin_popcount(to);
  }
}

}  // namespace earhip
