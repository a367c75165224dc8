// layout_registry.h — loudspeaker layouts beyond the ten BS.2051 rows of layout_table.h (include/earhip.h group H,
// earhip_layout_define): the one lookup every entry point uses, the augmented loudspeaker set of a layout
// (libear's extraPosVerticalNominal and virtual loudspeakers, src/common/point_source_panner.cpp:256-349, :431-476)
// and the convex hull that triangulates it (libear's convex_hull, src/common/convex_hull.cpp, restated).  Plain host
// C++ in double, no device and no HIP header: tests/cpp/test_hull.cpp compiles it with g++.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "layout_table.h"

namespace earhip {

constexpr int kMaxLayoutChannels = 32;      // channels of a layout, LFE included (kMaxPanOut, the 32-bit channel masks)
constexpr int kMaxLayoutSpeakers = 22;      // ... of which not LFE (kObjMaxOut: the lock and zone tables of the objects kernels)
constexpr int kMaxDefinedLayouts = 256;     // definitions a process may make
constexpr double kHullTolerance = 1e-5;     // libear's default

// what the geometry of a layout can fail with; `status` is an EARHIP_* code (the callers turn it into earhip::Error)
struct LayoutFailure {
  int status;
  std::string msg;
};

// the BS.2051 rows, then the definitions; throws earhip::Error{EARHIP_UNKNOWN_LAYOUT, "unknown layout: NAME"}
// (layout_registry.cpp).  The entry and everything it points at live as long as the process.
const LayoutEntry &find_layout(const char *name);

// One vertex of the augmented set, in polar form: a real loudspeaker, an extra one above or below a mid-layer
// loudspeaker (its gain is mixed into that loudspeaker), or a virtual one straight below / above.
struct AugVertex {
  double az, el;
  int mix_to;  // loudspeaker (counting those that are not LFE) this vertex's gain goes to; -1: virtual
  int pole;    // 0: on the sphere at (az, el); -1 / +1: the virtual loudspeaker at (0, 0, -1) / (0, 0, +1)
};

// The augmented set of a layout whose loudspeakers stand at real_az / real_el (one per channel of the full layout; both
// NULL: nominal): the loudspeakers that are not LFE; per layer (below, above) an extra loudspeaker under / over every
// mid-layer loudspeaker outside that layer's azimuth range, at the layer's mean elevation; the virtual bottom; the
// virtual top unless the layout has T+000 or UH+180.  The layer logic follows the nominal positions.
inline std::vector<AugVertex> augment_layout(const LayoutEntry &L, const double *real_az, const double *real_el) {
  struct Ch {
    const char *name;
    double az, el, az_nom, el_nom;
  };
  std::vector<Ch> real;
  for (int c = 0; c < L.n; c++)
    if (!L.channels[c].is_lfe)
      real.push_back({L.channels[c].name, real_az ? real_az[c] : L.channels[c].azimuth,
                      real_el ? real_el[c] : L.channels[c].elevation, L.channels[c].azimuth, L.channels[c].elevation});
  const int n_real = (int)real.size();
  std::vector<AugVertex> verts;
  for (int c = 0; c < n_real; c++) verts.push_back({real[c].az, real[c].el, c, 0});
  const double layers[2][3] = {{-30.0, -70.0, -10.0}, {30.0, 10.0, 70.0}};
  for (auto &layer : layers) {
    double az_range = -1.0, el_sum = 0.0;
    int in_layer = 0;
    for (auto &ch : real)
      if (layer[1] <= ch.el_nom && ch.el_nom <= layer[2])
        az_range = std::max(az_range, std::fabs(ch.az_nom)), el_sum += ch.el, in_layer++;
    const double az_limit = in_layer ? az_range + 40.0 : 0.0;
    const double layer_el = in_layer ? el_sum / in_layer : layer[0];
    for (int c = 0; c < n_real; c++)
      if (-10 <= real[c].el_nom && real[c].el_nom <= 10 && std::fabs(real[c].az) >= az_limit - 1e-5)
        verts.push_back({real[c].az, layer_el, c, 0});
  }
  bool overhead = false;
  for (auto &ch : real) overhead = overhead || std::strcmp(ch.name, "T+000") == 0 || std::strcmp(ch.name, "UH+180") == 0;
  verts.push_back({0.0, -90.0, -1, -1});
  if (!overhead) verts.push_back({0.0, 90.0, -1, +1});
  return verts;
}

using HullPoint = std::array<double, 3>;

// libear's polar convention (src/common/geom.cpp:82-87); the virtual loudspeakers are exact
inline HullPoint aug_point(const AugVertex &v) {
  if (v.pole) return {0.0, 0.0, (double)v.pole};
  const double pi = 3.14159265358979323846264338327950288;
  const double a = -v.az * pi / 180.0, e = v.el * pi / 180.0;
  return {std::sin(a) * std::cos(e), std::cos(a) * std::cos(e), std::sin(e)};
}

namespace hull_detail {
inline HullPoint sub(const HullPoint &a, const HullPoint &b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
inline double dot(const HullPoint &a, const HullPoint &b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline HullPoint cross(const HullPoint &a, const HullPoint &b) {
  return {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
}
}  // namespace hull_detail

// The facets of the convex hull of pts, each a list of vertex indices in ascending order, by brute force (the sets are
// a few dozen points, once per layout).  A triple of points spans a hull triangle when every point lies on one side of
// its plane — the side of the points' mean, which is inside the hull; triples whose plane passes through the mean are
// skipped.  Triangles in one plane are then merged: a triangle joins the first facet whose plane holds its first
// vertex and whose normal is parallel to its own, or starts a new facet.  Every comparison is within tol; three
// collinear points (squared norm of the cross product <= tol) are refused.
inline std::vector<std::vector<int>> convex_hull(const std::vector<HullPoint> &pts, double tol = kHullTolerance) {
  using namespace hull_detail;
  const int n = (int)pts.size();
  HullPoint mean = {0.0, 0.0, 0.0};
  for (auto &p : pts)
    for (int k = 0; k < 3; k++) mean[k] += p[k];
  for (int k = 0; k < 3; k++) mean[k] /= (double)n;

  struct Plane {
    HullPoint normal;
    int anchor;  // a vertex in the plane
  };
  std::vector<std::array<int, 3>> tris;
  std::vector<HullPoint> tri_normals;
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++)
      for (int k = j + 1; k < n; k++) {
        HullPoint nrm = cross(sub(pts[j], pts[i]), sub(pts[k], pts[i]));
        const double len2 = dot(nrm, nrm);
        if (!(len2 > tol)) throw LayoutFailure{1 /* EARHIP_INVALID_ARGUMENT */, "collinear points in convex hull"};
        const double len = std::sqrt(len2);
        for (int q = 0; q < 3; q++) nrm[q] /= len;
        const double side = dot(nrm, sub(mean, pts[i]));
        if (std::fabs(side) < tol) continue;
        bool all_inside = true;
        for (int q = 0; q < n && all_inside; q++) {
          const double d = dot(nrm, sub(pts[q], pts[i]));
          all_inside = side > 0 ? d > -tol : d < tol;
        }
        if (all_inside) tris.push_back({i, j, k}), tri_normals.push_back(nrm);
      }

  std::vector<std::vector<int>> facets;
  std::vector<Plane> planes;
  for (size_t t = 0; t < tris.size(); t++) {
    size_t f = 0;
    for (; f < facets.size(); f++) {
      const HullPoint x = cross(planes[f].normal, tri_normals[t]);
      if (std::fabs(dot(sub(pts[tris[t][0]], pts[planes[f].anchor]), planes[f].normal)) < tol && dot(x, x) < tol) break;
    }
    if (f == facets.size()) {
      facets.emplace_back();
      planes.push_back({tri_normals[t], tris[t][0]});
    }
    for (int v : tris[t])
      if (std::find(facets[f].begin(), facets[f].end(), v) == facets[f].end()) facets[f].push_back(v);
    std::sort(facets[f].begin(), facets[f].end());
    planes[f].anchor = facets[f][0];  // (libear measures from the facet's lowest vertex)
  }
  return facets;
}

// the hull of a layout's augmented set at its nominal positions: what a definition's facet list is made of
inline std::vector<std::vector<int>> nominal_hull(const LayoutEntry &L, double tol = kHullTolerance) {
  std::vector<HullPoint> pts;
  for (auto &v : augment_layout(L, nullptr, nullptr)) pts.push_back(aug_point(v));
  return convex_hull(pts, tol);
}

}  // namespace earhip
