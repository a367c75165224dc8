// test_hull.cpp — libear_amd/csrc/layout_registry.h on the CPU (plain g++, no device): the convex hull of a layout's
// augmented loudspeaker set.  The facet tables of layout_table.h were made by libear's own convex_hull, so they are the
// known answers: for each of the nine BS.2051 layouts that have a table the hull of the nominal augmented set equals the
// table as a set of sets, at tolerances 1e-6, 1e-5 and 1e-4 (libear's TEST_CASE("hull") makes the same check at its
// default).  Plus the small shapes where the merge of coplanar triangles and the collinearity refusal can be read off.
#include <cstdio>
#include <set>
#include <vector>

#include "layout_registry.h"

using namespace earhip;

static int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      failures++;                             \
      std::printf("FAILED %s: ", #cond);      \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
    }                                         \
  } while (0)

using FacetSet = std::set<std::set<int>>;

static FacetSet as_sets(const std::vector<std::vector<int>> &facets) {
  FacetSet s;
  for (auto &f : facets) s.insert(std::set<int>(f.begin(), f.end()));
  return s;
}

static FacetSet table_sets(const LayoutEntry &L) {
  FacetSet s;
  for (const int *f = L.facets; *f; f += 1 + *f) s.insert(std::set<int>(f + 1, f + 1 + *f));
  return s;
}

int main() {
  int tabled = 0;
  for (int i = 0; i < kNumLayouts; i++) {
    const LayoutEntry &L = kLayouts[i];
    if (!L.facets) continue;
    tabled++;
    const FacetSet want = table_sets(L);
    for (double tol : {1e-6, 1e-5, 1e-4}) {
      const std::vector<std::vector<int>> got = nominal_hull(L, tol);
      CHECK(as_sets(got) == want, "%s at tol %g: %zu facets, the table has %zu", L.name, tol, got.size(), want.size());
      CHECK(as_sets(got).size() == got.size(), "%s at tol %g: a facet appears twice", L.name, tol);
      for (auto &f : got)
        for (size_t k = 1; k < f.size(); k++) CHECK(f[k - 1] < f[k], "%s: facet vertices are not ascending", L.name);
    }
    // the augmented set itself: the loudspeakers that are not LFE first, the virtual ones last, every index of the table in range
    const std::vector<AugVertex> verts = augment_layout(L, nullptr, nullptr);
    int n_real = 0;
    for (int c = 0; c < L.n; c++) n_real += !L.channels[c].is_lfe;
    for (int c = 0; c < n_real; c++) CHECK(verts[c].mix_to == c && verts[c].pole == 0, "%s: vertex %d", L.name, c);
    CHECK(verts.back().pole != 0 && verts[n_real].pole == 0, "%s: order of the augmented set", L.name);
    for (auto &f : want)
      for (int v : f) CHECK(v >= 0 && v < (int)verts.size(), "%s: table vertex %d out of range", L.name, v);
  }
  CHECK(tabled == 9, "%d layouts with a table", tabled);

  // a cube: 12 hull triangles in 6 planes merge into 6 quads; an octahedron keeps its 8 triangles
  std::vector<HullPoint> cube;
  for (int x = -1; x <= 1; x += 2)
    for (int y = -1; y <= 1; y += 2)
      for (int z = -1; z <= 1; z += 2) cube.push_back({(double)x, (double)y, (double)z});
  const auto cube_hull = convex_hull(cube);
  CHECK(cube_hull.size() == 6, "cube: %zu facets", cube_hull.size());
  for (auto &f : cube_hull) CHECK(f.size() == 4, "cube: a facet of %zu", f.size());
  const std::vector<HullPoint> octa = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
  // (its three diagonals pass through the mean, but no three of its vertices are collinear)
  const auto octa_hull = convex_hull(octa);
  CHECK(octa_hull.size() == 8, "octahedron: %zu facets", octa_hull.size());
  for (auto &f : octa_hull) CHECK(f.size() == 3, "octahedron: a facet of %zu", f.size());

  // three points on a line, and a point given twice, are refused
  for (int twice = 0; twice < 2; twice++) {
    std::vector<HullPoint> bad = octa;
    bad.push_back(twice ? HullPoint{1, 0, 0} : HullPoint{0, 0, 0});
    bool refused = false;
    try {
      (void)convex_hull(bad);
    } catch (const LayoutFailure &e) {
      refused = e.status == 1 && e.msg == "collinear points in convex hull";
    }
    CHECK(refused, "collinear points (case %d) were not refused", twice);
  }

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("hull: all checks passed\n");
  return 0;
}
