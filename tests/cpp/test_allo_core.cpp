// libear_amd/csrc/allo.h alone, compiled by g++ without HIP: the known answers of include/earhip.h group T on tables written
// out here (0+5+0, 4+5+0, 3+7+0 and 9+10+3 as the specification's table gives them), a layout of 2 channels and one of 32,
// masks, clipping, and the split into direct and diffuse rows.  Run under ASan + UBSan by tests/test_allo_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "allo.h"

using namespace earhip::allo;

static long g_checked = 0, g_failed = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    g_checked++;                                                    \
    if (!(cond)) {                                                  \
      g_failed++;                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                               \
  } while (0)

struct Speaker {
  double x, y, z;
  bool lfe;
};

static Table table_of(const std::vector<Speaker> &sp) {
  Table t;
  std::memset(&t, 0, sizeof t);
  t.n = (int)sp.size();
  for (int c = 0; c < t.n; c++) {
    if (sp[c].lfe) continue;
    t.real |= 1u << c;
    t.x[c] = sp[c].x, t.y[c] = sp[c].y, t.z[c] = sp[c].z;
  }
  return t;
}

// the direct row of one position, and the checks every row passes: at most 8 non-zero, power gain^2, LFE columns +0
static std::vector<float> row_of(const Table &t, double x, double y, double z, uint32_t mask = 0, double gain = 1.0,
                                 double diffuse = 0.0, std::vector<float> *diffuse_row = nullptr) {
  CHECK(position_valid(x, y, z, gain, diffuse));
  Gains g;
  pan_position(t, x, y, z, mask, g);
  std::vector<float> direct(t.n, -1.0f), diff(t.n, -1.0f);
  write_row(t, g, gain, direct_factor(diffuse), direct.data());
  write_row(t, g, gain, diffuse_factor(diffuse), diff.data());
  double power = 0.0;
  int nonzero = 0;
  for (int c = 0; c < t.n; c++) {
    power += (double)direct[c] * direct[c] + (double)diff[c] * diff[c];
    nonzero += direct[c] != 0.0f || diff[c] != 0.0f;
    if (!((t.real >> c) & 1u)) {
      uint32_t bits[2];
      std::memcpy(&bits[0], &direct[c], 4), std::memcpy(&bits[1], &diff[c], 4);
      CHECK(bits[0] == 0 && bits[1] == 0);
    }
  }
  CHECK(nonzero >= 1 && nonzero <= 8);
  CHECK(std::fabs(power - gain * gain) <= 1e-6 * gain * gain);
  if (diffuse_row) *diffuse_row = diff;
  return direct;
}

// row == the listed (channel, value) pairs and exactly 0 elsewhere
static bool is_row(const std::vector<float> &row, std::vector<std::pair<int, float>> want) {
  std::vector<float> full(row.size(), 0.0f);
  for (auto &w : want) full[w.first] = w.second;
  return std::memcmp(full.data(), row.data(), sizeof(float) * row.size()) == 0;
}

int main() {
  const double s = std::sqrt(2.0) - 1.0;
  const float r2 = (float)std::sqrt(0.5), r8 = (float)std::sqrt(0.125);
  const Speaker LFE = {0, 0, 0, true};
  // 0+5+0: M+030 M-030 M+000 LFE1 M+110 M-110
  const Table t050 = table_of({{-1, 1, 0, false}, {1, 1, 0, false}, {0, 1, 0, false}, LFE, {-1, -1, 0, false}, {1, -1, 0, false}});
  CHECK(is_row(row_of(t050, 0, 1, 0), {{2, 1.0f}}));
  CHECK(is_row(row_of(t050, -0.5, 1, 0), {{0, r2}, {2, r2}}));
  CHECK(is_row(row_of(t050, 0, 0, 0), {{2, r2}, {4, 0.5f}, {5, 0.5f}}));
  CHECK(is_row(row_of(t050, 0, 0, 3), {{2, r2}, {4, 0.5f}, {5, 0.5f}}));
  CHECK(is_row(row_of(t050, 0, 1, 0, 1u << 2), {{0, r2}, {1, r2}}));
  CHECK(is_row(row_of(t050, 0, 1, 0, 1u << 3), {{2, 1.0f}}));                  // an LFE bit is ignored
  CHECK(is_row(row_of(t050, 0, 1, 0, 0xffffffc0u), {{2, 1.0f}}));              // bits beyond the layout are ignored
  CHECK(is_row(row_of(t050, 0, 1, 0, 0x37u), {{2, 1.0f}}));                    // every loudspeaker excluded: none is
  CHECK(is_row(row_of(t050, -0.0, 1, -0.0), {{2, 1.0f}}));
  CHECK(is_row(row_of(t050, 7, 7, -7), {{1, 1.0f}}));                          // clipped to the corner
  // 4+5+0: ... U+030 U-030 U+110 U-110
  const Table t450 = table_of({{-1, 1, 0, false}, {1, 1, 0, false}, {0, 1, 0, false}, LFE, {-1, -1, 0, false}, {1, -1, 0, false},
                               {-1, 1, 1, false}, {1, 1, 1, false}, {-1, -1, 1, false}, {1, -1, 1, false}});
  CHECK(is_row(row_of(t450, 0, 0, 0.5), {{2, 0.5f}, {4, r8}, {5, r8}, {6, r8}, {7, r8}, {8, r8}, {9, r8}}));
  // 3+7+0: M+000 M+030 M-030 U+045 U-045 M+090 M-090 M+135 M-135 UH+180 LFE1 LFE2
  const Table t370 = table_of({{0, 1, 0, false}, {-1, 1, 0, false}, {1, 1, 0, false}, {-1, 1, 1, false}, {1, 1, 1, false},
                               {-1, 0, 0, false}, {1, 0, 0, false}, {-1, -1, 0, false}, {1, -1, 0, false}, {0, -1, 1, false}, LFE, LFE});
  CHECK(is_row(row_of(t370, 0.5, -1, 1), {{9, 1.0f}}));
  CHECK(is_row(row_of(t370, 0, 0, 0.5), {{5, 0.5f}, {6, 0.5f}, {9, 0.5f}, {3, r8}, {4, r8}}));
  // 9+10+3: M+060 M-060 M+000 LFE1 M+135 M-135 M+030 M-030 M+180 LFE2 M+090 M-090 U+045 U-045 U+000 T+000 U+135 U-135 U+090
  // U-090 U+180 B+000 B+045 B-045
  const Table t9103 = table_of(
      {{-1, s, 0, false},  {1, s, 0, false},  {0, 1, 0, false},  LFE,               {-1, -1, 0, false}, {1, -1, 0, false},
       {-s, 1, 0, false},  {s, 1, 0, false},  {0, -1, 0, false}, LFE,               {-1, 0, 0, false},  {1, 0, 0, false},
       {-1, 1, 1, false},  {1, 1, 1, false},  {0, 1, 1, false},  {0, 0, 1, false},  {-1, -1, 1, false}, {1, -1, 1, false},
       {-1, 0, 1, false},  {1, 0, 1, false},  {0, -1, 1, false}, {0, 1, -1, false}, {-1, 1, -1, false}, {1, 1, -1, false}});
  CHECK(is_row(row_of(t9103, 0, 0, 1), {{15, 1.0f}}));
  CHECK(is_row(row_of(t9103, -1, 1, 0), {{6, 1.0f}}));  // no loudspeaker at that corner: clipped along x within the row
  CHECK(is_row(row_of(t9103, 0, 0, 0), {{10, r2}, {11, r2}}));
  for (int c = 0; c < t9103.n; c++)
    if ((t9103.real >> c) & 1u) CHECK(is_row(row_of(t9103, t9103.x[c], t9103.y[c], t9103.z[c], 0, 0.75), {{c, 0.75f}}));
  // the split: gain and diffuse
  {
    std::vector<float> diff;
    const std::vector<float> direct = row_of(t050, 0, 0, 0, 0, 2.0, 0.36, &diff);
    CHECK(std::fabs(direct[4] - 0.8f) <= 1.2e-7f && std::fabs(diff[4] - 0.6f) <= 1.2e-7f);
    CHECK(direct[3] == 0.0f && diff[3] == 0.0f);
    row_of(t050, 0.3, -0.2, 0.1, 0, -1.5, 1.0, &diff);
    row_of(t050, 0.3, -0.2, 0.1, 0, 1.5, 0.0, &diff);
    CHECK(is_row(diff, {}));
  }
  CHECK(!position_valid(NAN, 0, 0, 1, 0) && !position_valid(0, INFINITY, 0, 1, 0) && !position_valid(0, 0, -INFINITY, 1, 0));
  CHECK(!position_valid(0, 0, 0, NAN, 0) && !position_valid(0, 0, 0, 1, NAN) && !position_valid(0, 0, 0, 1, -1e-9));
  CHECK(!position_valid(0, 0, 0, 1, 1.0000001) && position_valid(0, 0, 0, -1e300, 1.0));
  // 2 channels: one row
  const Table t2 = table_of({{-1, 1, 0, false}, {1, 1, 0, false}});
  CHECK(is_row(row_of(t2, 0, -5, 2), {{0, r2}, {1, r2}}));
  CHECK(is_row(row_of(t2, -1, 0, 0), {{0, 1.0f}}));
  CHECK(is_row(row_of(t2, 0, 0, 0, 1u << 1), {{0, 1.0f}}));
  // 32 channels: a 3 x 3 x 3 grid without its centre (26 loudspeakers) and 6 LFE channels spread among them, bit 31 in use
  {
    std::vector<Speaker> sp;
    for (int k = 0; k < 27; k++) {
      if (k == 13) continue;
      if (sp.size() % 5 == 2 && sp.size() < 30) sp.push_back(LFE);
      sp.push_back({(double)(k % 3 - 1), (double)(k / 3 % 3 - 1), (double)(k / 9 - 1), false});
    }
    while (sp.size() < 32) sp.insert(sp.begin() + 7, LFE);
    CHECK(sp.size() == 32 && !sp[31].lfe);
    const Table t32 = table_of(sp);
    for (int c = 0; c < 32; c++)
      if (!sp[c].lfe) CHECK(is_row(row_of(t32, sp[c].x, sp[c].y, sp[c].z), {{c, 1.0f}}));
    // the centre: the middle plane's middle row has two loudspeakers
    const std::vector<float> centre = row_of(t32, 0, 0, 0);
    int nz = 0;
    for (float v : centre) nz += v != 0.0f;
    CHECK(nz == 2);
    // an interior point: 8 loudspeakers; with the top corner (channel 31) excluded the row is clipped to its neighbour
    nz = 0;
    for (float v : row_of(t32, 0.3, 0.6, 0.2)) nz += v != 0.0f;
    CHECK(nz == 8);
    CHECK(row_of(t32, 1, 1, 1)[31] == 1.0f && row_of(t32, 1, 1, 1, 1u << 31)[31] == 0.0f);
    unsigned seed = 1;
    for (int k = 0; k < 2000; k++) {
      double p[3];
      for (double &v : p) seed = seed * 1664525u + 1013904223u, v = (seed >> 8) / 16777216.0 * 2.6 - 1.3;
      seed = seed * 1664525u + 1013904223u;
      row_of(t32, p[0], p[1], p[2], k % 3 ? seed : 0u, 0.5 + k * 1e-3, (k % 11) / 10.0);
    }
  }
  std::printf("%ld checked, %ld failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
