// libear_amd/csrc/allo_objects.h alone, compiled by g++ without HIP: the factorised extent (60 terms per loudspeaker) against
// the triple sum over every grid source that it never forms, here written out with allo.h's pan_position at each source; the
// bit rule for plain rows; lock and divergence on tables written out here (2 channels with two flat axes, 0+5+0 with one,
// 4+5+1, and 32 channels with 11 LFEs).  Run under ASan + UBSan by tests/test_allo_objects_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "allo_objects.h"

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

struct Element {
  double x, y, z, width, height, depth;
  bool lock;
  double max_distance, divergence, range;
  uint32_t mask;
};

// the core, as the host form drives it
static std::vector<double> core_gains(const Table &t, const Extras &e, const Element &m) {
  Object o;
  prepare_object(t, e, m.x, m.y, m.z, m.width, m.height, m.depth, m.lock, m.max_distance, m.divergence, m.range, m.mask, o);
  double w[kMaxChannels][3], G[kMaxChannels][3], sum[3] = {0.0, 0.0, 0.0}, norm[3];
  for (int c = 0; c < t.n; c++) {
    channel_terms(t, e, o, c, w[c], G[c]);
    for (int k = 0; k < 3; k++) sum[k] += G[c][k] * G[c][k];
  }
  for (int k = 0; k < 3; k++) norm[k] = std::sqrt(sum[k]);
  std::vector<double> g(t.n);
  for (int c = 0; c < t.n; c++) g[c] = combine(o, w[c], G[c], norm);
  return g;
}

static std::vector<double> point_weights(const Table &t, double x, double y, double z, uint32_t mask) {
  Gains hit;
  pan_position(t, x, y, z, mask, hit);
  std::vector<double> w(t.n, 0.0);
  for (int s = 0; s < 8; s++)
    if (hit.c[s] >= 0) w[hit.c[s]] = hit.w[s];
  return w;
}

// step 3 of the specification for one position, the sum over every grid source taken term by term
static std::vector<double> brute_position(const Table &t, const Extras &e, const double q[3], const double size[3], uint32_t mask) {
  std::vector<double> w = point_weights(t, q[0], q[1], q[2], mask);
  const double *coord[3] = {t.x, t.y, t.z};
  std::vector<double> grid[3];
  double sum = 0.0, s_max = 0.0;
  int axes = 0;
  for (int k = 0; k < 3; k++) {
    if (e.flat[k]) {
      grid[k].push_back(coord[k][e.order[0]]);
      continue;
    }
    for (int j = 0; j < 20; j++) grid[k].push_back((2 * j - 19) / 19.0);
    const double s = std::fmin(size[k], 1.0);
    sum += s, axes++, s_max = std::fmax(s_max, s);
  }
  if (s_max == 0.0) return w;
  const double s_eff = sum / axes, p = s_eff <= 0.5 ? 6.0 : 6.0 - 8.0 * (s_eff - 0.5), alpha = std::fmin(s_max / 0.2, 1.0);
  auto F = [&](int k, double c) {
    if (e.flat[k]) return 1.0;
    const double o = std::fmin(std::fmax(q[k], -1.0), 1.0), h = std::fmax(size[k], 0.1), u = std::fmax(std::fabs(c - o), h) / h;
    return std::pow(10.0, -5.0625 * (u * u * u * u - 1.0));
  };
  std::vector<double> G(t.n, 0.0);
  for (double cx : grid[0])
    for (double cy : grid[1])
      for (double cz : grid[2]) {
        const double f = F(0, cx) * F(1, cy) * F(2, cz);
        const std::vector<double> ws = point_weights(t, cx, cy, cz, mask);
        for (int c = 0; c < t.n; c++) G[c] += std::pow(f * ws[c], p);
      }
  double total = 0.0;
  for (int c = 0; c < t.n; c++) G[c] = std::pow(G[c], 1.0 / p), total += G[c] * G[c];
  for (int c = 0; c < t.n; c++) {
    const double ghat = G[c] / std::sqrt(total);
    w[c] = std::sqrt((1.0 - alpha) * w[c] * w[c] + alpha * ghat * ghat);
  }
  return w;
}

static std::vector<double> brute_gains(const Table &t, const Extras &e, const Element &m) {
  double x = m.x, y = m.y, z = m.z;
  if (m.lock) {
    double least = HUGE_VAL;
    for (int k = 0; k < e.n_order; k++) {
      const double d = lock_distance(t, e.order[k], x, y, z);
      if (d < m.max_distance + 1e-10) least = std::fmin(least, d);
    }
    for (int k = 0; k < e.n_order; k++) {
      const int c = e.order[k];
      const double d = lock_distance(t, c, x, y, z);
      if (d < m.max_distance + 1e-10 && d < least + 1e-10) {
        x = t.x[c], y = t.y[c], z = t.z[c];
        break;
      }
    }
  }
  const double size[3] = {m.width, m.depth, m.height};
  const double q0[3] = {x, y, z}, q1[3] = {x - m.range, y, z}, q2[3] = {x + m.range, y, z};
  if (m.divergence == 0.0) return brute_position(t, e, q0, size, m.mask);
  const double v = m.divergence, wt[3] = {(1 - v) / (1 + v), v / (1 + v), v / (1 + v)};
  const std::vector<double> a = brute_position(t, e, q0, size, m.mask), b = brute_position(t, e, q1, size, m.mask),
                            c = brute_position(t, e, q2, size, m.mask);
  std::vector<double> g(t.n);
  for (int i = 0; i < t.n; i++) g[i] = std::sqrt(wt[0] * a[i] * a[i] + wt[1] * b[i] * b[i] + wt[2] * c[i] * c[i]);
  return g;
}

static unsigned g_state = 12345;
static double uniform(double lo, double hi) {
  g_state = g_state * 1664525u + 1013904223u;
  return lo + (hi - lo) * ((g_state >> 8) / 16777216.0);
}
static unsigned pick(unsigned n) { return (unsigned)uniform(0.0, (double)n) % n; }

static void compare(const Table &t, const char *what, int n_elements) {
  const Extras e = make_extras(t);
  const double sizes[7] = {0.0, 0.03, 0.1, 0.2, 0.5, 1.0, 1.7};
  const uint32_t all = t.n >= 32 ? ~0u : (1u << t.n) - 1u;
  const uint32_t masks[4] = {0u, all, 0x55555555u & all, 0x0f0f00f1u & all};
  double worst = 0.0;
  for (int i = 0; i < n_elements; i++) {
    Element m = {uniform(-1.3, 1.3), uniform(-1.3, 1.3), uniform(-1.3, 1.3), 0, 0, 0, false, HUGE_VAL, 0, 0, masks[pick(4)]};
    if (i % 8 == 0) m.x = 0.0, m.y = 0.0, m.z = 0.0;
    if (i % 4 != 0) m.width = sizes[pick(7)], m.height = sizes[pick(7)], m.depth = sizes[pick(7)];
    if (i % 3 == 0) m.lock = true, m.max_distance = i % 2 ? HUGE_VAL : 0.9;
    if (i % 5 < 2) m.divergence = i % 5 ? 1.0 : 0.4, m.range = sizes[pick(7)];
    const std::vector<double> got = core_gains(t, e, m), want = brute_gains(t, e, m);
    double power = 0.0;
    for (int c = 0; c < t.n; c++) {
      const double err = std::fabs(got[c] - want[c]);
      worst = std::fmax(worst, err);
      CHECK(err <= 1e-12);
      CHECK(((t.real >> c) & 1u) || got[c] == 0.0);
      power += got[c] * got[c];
    }
    CHECK(std::fabs(power - 1.0) <= 1e-12);
    if (!m.lock && m.divergence == 0.0 && m.width == 0.0 && m.height == 0.0 && m.depth == 0.0) {
      const std::vector<double> w = point_weights(t, m.x, m.y, m.z, m.mask);  // plain rows: group T's bits
      for (int c = 0; c < t.n; c++) CHECK(std::memcmp(&got[c], &w[c], sizeof(double)) == 0);
    }
  }
  std::printf("%s: %d elements, worst difference to the triple sum %.3g\n", what, n_elements, worst);
}

int main() {
  const double s = std::sqrt(2.0) - 1.0;
  const Table two = table_of({{-1, 1, 0, false}, {1, 1, 0, false}});
  const Table five = table_of({{-1, 1, 0, false}, {1, 1, 0, false}, {0, 1, 0, false}, {0, 0, 0, true}, {-1, -1, 0, false}, {1, -1, 0, false}});
  const Table four51 = table_of({{-1, 1, 0, false}, {1, 1, 0, false}, {0, 1, 0, false}, {0, 0, 0, true}, {-1, -1, 0, false},
                                 {1, -1, 0, false}, {-1, 1, 1, false}, {1, 1, 1, false}, {-1, -1, 1, false}, {1, -1, 1, false},
                                 {0, 1, -1, false}});
  std::vector<Speaker> wide;  // 21 loudspeakers in three planes and 11 LFEs in between
  for (int i = 0; i < 21; i++) {
    const double xs[4] = {-1.0, -s, s, 1.0}, ys[3] = {1.0, 0.0, -1.0};
    wide.push_back({xs[i % 4], ys[(i / 4) % 3], i < 12 ? 0.0 : (i < 18 ? 1.0 : -1.0), false});
    if (i % 2 == 1 || i == 20) wide.push_back({0, 0, 0, true});
  }
  const Table t32 = table_of(wide);
  CHECK(t32.n == 32);

  Extras e = make_extras(two);
  CHECK(e.n_order == 2 && e.flat[0] == 0 && e.flat[1] == 1 && e.flat[2] == 1 && e.order[0] == 0 && e.order[1] == 1);
  e = make_extras(five);
  CHECK(e.n_order == 5 && e.flat[2] == 1 && e.flat[0] == 0 && e.flat[1] == 0);
  CHECK(e.order[0] == 2 && e.order[1] == 0 && e.order[2] == 1 && e.order[3] == 4 && e.order[4] == 5);
  e = make_extras(four51);
  CHECK(e.order[0] == 2 && e.order[5] == 10 && e.order[6] == 6);  // z = 0, then z = -1, then z = 1

  CHECK(objects_valid(0, 0, 0, HUGE_VAL, 0, 0) && objects_valid(1.7, 0, 3, 0, 1, 2));
  CHECK(!objects_valid(-1e-9, 0, 0, 1, 0, 0) && !objects_valid(0, NAN, 0, 1, 0, 0) && !objects_valid(0, 0, HUGE_VAL, 1, 0, 0));
  CHECK(!objects_valid(0, 0, 0, -1e-9, 0, 0) && !objects_valid(0, 0, 0, NAN, 0, 0));
  CHECK(!objects_valid(0, 0, 0, 1, -1e-9, 0) && !objects_valid(0, 0, 0, 1, 1.0000001, 0) && !objects_valid(0, 0, 0, 1, NAN, 0));
  CHECK(!objects_valid(0, 0, 0, 1, 0, -1e-9) && !objects_valid(0, 0, 0, 1, 0, NAN) && !objects_valid(0, 0, 0, 1, 0, HUGE_VAL));

  compare(two, "2 channels", 60);
  compare(five, "0+5+0", 60);
  compare(four51, "4+5+1", 40);
  compare(t32, "32 channels", 24);
  std::printf("%ld checked, %ld failed\n", g_checked, g_failed);
  return g_failed != 0;
}
