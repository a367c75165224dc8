// ear/hip_timeline.hpp: the block timeline in the C++14 mirror, written against the mirror headers and the C ABI
// (include/earhip.h group W) alone.  Compiles as C++14 with -Wall -Wextra -Werror.  `test_timeline host` runs what needs no
// device: timelinePoints and timelineWindow on cases worked out by hand from the header's rule, and their refusals.  Without an
// argument ObjectsProgramme::bind runs too, on a GPU: a polar track, a Cartesian track and a stepped bed, bound whole, by
// window and behind a reproduction screen, must render bit for bit as the same curves made by hand — the calculators and the
// screen stage called directly, timelinePoints, one set_object_points call per object.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include <ear/bs2051.hpp>
#include <ear/decorrelate.hpp>
#include <ear/hip_timeline.hpp>

#include "dropin_check.h"

using namespace ear;
using ear::dsp::ObjectsRenderer;
using ear::hip::BlockTiming;
using ear::hip::TimelineMode;
using ear::hip::TimelinePoints;

typedef std::vector<std::pair<int64_t, int32_t>> Points;

static Points zip(const TimelinePoints &p) {
  Points out;
  for (size_t k = 0; k < p.times.size() && k < p.source.size(); k++) out.emplace_back(p.times[k], p.source[k]);
  return out;
}

static void test_points() {
  // a gap, a jump of 2 behind it, a contiguous block without one
  const std::vector<BlockTiming> gap{{0, 10}, {15, 8}, {30, 6, true, 2}, {36, 4}};
  CHECK(zip(hip::timelinePoints(TimelineMode::Interpolated, 0, gap)) ==
        (Points{{0, -1}, {0, 0}, {10, 0}, {10, -1}, {15, -1}, {15, 0}, {23, 1}, {23, -1}, {30, -1}, {30, 1}, {32, 2}, {36, 2}, {40, 3}, {40, -1}}));
  CHECK(hip::timelineWindow(TimelineMode::Interpolated, 0, gap) == std::make_pair(0, 3));
  // the window [16, 20): blocks 0 and 1, as if they were the whole list
  CHECK(hip::timelineWindow(TimelineMode::Interpolated, 0, gap, 16, 20) == std::make_pair(0, 1));
  CHECK(zip(hip::timelinePoints(TimelineMode::Interpolated, 0, gap, 16, 20)) ==
        (Points{{0, -1}, {0, 0}, {10, 0}, {10, -1}, {15, -1}, {15, 0}, {23, 1}, {23, -1}}));
  // jumps of 3 and 1, contiguous
  const std::vector<BlockTiming> jumps{{0, 10}, {10, 8, true, 3}, {18, 5, true, 1}};
  CHECK(zip(hip::timelinePoints(TimelineMode::Interpolated, 0, jumps)) ==
        (Points{{0, -1}, {0, 0}, {10, 0}, {13, 1}, {18, 1}, {19, 2}, {23, 2}, {23, -1}}));
  // a jump into an open end: nothing after the ramp
  CHECK(zip(hip::timelinePoints(TimelineMode::Interpolated, 0, {{0, 10}, {10, -1, true, 6}})) == (Points{{0, -1}, {0, 0}, {10, 0}, {16, 1}}));
  // a negative start
  CHECK(zip(hip::timelinePoints(TimelineMode::Interpolated, -100, {{4, 10}, {14, 5, true, 2}, {25, 5}})) ==
        (Points{{-96, -1}, {-96, 0}, {-86, 0}, {-84, 1}, {-81, 1}, {-81, -1}, {-75, -1}, {-75, 1}, {-70, 2}, {-70, -1}}));
  // stepped, with gaps and an open end: steps only, the jump of block 1 is not read
  CHECK(zip(hip::timelinePoints(TimelineMode::Stepped, 5, {{0, 10}, {12, 7, true, 3}, {19, 9}, {40, -1}})) ==
        (Points{{5, -1}, {5, 0}, {15, 0}, {15, -1}, {17, -1}, {17, 1}, {24, 1}, {24, 2}, {33, 2}, {33, -1}, {45, -1}, {45, 3}}));
  // one block, and one open-ended block
  CHECK(zip(hip::timelinePoints(TimelineMode::Interpolated, 0, {{3, 10}})) == (Points{{3, -1}, {3, 0}, {13, 0}, {13, -1}}));
  CHECK(zip(hip::timelinePoints(TimelineMode::Interpolated, 0, {{3, -1}})) == (Points{{3, -1}, {3, 0}}));
  // refusals: ear::invalid_argument, the message naming the block
  CHECK_THROWS_AS(hip::timelinePoints(TimelineMode::Interpolated, 0, {}), ear::invalid_argument);
  CHECK_THROWS_AS(hip::timelinePoints(TimelineMode::Interpolated, 0, {{0, 10}, {9, 5}}), ear::invalid_argument);
  CHECK_THROWS_AS(hip::timelinePoints(TimelineMode::Interpolated, 0, {{0, 10}, {10, 5, true, 6}}), ear::invalid_argument);
  CHECK_THROWS_AS(hip::timelinePoints(TimelineMode::Interpolated, 0, {{0, 10}, {10, -1}}), ear::invalid_argument);
  CHECK_THROWS_AS(hip::timelinePoints(TimelineMode::Interpolated, 0, {{0, -1}, {10, 5}}), ear::invalid_argument);
  CHECK_THROWS_AS(hip::timelinePoints(TimelineMode::Interpolated, 0, {{0, 0}}), ear::invalid_argument);
  CHECK_THROWS_AS(hip::timelinePoints(TimelineMode::Interpolated, 0, {{-1, 5}}), ear::invalid_argument);
  CHECK_THROWS_AS(hip::timelinePoints((TimelineMode)2, 0, {{0, 5}}), ear::invalid_argument);
  CHECK_THROWS_AS(hip::timelineWindow(TimelineMode::Interpolated, 0, gap, 5, 5), ear::invalid_argument);
  std::string text;
  try {
    hip::timelinePoints(TimelineMode::Interpolated, 0, {{0, 10}, {10, 5}, {14, 5}});
  } catch (const ear::invalid_argument &e) {
    text = e.what();
  }
  CHECK(text.find("block 2") != std::string::npos);
}

// ---- ObjectsProgramme::bind == the calculators, the screen stage and set_object_points by hand ----------------------------
static ObjectsTypeMetadata polar(double az, double el, double width = 0.0, double diffuse = 0.0) {
  ObjectsTypeMetadata m;
  m.position = PolarPosition(az, el, 1.0);
  m.width = width, m.diffuse = diffuse;
  return m;
}
static ObjectsTypeMetadata cart(double x, double y, double z, double diffuse = 0.0) {
  ObjectsTypeMetadata m;
  m.position = CartesianPosition(x, y, z);
  m.cartesian = true;
  m.diffuse = diffuse;
  return m;
}

struct Scene {
  std::vector<std::pair<BlockTiming, ObjectsTypeMetadata>> polar_blocks, cart_blocks;
  std::vector<ScreenEdgeLock> polar_locks, cart_locks;
  std::vector<BlockTiming> bed_timing;
  std::vector<std::vector<float>> bed_rows;
  int64_t polar_start = 7, cart_start = -30, bed_start = 0;
};

static Scene scene(bool with_screen) {
  Scene s;
  s.polar_blocks = {{BlockTiming(0, 90), polar(30.0, 0.0)},
                    {BlockTiming(90, 70, true, 16), polar(-40.0, 10.0, 20.0, 0.5)},
                    {BlockTiming(200, 100), polar(110.0, 0.0, 0.0, 0.25)},
                    {BlockTiming(300, 150, true, 0), polar(0.0, 25.0)}};
  s.cart_blocks = {{BlockTiming(40, 100), cart(-0.5, 1.0, 0.0)},
                   {BlockTiming(140, 128), cart(0.7, 0.2, 0.4, 0.3)},
                   {BlockTiming(268, 60, true, 30), cart(0.0, -1.0, 0.0)},
                   {BlockTiming(340, -1, true, 64), cart(1.0, 1.0, 1.0, 1.0)}};
  s.polar_locks.assign(4, ScreenEdgeLock()), s.cart_locks.assign(4, ScreenEdgeLock());
  if (with_screen) {
    s.polar_blocks[1].second.screenRef = true;
    s.polar_locks[3].horizontal = std::string("left");
    s.cart_blocks[0].second.screenRef = true;
    s.cart_locks[2].vertical = std::string("top");
  }
  s.bed_timing = {BlockTiming(0, 256), BlockTiming(256, 100), BlockTiming(400, -1)};
  s.bed_rows = {{0, 0, 1, 0, 0, 0}, {0, 0, 0.5f, 0.25f, 0, 0}, {0.125f, 0, 0, 0, 0, 1}};
  return s;
}

typedef std::vector<std::vector<float>> Rows;

static void set_by_hand(ObjectsRenderer &r, size_t object, TimelineMode mode, int64_t start, const std::vector<BlockTiming> &timing,
                        const Rows &direct, const Rows &diffuse, int64_t t0, int64_t t1) {
  const TimelinePoints p = hip::timelinePoints(mode, start, timing, t0, t1);
  const std::vector<float> zero(6, 0.0f);
  Rows d, f;
  for (int32_t src : p.source) d.push_back(src < 0 ? zero : direct[src]), f.push_back(src < 0 ? zero : diffuse[src]);
  r.set_object_points(object, p.times, d, f);
}

static std::vector<std::vector<float>> render(ObjectsRenderer &r, size_t n_blocks, size_t first_block) {
  const size_t M = 3, N = 6, B = 64;
  std::vector<std::vector<float>> in(M, std::vector<float>(n_blocks * B)), out(N, std::vector<float>(n_blocks * B));
  for (size_t m = 0; m < M; m++)
    for (size_t i = 0; i < n_blocks * B; i++) {
      const size_t n = first_block * B + i;
      in[m][i] = (float)((int)((n * (2 * m + 3) + 5 * m) % 17) - 8) / 8.0f;
    }
  std::vector<const float *> ip(M);
  std::vector<float *> op(N);
  for (size_t m = 0; m < M; m++) ip[m] = in[m].data();
  for (size_t c = 0; c < N; c++) op[c] = out[c].data();
  r.process(n_blocks, ip.data(), op.data());
  return out;
}

static bool same_bits(const std::vector<std::vector<float>> &a, const std::vector<std::vector<float>> &b) {
  if (a.size() != b.size()) return false;
  for (size_t c = 0; c < a.size(); c++)
    if (a[c].size() != b[c].size() || std::memcmp(a[c].data(), b[c].data(), a[c].size() * sizeof(float)) != 0) return false;
  return true;
}

static void test_bind(bool with_screen) {
  const Layout layout = getLayout("0+5+0");
  const Screen reproduction = PolarScreen{1.78, PolarPosition(0.0, 0.0, 1.0), 30.0};
  const Scene s = scene(with_screen);
  const size_t B = 64, T = 8;
  const auto dec = designDecorrelators(layout);
  const int delay = decorrelatorCompensationDelay();

  // by hand: the screen stage and the calculators on each track's blocks, then the points
  std::vector<ObjectsTypeMetadata> pm, cm;
  std::vector<BlockTiming> pt, ct;
  for (auto &b : s.polar_blocks) pt.push_back(b.first), pm.push_back(b.second);
  for (auto &b : s.cart_blocks) ct.push_back(b.first), cm.push_back(b.second);
  if (with_screen) {
    const hip::ScreenHandler handler(reproduction);
    handler.apply(pm, s.polar_locks);
    handler.apply_cartesian(cm, s.cart_locks);
  }
  Rows pd, pf, cd, cf;
  hip::ObjectsGainCalculator polar_calc(layout);
  polar_calc.calculate(pm, pd, pf);
  const hip::AllocentricObjectsGainCalculator cart_calc(layout);
  cart_calc.calculate(cm, cd, cf);
  const Rows bed_diffuse(s.bed_rows.size(), std::vector<float>(6, 0.0f));

  hip::ObjectsProgramme programme = with_screen ? hip::ObjectsProgramme(layout, reproduction) : hip::ObjectsProgramme(layout);
  programme.add_object(0, s.polar_start, s.polar_blocks, s.polar_locks);
  programme.add_object(1, s.cart_start, s.cart_blocks, with_screen ? s.cart_locks : std::vector<ScreenEdgeLock>());
  programme.add_stepped(2, s.bed_start, s.bed_timing, s.bed_rows);
  CHECK(programme.size() == 3);

  const int64_t whole[2][2] = {{hip::kTimelineBegin, hip::kTimelineEnd}, {hip::kTimelineBegin, hip::kTimelineEnd}};
  const int64_t halves[2][2] = {{0, 256}, {256, 512}};
  std::vector<std::vector<float>> first_out;
  for (const auto &windows : {whole, halves}) {
    ObjectsRenderer bound(3, 6, B, dec, delay, T), hand(3, 6, B, dec, delay, T);
    bool same = true, loud = false;
    for (size_t half = 0; half < 2; half++) {
      const int64_t t0 = windows[half][0], t1 = windows[half][1];
      if (half == 0 || windows == halves) {
        programme.bind(bound, t0, t1);
        bound.commit();
        set_by_hand(hand, 0, TimelineMode::Interpolated, s.polar_start, pt, pd, pf, t0, t1);
        set_by_hand(hand, 1, TimelineMode::Interpolated, s.cart_start, ct, cd, cf, t0, t1);
        set_by_hand(hand, 2, TimelineMode::Stepped, s.bed_start, s.bed_timing, s.bed_rows, bed_diffuse, t0, t1);
        hand.commit();
      }
      const auto got = render(bound, T / 2, half * T / 2), want = render(hand, T / 2, half * T / 2);
      same = same && same_bits(got, want);
      for (auto &row : want)
        for (float v : row) loud = loud || v > 0.05f || v < -0.05f;
      if (windows == whole && half == 0) first_out = got;
      if (windows == halves && half == 0) CHECK(same_bits(got, first_out));  // a window's curve is the whole curve inside it
    }
    CHECK(same);
    CHECK(loud);
  }

  // a refused block propagates the calculator's exception and changes no curve: screenRef without a reproduction screen
  if (!with_screen) {
    ObjectsRenderer r(3, 6, B, dec, delay, T), untouched(3, 6, B, dec, delay, T);
    hip::ObjectsProgramme bad(layout);
    bad.add_stepped(2, s.bed_start, s.bed_timing, s.bed_rows);
    std::vector<std::pair<BlockTiming, ObjectsTypeMetadata>> blocks = s.polar_blocks;
    blocks[2].second.screenRef = true;
    bad.add_object(0, s.polar_start, blocks);
    CHECK_THROWS_AS(bad.bind(r), ear::not_implemented);
    CHECK(same_bits(render(r, T, 0), render(untouched, T, 0)));
    // ... and so does a block list the timeline refuses
    hip::ObjectsProgramme overlap(layout);
    overlap.add_stepped(2, s.bed_start, s.bed_timing, s.bed_rows);
    overlap.add_stepped(1, 0, {BlockTiming(0, 10), BlockTiming(5, 10)}, {s.bed_rows[0], s.bed_rows[1]});
    CHECK_THROWS_AS(overlap.bind(r), ear::invalid_argument);
    r.reset(0), untouched.reset(0);
    CHECK(same_bits(render(r, T, 0), render(untouched, T, 0)));
    // a renderer of another width
    ObjectsRenderer narrow(3, 5, B, std::vector<std::vector<float>>(), 0, T);
    CHECK_THROWS_AS(programme.bind(narrow), ear::invalid_argument);
  }
}

int main(int argc, char **argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "host") == 0;
  try {
    test_points();
    if (host_only) return summary("host") ? 1 : 0;
    test_bind(false);
    test_bind(true);
  } catch (const std::exception &e) {
    std::printf("FAILED: unexpected exception: %s\n", e.what());
    g_failed++;
  }
  return summary() ? 1 : 0;
}
