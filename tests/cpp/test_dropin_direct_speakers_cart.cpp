// Drop-in test of ear::hip::DirectSpeakersGainCalculator and ObjectsProgramme::add_direct_speakers (earhip group X): a bed with
// Cartesian positions and screenEdgeLocks, written against the C++14 mirror headers alone.  Expected gains are one-hot vectors,
// the rows of ear::GainCalculatorDirectSpeakers at a position worked out with the mirror's own conversion and screen stage, or
// a programme fed the calculator's rows by hand, so this program needs nothing but libearhip.so and a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include <ear/ear.hpp>
#include <ear/conversion.hpp>
#include <ear/hip_timeline.hpp>

#include "dropin_check.h"

using namespace ear;
using ear::dsp::ObjectsRenderer;
using ear::hip::BlockTiming;

typedef std::vector<float> Gains;
typedef std::vector<std::vector<float>> Rows;

struct BedChannel {
  const char *label;
  double x, y, z;
};
// the 7.1.2 bed of an Atmos-style ADM master
static const BedChannel kBed[10] = {{"RC_L", -1, 1, 0},   {"RC_R", 1, 1, 0},    {"RC_C", 0, 1, 0},    {"RC_LFE", -1, 1, -1},
                                    {"RC_Lss", -1, 0, 0}, {"RC_Rss", 1, 0, 0},  {"RC_Lrs", -1, -1, 0}, {"RC_Rrs", 1, -1, 0},
                                    {"RC_Lts", -1, 0, 1}, {"RC_Rts", 1, 0, 1}};

static std::vector<DirectSpeakersTypeMetadata> atmos_bed() {
  std::vector<DirectSpeakersTypeMetadata> bed;
  for (const BedChannel &b : kBed) {
    DirectSpeakersTypeMetadata tm;
    tm.speakerLabels = {b.label};
    tm.position = CartesianSpeakerPosition(b.x, b.y, b.z);
    if (std::string(b.label) == "RC_LFE") tm.channelFrequency.lowPass = 120.0;
    bed.push_back(tm);
  }
  return bed;
}

static Gains one_hot(const Layout &layout, const std::string &channel) {
  Gains g(layout.channels().size(), 0.0f);
  g[layout.indexForName(channel)] = 1.0f;
  return g;
}

static void test_atmos_bed() {
  const Layout layout = getLayout("0+5+0");
  hip::DirectSpeakersGainCalculator calc(layout);
  GainCalculatorDirectSpeakers libear_calc(layout);
  const std::vector<DirectSpeakersTypeMetadata> bed = atmos_bed();
  Rows rows;
  std::vector<Warning> warnings;
  calc.calculate(bed, rows, [&](const Warning &w) { warnings.push_back(w); });
  CHECK(rows.size() == 10);
  // (RC_LFE is no LFE label: libear's warning that the frequency and the label disagree, once)
  CHECK(warnings.size() == 1 && warnings[0].code == Warning::Code::FREQ_SPEAKERLABEL_LFE_MISMATCH);
  const char *want[10] = {"M+030", "M-030", "M+000", "LFE1", nullptr, nullptr, "M+110", "M-110", nullptr, nullptr};
  for (size_t i = 0; i < 10; i++) {
    if (want[i]) {
      CHECK(rows[i] == one_hot(layout, want[i]));
      continue;
    }
    // the rest reach the panner at the converted position: the row of the polar calculator there, bit for bit
    const PolarPosition p = conversion::pointCartToPolar(CartesianPosition(kBed[i].x, kBed[i].y, kBed[i].z));
    DirectSpeakersTypeMetadata tm;
    tm.position = PolarSpeakerPosition(p.azimuth, p.elevation, 1.0);
    Gains polar(layout.channels().size());
    libear_calc.calculate(tm, polar);
    CHECK(rows[i] == polar);
    double power = 0.0;
    for (float v : rows[i]) power += (double)v * v;
    CHECK(std::fabs(power - 1.0) < 1e-5 && rows[i][layout.indexForName("LFE1")] == 0.0f);
  }
  // one at a time, into vectors of the caller's
  for (size_t i = 0; i < 10; i++) {
    Gains one(layout.channels().size(), 7.0f);
    calc.calculate(bed[i], one, [](const Warning &) {});
    CHECK(one == rows[i]);
  }
  // the loudspeakers as the bounds test sees them: the corners of the room
  const auto positions = calc.cartesianPositions();
  const CartesianPosition &l = positions.first[layout.indexForName("M+030")], &rs = positions.second[layout.indexForName("M-110")];
  CHECK(std::fabs(l.X + 1.0) < 1e-12 && std::fabs(l.Y - 1.0) < 1e-12 && std::fabs(l.Z) < 1e-12);
  CHECK(std::fabs(rs.X - 1.0) < 1e-12 && std::fabs(rs.Y + 1.0) < 1e-12 && std::fabs(rs.Z) < 1e-12);
  // a layout without its LFE channels, and bounds that pick a loudspeaker
  const Layout no_lfe = getLayout("4+7+0").withoutLfe();
  hip::DirectSpeakersGainCalculator narrow(no_lfe);
  CartesianSpeakerPosition pos(-0.8, 0.9, 0.0);
  pos.XMin = -1.0;
  pos.YMax = 1.0;
  DirectSpeakersTypeMetadata tm;
  tm.position = pos;
  Gains g(no_lfe.channels().size());
  narrow.calculate(tm, g);
  CHECK(g == one_hot(no_lfe, "M+030"));
}

static void test_locked_polar_channel() {
  const Layout layout = getLayout("4+7+0");
  const Screen reproduction = PolarScreen{1.78, PolarPosition(8.0, 5.0, 1.0), 58.0};
  hip::DirectSpeakersGainCalculator calc(layout, reproduction), no_screen(layout);
  GainCalculatorDirectSpeakers libear_calc(layout);
  const hip::ScreenHandler handler(reproduction);
  PolarSpeakerPosition pos(12.0, 3.0, 1.0);
  pos.screenEdgeLock.horizontal = std::string("left");
  pos.screenEdgeLock.vertical = std::string("top");
  DirectSpeakersTypeMetadata tm;
  tm.position = pos;
  Gains got(layout.channels().size()), want(layout.channels().size()), unlocked(layout.channels().size());
  calc.calculate(tm, got);
  // the screen stage of group R by hand, then libear's calculator at that position
  ObjectsTypeMetadata otm;
  otm.position = PolarPosition(12.0, 3.0, 1.0);
  const ObjectsTypeMetadata moved = handler.apply(otm, pos.screenEdgeLock);
  DirectSpeakersTypeMetadata plain;
  plain.position = PolarSpeakerPosition(moved.position.polar.azimuth, moved.position.polar.elevation, 1.0);
  libear_calc.calculate(plain, want);
  CHECK(got == want);
  CHECK(moved.position.polar.azimuth > 30.0 && moved.position.polar.elevation > 15.0);
  // without a screen the lock changes nothing
  no_screen.calculate(tm, got);
  plain.position = PolarSpeakerPosition(12.0, 3.0, 1.0);
  libear_calc.calculate(plain, unlocked);
  CHECK(got == unlocked && got != want);
  // a locked Cartesian channel: group V's stage by hand, then the calculator without a lock
  CartesianSpeakerPosition cpos(0.1, 1.0, 0.0);
  cpos.screenEdgeLock.horizontal = std::string("right");
  tm.position = cpos;
  calc.calculate(tm, got);
  ObjectsTypeMetadata cotm;
  cotm.position = CartesianPosition(0.1, 1.0, 0.0);
  cotm.cartesian = true;
  const ObjectsTypeMetadata cmoved = handler.apply_cartesian(cotm, cpos.screenEdgeLock);
  plain.position = CartesianSpeakerPosition(cmoved.position.cartesian.X, cmoved.position.cartesian.Y, cmoved.position.cartesian.Z);
  calc.calculate(plain, want);
  CHECK(got == want && cmoved.position.cartesian.X > 0.5);
}

static void test_exceptions() {
  const Layout layout = getLayout("4+7+0");
  hip::DirectSpeakersGainCalculator calc(layout);
  Gains gains(layout.channels().size());
  {
    DirectSpeakersTypeMetadata tm;
    PolarSpeakerPosition pos;
    pos.screenEdgeLock.horizontal = std::string("top");
    tm.position = pos;
    CHECK_THROWS_AS(calc.calculate(tm, gains), ear::invalid_argument);
  }
  {
    DirectSpeakersTypeMetadata tm;
    tm.position = CartesianSpeakerPosition(std::numeric_limits<double>::quiet_NaN(), 1.0, 0.0);
    CHECK_THROWS_AS(calc.calculate(tm, gains), ear::invalid_argument);
    CartesianSpeakerPosition pos(0.0, 1.0, 0.0);
    pos.ZMax = std::numeric_limits<double>::infinity();
    tm.position = pos;
    CHECK_THROWS_AS(calc.calculate(tm, gains), ear::invalid_argument);
  }
  {
    DirectSpeakersTypeMetadata tm;
    tm.position = CartesianSpeakerPosition();
    tm.audioPackFormatID = "AP_00010002";
    CHECK_THROWS_AS(calc.calculate(tm, gains), adm_error);
    tm.speakerLabels = {"urn:itu:bs:2051:0:speaker:M+030"};
    CHECK_THROWS_AS(calc.calculate(tm, gains), not_implemented);
  }
  {
    DirectSpeakersTypeMetadata tm;
    tm.position = CartesianSpeakerPosition();
    Gains wrong(layout.channels().size() + 1);
    CHECK_THROWS_AS(calc.calculate(tm, wrong), ear::invalid_argument);
  }
  // in a batch the message names the channel, and the warnings raised before it are delivered
  std::vector<DirectSpeakersTypeMetadata> batch(3);
  batch[0].channelFrequency.lowPass = 300.0;
  batch[0].speakerLabels = {"M+000"};
  batch[2].position = CartesianSpeakerPosition(0.0, std::numeric_limits<double>::infinity(), 0.0);
  Rows rows;
  std::string text;
  size_t n_warnings = 0;
  try {
    calc.calculate(batch, rows, [&](const Warning &) { n_warnings++; });
  } catch (const ear::invalid_argument &e) {
    text = e.what();
  }
  CHECK(text.find("metadata[2]") != std::string::npos && n_warnings == 1);
  // a screen across the rear seam
  CHECK_THROWS_AS(hip::DirectSpeakersGainCalculator(layout, Screen(PolarScreen{1.78, PolarPosition(170.0, 0.0, 1.0), 58.0})),
                  ear::invalid_argument);
  // libear's class still refuses what this one takes
  GainCalculatorDirectSpeakers libear_calc(layout);
  DirectSpeakersTypeMetadata tm;
  tm.position = CartesianSpeakerPosition();
  CHECK_THROWS_AS(libear_calc.calculate(tm, gains), not_implemented);
}

// ---- ObjectsProgramme::add_direct_speakers == add_stepped fed the calculator's rows by hand -------------------------------
static ObjectsTypeMetadata cart(double x, double y, double z, double diffuse = 0.0) {
  ObjectsTypeMetadata m;
  m.position = CartesianPosition(x, y, z);
  m.cartesian = true;
  m.diffuse = diffuse;
  return m;
}

static Rows render(ObjectsRenderer &r, size_t n_in, size_t n_out, size_t n_blocks) {
  const size_t B = 64;
  Rows in(n_in, std::vector<float>(n_blocks * B)), out(n_out, std::vector<float>(n_blocks * B));
  for (size_t m = 0; m < n_in; m++)
    for (size_t i = 0; i < n_blocks * B; i++) in[m][i] = (float)((int)((i * (2 * m + 3) + 5 * m) % 17) - 8) / 8.0f;
  std::vector<const float *> ip(n_in);
  std::vector<float *> op(n_out);
  for (size_t m = 0; m < n_in; m++) ip[m] = in[m].data();
  for (size_t c = 0; c < n_out; c++) op[c] = out[c].data();
  r.process(n_blocks, ip.data(), op.data());
  return out;
}

static bool same_bits(const Rows &a, const Rows &b) {
  if (a.size() != b.size()) return false;
  for (size_t c = 0; c < a.size(); c++)
    if (a[c].size() != b[c].size() || std::memcmp(a[c].data(), b[c].data(), a[c].size() * sizeof(float)) != 0) return false;
  return true;
}

static void test_programme() {
  const Layout layout = getLayout("4+7+0");
  const size_t N = layout.channels().size(), M = 12, B = 64, T = 8;
  const Screen reproduction = PolarScreen{1.78, PolarPosition(8.0, 5.0, 1.0), 58.0};
  const auto dec = designDecorrelators(layout);
  const int delay = decorrelatorCompensationDelay();
  // the bed: ten channels of two blocks each; in the second block the front pair is locked to the screen's edges
  const std::vector<BlockTiming> timing{BlockTiming(0, 200), BlockTiming(200, -1)};
  std::vector<std::vector<DirectSpeakersTypeMetadata>> channels;
  for (const DirectSpeakersTypeMetadata &tm : atmos_bed()) channels.push_back({tm, tm});
  channels[0][1].position.cartesian.screenEdgeLock.horizontal = std::string("left");
  channels[1][1].position.cartesian.screenEdgeLock.horizontal = std::string("right");
  const std::vector<std::pair<BlockTiming, ObjectsTypeMetadata>> object_a{{BlockTiming(0, 128), cart(-0.5, 1.0, 0.0)},
                                                                          {BlockTiming(128, 256, true, 32), cart(0.7, 0.2, 0.4, 0.3)}},
      object_b{{BlockTiming(40, 100), cart(0.0, -1.0, 0.0)}, {BlockTiming(140, -1, true, 64), cart(1.0, 1.0, 1.0, 1.0)}};

  for (int with_screen = 0; with_screen < 2; with_screen++) {
    hip::ObjectsProgramme programme = with_screen ? hip::ObjectsProgramme(layout, reproduction) : hip::ObjectsProgramme(layout);
    hip::ObjectsProgramme by_hand = with_screen ? hip::ObjectsProgramme(layout, reproduction) : hip::ObjectsProgramme(layout);
    // by hand: every block of every bed channel through one call of the calculator, the rows as stepped tracks
    std::vector<DirectSpeakersTypeMetadata> all;
    for (auto &ch : channels) all.insert(all.end(), ch.begin(), ch.end());
    Rows rows;
    const WarningCB quiet = [](const Warning &) {};
    if (with_screen)
      hip::DirectSpeakersGainCalculator(layout, reproduction).calculate(all, rows, quiet);
    else
      hip::DirectSpeakersGainCalculator(layout).calculate(all, rows, quiet);
    for (size_t c = 0; c < channels.size(); c++) {
      programme.add_direct_speakers(c, 16, timing, channels[c]);
      by_hand.add_stepped(c, 16, timing, Rows{rows[2 * c], rows[2 * c + 1]});
    }
    programme.add_object(10, 0, object_a), by_hand.add_object(10, 0, object_a);
    programme.add_object(11, -30, object_b), by_hand.add_object(11, -30, object_b);
    CHECK(programme.size() == 12);
    // the lock moves the front pair with a screen and leaves it alone without one
    CHECK((rows[0] != rows[1]) == (with_screen == 1) && (rows[2] != rows[3]) == (with_screen == 1));

    ObjectsRenderer bound(M, N, B, dec, delay, T), hand(M, N, B, dec, delay, T);
    // the bed's warnings reach the caller's callback: RC_LFE's two blocks, once each
    std::vector<Warning> warnings;
    const WarningCB collect = [&](const Warning &w) { warnings.push_back(w); };
    programme.bind(bound, hip::kTimelineBegin, hip::kTimelineEnd, collect), bound.commit();
    CHECK(warnings.size() == 2 && warnings[0].code == Warning::Code::FREQ_SPEAKERLABEL_LFE_MISMATCH);
    by_hand.bind(hand, hip::kTimelineBegin, hip::kTimelineEnd, collect), hand.commit();
    CHECK(warnings.size() == 2);  // (rows given by hand raise none)
    const Rows got = render(bound, M, N, T), want = render(hand, M, N, T);
    bool loud = false;
    for (auto &row : want)
      for (float v : row) loud = loud || v > 0.05f || v < -0.05f;
    CHECK(same_bits(got, want));
    CHECK(loud);
    // by window: bound half by half it renders what the rows bound whole by hand render in the same two calls
    ObjectsRenderer windowed(M, N, B, dec, delay, T), whole(M, N, B, dec, delay, T);
    by_hand.bind(whole), whole.commit();
    programme.bind(windowed, 0, 256, collect), windowed.commit();
    const Rows first = render(windowed, M, N, T / 2), first_want = render(whole, M, N, T / 2);
    programme.bind(windowed, 256, 512, collect), windowed.commit();
    const Rows second = render(windowed, M, N, T / 2), second_want = render(whole, M, N, T / 2);
    CHECK(same_bits(first, first_want) && same_bits(second, second_want));
  }

  // a refused block in the bed throws the calculator's exception and leaves every curve as it was
  {
    ObjectsRenderer r(M, N, B, dec, delay, T), untouched(M, N, B, dec, delay, T);
    hip::ObjectsProgramme bad(layout);
    bad.add_object(10, 0, object_a);
    bad.add_stepped(0, 16, timing, Rows{one_hot(layout, "M+030"), one_hot(layout, "M-030")});
    std::vector<DirectSpeakersTypeMetadata> blocks = channels[4];
    blocks[1].position.cartesian.X = std::numeric_limits<double>::quiet_NaN();
    bad.add_direct_speakers(4, 16, timing, blocks);
    CHECK_THROWS_AS(bad.bind(r), ear::invalid_argument);
    CHECK(same_bits(render(r, M, N, T), render(untouched, M, N, T)));
    // ... a window that does not reach the bad block binds
    bad.bind(r, 0, 100);
    CHECK_THROWS_AS(bad.add_direct_speakers(5, 0, timing, {channels[5][0]}), ear::invalid_argument);
  }
}

int main() {
  try {
    test_atmos_bed();
    test_locked_polar_channel();
    test_exceptions();
    test_programme();
  } catch (const std::exception &e) {
    g_failed++;
    std::printf("FAILED: exception %s\n", e.what());
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
