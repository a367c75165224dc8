// Drop-in test of ear::GainCalculatorDirectSpeakers: a libear application's lines, compiled against the C++14
// mirror headers only (libear_amd/host/ear/...), restating the reference's own Catch2 cases
// (tests/gain_calculator_direct_speakers_tests.cpp) without Eigen/Catch2.  Expected gains are one-hot vectors
// or closed forms (a source half way between two loudspeakers: sqrt(0.5) on each), so this program needs
// nothing but libearhip.so and a GPU.
// Build (one line): g++ -std=c++14 -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_direct_speakers.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_direct_speakers
#include <cmath>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include <ear/ear.hpp>

#include "dropin_check.h"

using namespace ear;


typedef std::vector<double> Gains;

static DirectSpeakersTypeMetadata tmWithLabels(std::vector<std::string> labels) {
  DirectSpeakersTypeMetadata tm;
  tm.speakerLabels = labels;
  return tm;
}
static Gains directPv(const Layout &layout, const std::string &channel) {
  Gains g(layout.channels().size(), 0.0);
  g[layout.indexForName(channel)] = 1.0;
  return g;
}
static bool approx(const Gains &a, const Gains &b, double tol = 1e-6) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (std::fabs(a[i] - b[i]) > tol) return false;
  return true;
}

// the line of the pull request's issue: a 4+5+0 calculator with an extra substitution, a WarningCB, and a refusal
static void test_issue_program() {
  GainCalculatorDirectSpeakers p(getLayout("4+5+0"), {{"foo", "M+030"}});
  const Layout layout = getLayout("4+5+0");
  std::vector<float> gains(layout.channels().size());
  std::vector<Warning> warnings;
  WarningCB cb = [&](const Warning &w) { warnings.push_back(w); };
  p.calculate(tmWithLabels({"foo"}), gains, cb);
  CHECK(gains[layout.indexForName("M+030")] == 1.0f);
  CHECK(warnings.empty());
  DirectSpeakersTypeMetadata tm = tmWithLabels({"urn:itu:bs:2051:0:speaker:M+030"});
  tm.audioPackFormatID = "AP_00010003";
  bool refused = false;
  try {
    p.calculate(tm, gains, cb);
  } catch (const not_implemented &e) {
    refused = std::string(e.what()).find("AP_00010003") != std::string::npos;
  }
  CHECK(refused);
}

static void test_speaker_label() {
  Layout layout = getLayout("4+5+0");
  GainCalculatorDirectSpeakers p(layout);
  Gains actual(layout.channels().size());
  for (const std::string prefix : {"", "urn:itu:bs:2051:0:speaker:", "urn:itu:bs:2051:1:speaker:"}) {
    p.calculate(tmWithLabels({prefix + "M+000"}), actual);
    CHECK(approx(actual, directPv(layout, "M+000")));
    p.calculate(tmWithLabels({prefix + "M+030"}), actual);
    CHECK(approx(actual, directPv(layout, "M+030")));
    p.calculate(tmWithLabels({prefix + "M+030", prefix + "B+000"}), actual);
    CHECK(approx(actual, directPv(layout, "M+030")));
    p.calculate(tmWithLabels({prefix + "B+000", prefix + "M+030"}), actual);
    CHECK(approx(actual, directPv(layout, "M+030")));
    p.calculate(tmWithLabels({prefix + "M+000", prefix + "M+030"}), actual);
    CHECK(approx(actual, directPv(layout, "M+000")));
    p.calculate(tmWithLabels({prefix + "M+030", prefix + "M+000"}), actual);
    CHECK(approx(actual, directPv(layout, "M+030")));
  }
}

static void test_lfe() {
  Layout layout = getLayout("4+5+0");
  GainCalculatorDirectSpeakers p(layout);
  Gains actual(layout.channels().size());
  p.calculate(tmWithLabels({"LFE1"}), actual);
  CHECK(approx(actual, directPv(layout, "LFE1")));
  p.calculate(tmWithLabels({"LFE2"}), actual);
  CHECK(approx(actual, directPv(layout, "LFE1")));
  DirectSpeakersTypeMetadata tm;
  tm.channelFrequency.lowPass = 100.0;
  p.calculate(tm, actual);
  CHECK(approx(actual, directPv(layout, "LFE1")));

  Layout stereo = getLayout("0+2+0");
  GainCalculatorDirectSpeakers q(stereo);
  Gains silent(stereo.channels().size(), 1.0);
  q.calculate(tmWithLabels({"LFE1"}), silent);
  CHECK(approx(silent, Gains(2, 0.0)));
  q.calculate(tmWithLabels({"LFE2"}), silent);
  CHECK(approx(silent, Gains(2, 0.0)));
}

static void test_dist_bounds_polar() {
  Layout layout = getLayout("9+10+3");
  GainCalculatorDirectSpeakers p(layout);
  DirectSpeakersTypeMetadata tm;
  Gains actual(layout.channels().size(), 0.0);
  Gains expected(layout.channels().size(), 0.0);
  expected[layout.indexForName("M+000")] = std::sqrt(0.5);
  expected[layout.indexForName("M+030")] = std::sqrt(0.5);
  PolarSpeakerPosition pos(15.0, 0.0, 1.0);
  tm.position = pos;
  p.calculate(tm, actual);
  CHECK(approx(actual, expected));
  pos = PolarSpeakerPosition(15.0, 0.0, 1.0);
  pos.azimuthMin = 0.0;
  tm.position = pos;
  p.calculate(tm, actual);
  CHECK(approx(actual, directPv(layout, "M+000")));
  pos = PolarSpeakerPosition(15.0, 0.0, 1.0);
  pos.azimuthMax = 30.0;
  tm.position = pos;
  p.calculate(tm, actual);
  CHECK(approx(actual, directPv(layout, "M+030")));
  pos.azimuthMin = 0.0;
  tm.position = pos;
  p.calculate(tm, actual);
  CHECK(approx(actual, expected));
  pos = PolarSpeakerPosition(14.0, 0.0, 1.0);
  pos.azimuthMin = 0.0;
  pos.azimuthMax = 30.0;
  tm.position = pos;
  p.calculate(tm, actual);
  CHECK(approx(actual, directPv(layout, "M+000")));
  pos = PolarSpeakerPosition(15.0, 90.0, 1.0);
  pos.azimuthMin = 10.0;
  pos.azimuthMax = 20.0;
  tm.position = pos;
  p.calculate(tm, actual);
  CHECK(approx(actual, directPv(layout, "T+000")));
}

static void test_refusals_errors_warnings() {
  Layout layout = getLayout("4+7+0").withoutLfe();
  GainCalculatorDirectSpeakers p(layout);
  Gains gains(layout.channels().size(), 0.0);
  {
    DirectSpeakersTypeMetadata tm;
    PolarSpeakerPosition pos;
    pos.screenEdgeLock.horizontal = "left";
    tm.position = pos;
    CHECK_THROWS_AS(p.calculate(tm, gains), not_implemented);
  }
  {
    DirectSpeakersTypeMetadata tm;
    PolarSpeakerPosition pos;
    pos.screenEdgeLock.vertical = "top";
    tm.position = pos;
    CHECK_THROWS_AS(p.calculate(tm, gains), not_implemented);
  }
  {
    DirectSpeakersTypeMetadata tm;
    tm.position = CartesianSpeakerPosition();
    CHECK_THROWS_AS(p.calculate(tm, gains), not_implemented);
  }
  {
    DirectSpeakersTypeMetadata tm;
    tm.audioPackFormatID = "AP_00010002";
    CHECK_THROWS_AS(p.calculate(tm, gains), adm_error);
    Gains wrong(3);
    CHECK_THROWS_AS(p.calculate(tm, wrong), adm_error);  // (the ADM check comes first, as in libear)
  }
  Gains wrong(layout.channels().size() + 1);
  CHECK_THROWS_AS(p.calculate(tmWithLabels({"M+000"}), wrong), invalid_argument);
  {
    DirectSpeakersTypeMetadata tm;
    tm.channelFrequency.lowPass = 300.0;
    std::vector<Warning> warnings;
    p.calculate(tm, gains, [&](const Warning &w) { warnings.push_back(w); });
    CHECK(warnings.size() == 1 && warnings[0].code == Warning::Code::FREQ_NOT_LFE);
  }
  {
    DirectSpeakersTypeMetadata tm;
    tm.channelFrequency.lowPass = 100.0;
    tm.speakerLabels = {"M+000"};
    std::vector<Warning> warnings;
    p.calculate(tm, gains, [&](const Warning &w) { warnings.push_back(w); });
    CHECK(warnings.size() == 1 && warnings[0].code == Warning::Code::FREQ_SPEAKERLABEL_LFE_MISMATCH);
    // the layout has no LFE channel: silence
    CHECK(approx(gains, Gains(layout.channels().size(), 0.0)));
  }
  {
    // a pack that is not of the common definitions follows the labels, as in libear
    DirectSpeakersTypeMetadata tm = tmWithLabels({"urn:itu:bs:2051:0:speaker:M+090"});
    tm.audioPackFormatID = "AP_00020001";
    p.calculate(tm, gains);
    CHECK(approx(gains, directPv(layout, "M+090")));
  }
}

int main() {
  try {
    test_issue_program();
    test_speaker_label();
    test_lfe();
    test_dist_bounds_polar();
    test_refusals_errors_warnings();
  } catch (const std::exception &e) {
    g_failed++;
    std::printf("FAILED: exception %s\n", e.what());
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
