// A hand-built ear::Layout — libear's Layout(name, channels) is a public constructor — through the gain calculators of the
// C++14 mirror, written against the mirror headers alone: the layout 2+7+0 (no row of BS.2051), its withoutLfe() form and a
// layout with an empty name go through GainCalculatorObjects, ear::hip::ObjectsGainCalculator (batch), GainCalculatorHOA and
// GainCalculatorDirectSpeakers; BS.2051 names keep their errors.  Compiles as C++14 with -Wall -Wextra -Werror.
// `test_dropin_custom_layout host` runs what needs no device (the definitions and the refusals); without an argument the
// calculators run too, on a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <ear/bs2051.hpp>
#include <ear/gain_calculators.hpp>
#include <ear/hip_objects.hpp>

#include "dropin_check.h"

using namespace ear;


static Layout layout_2_7_0(const std::string &name) {
  std::vector<Channel> ch;
  ch.emplace_back("M+030", PolarPosition(30.0, 0.0));
  ch.emplace_back("M-030", PolarPosition(-30.0, 0.0));
  ch.emplace_back("M+000", PolarPosition(0.0, 0.0));
  ch.emplace_back("LFE1", PolarPosition(45.0, -30.0), true);
  ch.emplace_back("M+090", PolarPosition(90.0, 0.0));
  ch.emplace_back("M-090", PolarPosition(-90.0, 0.0));
  ch.emplace_back("M+135", PolarPosition(135.0, 0.0));
  ch.emplace_back("M-135", PolarPosition(-135.0, 0.0));
  ch.emplace_back("U+090", PolarPosition(90.0, 30.0));
  ch.emplace_back("U-090", PolarPosition(-90.0, 30.0));
  return Layout(name, ch);
}

static ObjectsTypeMetadata at(double az, double el) {
  ObjectsTypeMetadata m;
  m.position = PolarPosition(az, el, 1.0);
  return m;
}

static bool near(double a, double b, double tol = 1e-6) { return std::fabs(a - b) <= tol; }

// one loudspeaker plays a source at its own position, LFE channels stay silent, the power of any direction is 1
template <typename Calc>
static void check_objects(Calc &calc, const Layout &layout) {
  const size_t n = layout.channels().size();
  for (size_t c = 0; c < n; c++) {
    const Channel &ch = layout.channels()[c];
    if (ch.isLfe()) continue;
    std::vector<double> direct(n, -1.0), diffuse(n, -1.0);
    calc.calculate(at(ch.polarPosition().azimuth, ch.polarPosition().elevation), direct, diffuse);
    for (size_t k = 0; k < n; k++) CHECK(near(direct[k], k == c ? 1.0 : 0.0) && diffuse[k] == 0.0);
  }
  std::vector<ObjectsTypeMetadata> batch;
  for (int i = 0; i < 64; i++) batch.push_back(at(-180.0 + 360.0 * i / 64.0, -80.0 + 2.5 * i));
  batch[5].diffuse = 0.5;
  std::vector<std::vector<float>> direct, diffuse;
  calc.calculate(batch, direct, diffuse);
  CHECK(direct.size() == batch.size() && direct[0].size() == n);
  for (size_t i = 0; i < batch.size() && direct.size() == batch.size(); i++) {
    double power = 0.0;
    for (size_t k = 0; k < n; k++) {
      power += (double)direct[i][k] * direct[i][k] + (double)diffuse[i][k] * diffuse[i][k];
      if (layout.channels()[k].isLfe()) CHECK(direct[i][k] == 0.0f && diffuse[i][k] == 0.0f);
    }
    CHECK(near(power, 1.0, 1e-5));
  }
}

static void check_layout_on_device(const Layout &layout) {
  const size_t n = layout.channels().size();
  {
    GainCalculatorObjects calc(layout);
    check_objects(calc, layout);
  }
  {
    ear::hip::ObjectsGainCalculator calc(layout);
    check_objects(calc, layout);
    // what only the batch calculator carries: a locked object plays from the nearest loudspeaker alone
    ObjectsTypeMetadata m = at(80.0, 5.0);
    m.channelLock = ChannelLock(true);
    std::vector<double> direct(n), diffuse(n);
    calc.calculate(m, direct, diffuse);
    const int want = layout.indexForName("M+090");
    for (size_t k = 0; k < n; k++) CHECK(near(direct[k], (int)k == want ? 1.0 : 0.0));
  }
  {
    GainCalculatorHOA calc(layout);
    HOATypeMetadata m;
    m.orders = {0, 1, 1, 1};
    m.degrees = {0, -1, 0, 1};
    std::vector<std::vector<double>> gains(4, std::vector<double>(n, -1.0));
    calc.calculate(m, gains);
    double w = 0.0;
    for (size_t k = 0; k < n; k++) {
      const Channel &ch = layout.channels()[k];
      w += gains[0][k];
      if (ch.isLfe()) {
        for (size_t c = 0; c < 4; c++) CHECK(gains[c][k] == 0.0);
        continue;
      }
      // every loudspeaker plays W; Y (ACN 1) is positive on the left and negative on the right, X (ACN 3) positive in front
      // and negative behind, and the upper loudspeakers take more of Z (ACN 2) than the middle ones beside them
      const double az = ch.polarPositionNominal().azimuth;
      CHECK(gains[0][k] > 0.0);
      if (az != 0.0) CHECK(az > 0.0 ? gains[1][k] > 0.0 : gains[1][k] < 0.0);
      if (std::fabs(az) != 90.0) CHECK(std::fabs(az) < 90.0 ? gains[3][k] > 0.0 : gains[3][k] < 0.0);
    }
    CHECK(gains[2][(size_t)layout.indexForName("U+090")] > gains[2][(size_t)layout.indexForName("M+090")]);
    CHECK(gains[2][(size_t)layout.indexForName("U-090")] > gains[2][(size_t)layout.indexForName("M-090")]);
    CHECK(w > 0.5);
  }
  {
    GainCalculatorDirectSpeakers calc(layout);
    DirectSpeakersTypeMetadata m;
    m.speakerLabels = {"U-090"};
    std::vector<double> gains(n, -1.0);
    calc.calculate(m, gains);
    for (size_t k = 0; k < n; k++) CHECK(gains[k] == ((int)k == layout.indexForName("U-090") ? 1.0 : 0.0));
    // no label, a position between two loudspeakers: the point source panner
    DirectSpeakersTypeMetadata p;
    p.position = PolarSpeakerPosition(15.0, 0.0, 1.0);
    calc.calculate(p, gains);
    CHECK(near(gains[(size_t)layout.indexForName("M+030")], std::sqrt(0.5)) && near(gains[(size_t)layout.indexForName("M+000")], std::sqrt(0.5)));
  }
}

int main(int argc, char **argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "host") == 0;

  // ---- the definitions behind the calculators (no device) ----
  const Layout custom = layout_2_7_0("2+7+0"), unnamed = layout_2_7_0(""), bare = custom.withoutLfe();
  std::vector<double> az, el;
  std::string name, name_unnamed, name_bare, name_moved, name_ranged;
  std::vector<int> keep = detail::match_layout(custom, name, az, el);
  CHECK(name.size() == 20 && name.compare(0, 4, "ear:") == 0 && keep.size() == 10 && az.size() == 10 && keep[9] == 9);
  az.clear(), el.clear();
  detail::match_layout(unnamed, name_unnamed, az, el);
  CHECK(name_unnamed == name);  // the layout's own name is no part of the definition
  az.clear(), el.clear();
  keep = detail::match_layout(bare, name_bare, az, el);
  CHECK(name_bare != name && keep.size() == 9 && az.size() == 9);  // a definition of its own
  Layout moved = custom;
  moved.channels()[0].polarPosition(PolarPosition(33.0, 2.0));  // where a loudspeaker really stands is no part of it either
  az.clear(), el.clear();
  detail::match_layout(moved, name_moved, az, el);
  CHECK(name_moved == name && az[0] == 33.0 && el[0] == 2.0);
  Layout ranged = custom;
  ranged.channels()[0].azimuthRange(std::make_pair(25.0, 35.0));
  az.clear(), el.clear();
  detail::match_layout(ranged, name_ranged, az, el);
  CHECK(name_ranged != name);
  int kind = 0, n = 0;
  CHECK(earhip_layout_kind(name.c_str(), &kind) == EARHIP_OK && kind == 2);
  CHECK(earhip_layout_num_channels(name.c_str(), &n) == EARHIP_OK && n == 10);
  CHECK(earhip_layout_num_channels(name_bare.c_str(), &n) == EARHIP_OK && n == 9);
  double azr[2] = {0, 0}, elr[2] = {0, 0};
  CHECK(earhip_layout_channel_ranges(name_moved.c_str(), 0, azr, elr) == EARHIP_OK && azr[0] == 30.0 && azr[1] == 30.0 && elr[0] == 0.0);
  CHECK(earhip_layout_channel_ranges(name_ranged.c_str(), 0, azr, elr) == EARHIP_OK && azr[0] == 25.0 && azr[1] == 35.0 && elr[1] == 0.0);

  // ---- BS.2051 names keep their path and their errors ----
  {
    Layout foreign = getLayout("0+5+0");
    foreign.channels().push_back(Channel("U+090", PolarPosition(90.0, 30.0)));
    bool refused = false;
    try {
      az.clear(), el.clear();
      detail::match_layout(foreign, name, az, el);
    } catch (const ear::invalid_argument &e) {
      refused = std::string(e.what()) == "channel U+090 is not part of layout 0+5+0";
    }
    CHECK(refused);
    az.clear(), el.clear();
    keep = detail::match_layout(getLayout("4+5+0").withoutLfe(), name, az, el);
    CHECK(name == "4+5+0" && az.size() == 10 && keep.size() == 9 && keep[3] == 4);
    refused = false;
    try {
      getLayout("1+2+3");
    } catch (const ear::unknown_layout &e) {
      refused = std::string(e.what()) == "unknown layout: 1+2+3";
    }
    CHECK(refused);
    // a layout the hull refuses fails when the calculator is made, as an invalid argument
    Layout twice = custom;
    twice.channels().push_back(Channel("M+030 again", PolarPosition(30.0, 0.0)));
    refused = false;
    try {
      az.clear(), el.clear();
      detail::match_layout(twice, name, az, el);
    } catch (const ear::invalid_argument &e) {
      refused = std::string(e.what()).find("collinear") != std::string::npos;
    }
    CHECK(refused);
  }
  if (host_only) {
    return summary("host");
  }

  // ---- the calculators (device) ----
  check_layout_on_device(custom);
  check_layout_on_device(bare);
  check_layout_on_device(unnamed);
  {
    GainCalculatorObjects calc(moved);  // the geometry follows the real positions
    check_objects(calc, moved);
  }
  return summary();
}
