// ear::hip::ObjectsGainCalculator (libear_amd/host/ear/hip_objects.hpp): channelLock, polar objectDivergence and
// zoneExclusion of an Objects audioBlockFormat, written against the mirror headers alone.  The expected gains are the
// known answers of include/earhip.h group I (the _objects forms) as tests/objects_model.py gives them.  Compiles as C++14 with
// -Wall -Wextra -Werror; runs on a GPU.
#include <cmath>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include <ear/bs2051.hpp>
#include <ear/gain_calculators.hpp>
#include <ear/hip_objects.hpp>

#include "dropin_check.h"

using namespace ear;
using ear::hip::ObjectsGainCalculator;


// the gains are `want` on the channels it names and 0 everywhere else, within tol
static bool gains_are(const Layout &layout, const std::vector<float> &g, const std::map<std::string, double> &want, double tol) {
  bool ok = g.size() == layout.channels().size();
  for (size_t i = 0; ok && i < g.size(); i++) {
    const auto it = want.find(layout.channels()[i].name());
    ok = std::fabs(g[i] - (it == want.end() ? 0.0 : it->second)) <= tol;
  }
  return ok;
}

template <typename Calc>
static bool refuses(Calc &calc, const ObjectsTypeMetadata &m, size_t n) {
  std::vector<float> direct(n), diffuse(n);
  try {
    calc.calculate(m, direct, diffuse);
  } catch (const ear::not_implemented &) {
    return true;
  }
  return false;
}

int main() {
  const Layout layout = getLayout("4+5+0");
  const size_t n = layout.channels().size();
  ObjectsGainCalculator calc(layout);
  std::vector<float> direct(n), diffuse(n);
  const ObjectsTypeMetadata base;

  // divergence: (0, 0, 1), 0.5 over 30 degrees: a third of the power each at M+000, M+030, M-030
  ObjectsTypeMetadata m = base;
  m.position = PolarPosition(0.0, 0.0, 1.0);
  m.objectDivergence = PolarObjectDivergence(0.5, 30.0);
  calc.calculate(m, direct, diffuse);
  CHECK(gains_are(layout, direct, {{"M+030", 0.57735}, {"M-030", 0.57735}, {"M+000", 0.57735}}, 2e-6));
  CHECK(gains_are(layout, diffuse, {}, 0.0));

  // zone exclusion: a point source at (20, 20, 1), before and with every U* loudspeaker excluded
  m = base;
  m.position = PolarPosition(20.0, 20.0, 1.0);
  calc.calculate(m, direct, diffuse);
  CHECK(gains_are(layout, direct, {{"M+030", 0.066341}, {"M+000", 0.42965}, {"U+030", 0.900555}}, 2e-6));
  m.zoneExclusion.zones.push_back(PolarExclusionZone{-180.0f, 180.0f, 10.0f, 90.0f, 0.0f, 1.0f, "upper layer"});
  calc.calculate(m, direct, diffuse);
  CHECK(gains_are(layout, direct, {{"M+030", 0.902996}, {"M+000", 0.42965}}, 2e-6));
  // the same set as a Cartesian box above z = 0.2, and split over the diffuse path
  m.zoneExclusion.zones.clear();
  m.zoneExclusion.zones.push_back(CartesianExclusionZone{-1.0f, 1.0f, -1.0f, 1.0f, 0.2f, 1.0f, "above"});
  m.diffuse = 0.5;
  calc.calculate(m, direct, diffuse);
  const double h = std::sqrt(0.5);
  CHECK(gains_are(layout, direct, {{"M+030", 0.902996 * h}, {"M+000", 0.42965 * h}}, 2e-6));
  CHECK(gains_are(layout, diffuse, {{"M+030", 0.902996 * h}, {"M+000", 0.42965 * h}}, 2e-6));

  // channel lock: (10, 5) is nearest to M+000; with a maxDistance that it is out of reach of it stays
  m = base;
  m.position = PolarPosition(10.0, 5.0, 1.0);
  m.channelLock = ChannelLock(true);
  calc.calculate(m, direct, diffuse);
  CHECK(gains_are(layout, direct, {{"M+000", 1.0}}, 1e-6));
  std::vector<float> unlocked(n), unused(n);
  m.channelLock = ChannelLock(false);
  calc.calculate(m, unlocked, unused);
  m.channelLock = ChannelLock(true, 0.1);
  calc.calculate(m, direct, diffuse);
  {
    double worst = 0.0;
    for (size_t c = 0; c < n; c++) worst = std::fmax(worst, std::fabs(direct[c] - unlocked[c]));
    CHECK(worst <= 1e-6 && !gains_are(layout, direct, {{"M+000", 1.0}}, 1e-3));
  }
  m.channelLock = ChannelLock(true, 0.5);
  calc.calculate(m, direct, diffuse);
  CHECK(gains_are(layout, direct, {{"M+000", 1.0}}, 1e-6));

  // a batch, and a layout without its LFE channels
  {
    const Layout no_lfe = getLayout("4+5+0").withoutLfe();
    ObjectsGainCalculator calc2(no_lfe);
    std::vector<ObjectsTypeMetadata> batch(3);
    batch[0].position = PolarPosition(0.0, 0.0, 1.0);
    batch[0].objectDivergence = PolarObjectDivergence(0.5, 30.0);
    batch[1].position = PolarPosition(10.0, 5.0, 1.0);
    batch[1].channelLock = ChannelLock(true);
    batch[2].position = PolarPosition(-30.0, 0.0, 1.0);
    std::vector<std::vector<double>> d, f;
    calc2.calculate(batch, d, f);
    CHECK(d.size() == 3 && d[0].size() == no_lfe.channels().size());
    CHECK(gains_are(no_lfe, std::vector<float>(d[0].begin(), d[0].end()), {{"M+030", 0.57735}, {"M-030", 0.57735}, {"M+000", 0.57735}},
                    2e-6));
    CHECK(gains_are(no_lfe, std::vector<float>(d[1].begin(), d[1].end()), {{"M+000", 1.0}}, 1e-6));
    CHECK(gains_are(no_lfe, std::vector<float>(d[2].begin(), d[2].end()), {{"M-030", 1.0}}, 1e-6));
  }

  // what stays refused
  m = base;
  m.cartesian = true;
  CHECK(refuses(calc, m, n));
  m = base;
  m.position = CartesianPosition(0.0, 1.0, 0.0);
  CHECK(refuses(calc, m, n));
  m = base;
  m.objectDivergence = CartesianObjectDivergence(0.5);
  CHECK(refuses(calc, m, n));
  m.objectDivergence = CartesianObjectDivergence(0.0);
  CHECK(!refuses(calc, m, n));
  m = base;
  m.screenRef = true;
  CHECK(refuses(calc, m, n));
  CHECK(!refuses(calc, base, n));
  // values outside their ranges are invalid arguments
  {
    m = base;
    m.objectDivergence = PolarObjectDivergence(1.5);
    CHECK_THROWS_AS(calc.calculate(m, direct, diffuse), ear::invalid_argument);
  }

  // ear::GainCalculatorObjects refuses all three, as libear does
  GainCalculatorObjects plain(layout);
  m = base;
  m.objectDivergence = PolarObjectDivergence(0.5);
  CHECK(refuses(plain, m, n));
  m = base;
  m.channelLock.flag = true;
  CHECK(refuses(plain, m, n));
  m = base;
  m.zoneExclusion.zones.push_back(PolarExclusionZone{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, ""});
  CHECK(refuses(plain, m, n));
  CHECK(!refuses(plain, base, n));
  // ... and without them the two calculators give the same bits
  m = base;
  m.position = PolarPosition(35.0, 12.0, 0.7);
  m.width = 30.0;
  m.depth = 0.2;
  std::vector<float> d2(n), f2(n);
  plain.calculate(m, direct, diffuse);
  calc.calculate(m, d2, f2);
  CHECK(direct == d2 && diffuse == f2);

  return summary();
}
