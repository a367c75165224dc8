// ear::hip::ScreenHandler (libear_amd/host/ear/hip_screen.hpp): screenRef scaling and screenEdgeLock of Objects metadata,
// written against the mirror headers alone.  The expected values are the known answers of include/earhip.h group R.  Compiles
// as C++14 with -Wall -Wextra -Werror.  `test_dropin_screen host` runs what needs no device (edges, the single-element path,
// the refusals); without an argument the batch path and the gain calculators run too, on a GPU.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <ear/bs2051.hpp>
#include <ear/gain_calculators.hpp>
#include <ear/hip_objects.hpp>
#include <ear/hip_screen.hpp>

#include "dropin_check.h"

using namespace ear;
using ear::hip::ScreenHandler;


static const Screen kScreen30 = PolarScreen{1.78, PolarPosition(0.0, 0.0, 1.0), 30.0};
static const Screen kPolar15 = PolarScreen{1.5, PolarPosition(-20.0, 10.0, 2.0), 40.0};
static const Screen kCart = CartesianScreen{1.78, CartesianPosition(0.0, 1.0, 0.0), 1.0};

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-10; }

static bool edges_are(const Screen &s, double left, double right, double bottom, double top) {
  const std::array<double, 4> e = ScreenHandler::edges(s);
  return near(e[0], left) && near(e[1], right) && near(e[2], bottom) && near(e[3], top);
}

static ObjectsTypeMetadata at(double az, double el, bool screen_ref = true, const Screen &reference = getDefaultScreen()) {
  ObjectsTypeMetadata m;
  m.position = PolarPosition(az, el, 1.0);
  m.screenRef = screen_ref;
  m.referenceScreen = reference;
  return m;
}

static ScreenEdgeLock lock(const char *horizontal, const char *vertical) {
  ScreenEdgeLock l;
  if (horizontal) l.horizontal = std::string(horizontal);
  if (vertical) l.vertical = std::string(vertical);
  return l;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

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

int main(int argc, char **argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "host") == 0;

  // edges
  CHECK(edges_are(getDefaultScreen(), 29.0, -29.0, -17.29708889245067, 17.29708889245067));
  CHECK(edges_are(kPolar15, 0.283559454529715, -40.283559454529716, -3.639039283545732, 23.63903928354573));
  CHECK(edges_are(kCart, 26.56505117707799, -26.56505117707799, -15.689992929083877, 15.689992929083877));
  CHECK(edges_are(kScreen30, 15.0, -15.0, -8.560644163419065, 8.560644163419065));

  // scalings; apply clears screenRef and leaves everything else alone
  {
    const ScreenHandler to30(kScreen30), to15(kPolar15), to_default(getDefaultScreen());
    ObjectsTypeMetadata m = at(90.0, 45.0);
    m.gain = 0.5, m.width = 20.0, m.position.polar.distance = 0.75;
    ObjectsTypeMetadata r = to30.apply(m);
    CHECK(near(r.position.polar.azimuth, 81.65562913907284) && near(r.position.polar.elevation, 39.59251346586589));
    CHECK(!r.screenRef && m.screenRef && r.gain == 0.5 && r.width == 20.0 && r.position.polar.distance == 0.75);
    r = to30.apply(at(14.5, -8.0));
    CHECK(near(r.position.polar.azimuth, 7.5) && near(r.position.polar.elevation, -3.9593456293817697));
    r = to30.apply(at(-100.0, -50.0));
    CHECK(near(r.position.polar.azimuth, -92.58278145695364) && near(r.position.polar.elevation, -45.1933453029919));
    r = to15.apply(at(0.0, 0.0));
    CHECK(near(r.position.polar.azimuth, -20.0) && near(r.position.polar.elevation, 10.0));
    r = to15.apply(at(90.0, 45.0));
    CHECK(near(r.position.polar.azimuth, 72.88424073448789) && near(r.position.polar.elevation, 48.92539670353921));
    r = to_default.apply(at(90.0, 45.0, true, kCart));
    CHECK(near(r.position.polar.azimuth, 91.42826256823597) && near(r.position.polar.elevation, 45.97321102772186));
    // exact: the seam and the poles, an azimuth beyond a turn, a block without screenRef
    r = to15.apply(at(180.0, -90.0));
    CHECK(r.position.polar.azimuth == 180.0 && r.position.polar.elevation == -90.0);
    CHECK(same_bits(to30.apply(at(389.0, 0.0)).position.polar.azimuth, to30.apply(at(29.0, 0.0)).position.polar.azimuth));
    r = to30.apply(at(400.0, 12.0, false));
    CHECK(r.position.polar.azimuth == 400.0 && r.position.polar.elevation == 12.0 && !r.screenRef);
    // locks: the reproduction screen's edges, scaled or not; the other component scaled or untouched
    const std::array<double, 4> e = ScreenHandler::edges(kScreen30);
    r = to30.apply(at(400.0, 12.0, false), lock("left", nullptr));
    CHECK(r.position.polar.azimuth == e[0] && r.position.polar.elevation == 12.0);
    r = to30.apply(at(400.0, 12.0, false), lock(nullptr, "top"));
    CHECK(r.position.polar.azimuth == 400.0 && r.position.polar.elevation == e[3]);
    r = to30.apply(at(90.0, 45.0), lock("right", "bottom"));
    CHECK(r.position.polar.azimuth == e[1] && r.position.polar.elevation == e[2]);
    r = to30.apply(at(90.0, 45.0), lock("right", nullptr));
    CHECK(r.position.polar.azimuth == e[1] && near(r.position.polar.elevation, 39.59251346586589));
  }
  // the default-constructed handler has no reproduction screen: everything passes through, screenRef cleared
  {
    const ScreenHandler none;
    ObjectsTypeMetadata r = none.apply(at(400.0, 45.0), lock("left", "top"));
    CHECK(r.position.polar.azimuth == 400.0 && r.position.polar.elevation == 45.0 && !r.screenRef);
  }
  // what is refused
  {
    const ScreenHandler to30(kScreen30);
    bool threw = false;
    ObjectsTypeMetadata m = at(10.0, 5.0);
    m.position = CartesianPosition(0.1, 0.9, 0.0);
    try {
      to30.apply(m);
    } catch (const ear::not_implemented &e) {
      threw = std::string(e.what()) == "not implemented: cartesian";
    }
    CHECK(threw);
    threw = false;
    m = at(10.0, 5.0), m.cartesian = true;
    CHECK_THROWS_AS(to30.apply(m), ear::not_implemented);
    for (int k = 0; k < 3; k++) {
      const ScreenEdgeLock bad_lock = k == 0 ? lock("top", nullptr) : (k == 1 ? lock(nullptr, "left") : lock("Left", nullptr));
      CHECK_THROWS_AS(to30.apply(at(10.0, 5.0), bad_lock), ear::adm_error);
    }
    CHECK_THROWS_AS(to30.apply(at(10.0, 91.0)), ear::invalid_argument);
    // screens: across the rear seam, a zero aspect ratio, a width of 180 — as reproduction, as reference, in edges()
    const Screen bad[3] = {PolarScreen{1.78, PolarPosition(170.0, 0.0, 1.0), 58.0}, PolarScreen{0.0, PolarPosition(0.0, 0.0, 1.0), 58.0},
                           PolarScreen{1.78, PolarPosition(0.0, 0.0, 1.0), 180.0}};
    for (const Screen &s : bad) {
      int caught = 0;
      try {
        ScreenHandler h(s);
      } catch (const ear::invalid_argument &) {
        caught++;
      }
      try {
        to30.apply(at(10.0, 5.0, true, s));
      } catch (const ear::invalid_argument &) {
        caught++;
      }
      try {
        ScreenHandler::edges(s);
      } catch (const ear::invalid_argument &) {
        caught++;
      }
      CHECK(caught == 3);
    }
  }
  if (host_only) {
    return summary("host");
  }

  // the batch form (one device launch per reference screen) equals the single form bit for bit
  {
    const ScreenHandler to15(kPolar15);
    const char *hs[3] = {nullptr, "left", "right"}, *vs[3] = {nullptr, "bottom", "top"};
    std::vector<ObjectsTypeMetadata> blocks;
    std::vector<ScreenEdgeLock> locks;
    for (int i = 0; i < 203; i++) {
      const Screen &ref = i % 5 == 0 ? kCart : (i % 7 == 0 ? kScreen30 : getDefaultScreen());
      ObjectsTypeMetadata m = at(-400.0 + 4.25 * i, -90.0 + 0.875 * i, i % 3 != 0, ref);
      m.gain = 0.01 * i;
      blocks.push_back(m);
      locks.push_back(lock(hs[i % 3], vs[(i / 3) % 3]));
    }
    std::vector<ObjectsTypeMetadata> batch = blocks;
    to15.apply(batch, locks);
    size_t differ = 0;
    for (size_t i = 0; i < blocks.size(); i++) {
      const ObjectsTypeMetadata one = to15.apply(blocks[i], locks[i]);
      if (!same_bits(one.position.polar.azimuth, batch[i].position.polar.azimuth) ||
          !same_bits(one.position.polar.elevation, batch[i].position.polar.elevation) || batch[i].screenRef ||
          batch[i].gain != blocks[i].gain || batch[i].position.polar.distance != 1.0)
        differ++;
    }
    std::printf("batch vs single: %zu of %zu blocks differ\n", differ, blocks.size());
    CHECK(differ == 0);
    // without locks; an empty batch; the default-constructed handler
    batch = blocks;
    to15.apply(batch);
    differ = 0;
    for (size_t i = 0; i < blocks.size(); i++)
      if (!same_bits(to15.apply(blocks[i]).position.polar.azimuth, batch[i].position.polar.azimuth)) differ++;
    CHECK(differ == 0);
    std::vector<ObjectsTypeMetadata> none;
    to15.apply(none);
    CHECK(none.empty());
    batch = blocks;
    ScreenHandler().apply(batch, locks);
    differ = 0;
    for (size_t i = 0; i < blocks.size(); i++)
      if (!same_bits(blocks[i].position.polar.azimuth, batch[i].position.polar.azimuth) || batch[i].screenRef) differ++;
    CHECK(differ == 0);
    // the batch refuses what the single form refuses, names a bad element and writes nothing
    batch = blocks;
    batch[77] = at(0.0, 90.0000001);
    bool threw = false;
    try {
      to15.apply(batch, locks);
    } catch (const ear::invalid_argument &e) {
      threw = std::string(e.what()).find("metadata block 77") != std::string::npos;
    }
    CHECK(threw && batch[0].screenRef == blocks[0].screenRef && batch[1].position.polar.azimuth == blocks[1].position.polar.azimuth);
    batch = blocks;
    batch[5].position = CartesianPosition(0.0, 1.0, 0.0);
    CHECK_THROWS_AS(to15.apply(batch, locks), ear::not_implemented);
    CHECK_THROWS_AS(to15.apply(batch, std::vector<ScreenEdgeLock>(3)), ear::invalid_argument);
  }
  // in front of the gain calculators: they refuse the raw block and accept the handler's result
  {
    const Layout layout = getLayout("0+5+0");
    const size_t n = layout.channels().size();
    ear::hip::ObjectsGainCalculator calc(layout);
    GainCalculatorObjects libear_calc(layout);
    const ObjectsTypeMetadata raw = at(29.0, 0.0);
    CHECK(refuses(calc, raw, n));
    CHECK(refuses(libear_calc, raw, n));
    const ObjectsTypeMetadata scaled = ScreenHandler(kScreen30).apply(raw);
    CHECK(!refuses(calc, scaled, n));
    CHECK(!refuses(libear_calc, scaled, n));
    std::vector<float> direct(n), diffuse(n);
    calc.calculate(scaled, direct, diffuse);
    bool ok = true;
    for (size_t i = 0; i < n; i++) {
      const std::string name = layout.channels()[i].name();
      const double want = name == "M+000" || name == "M+030" ? std::sqrt(0.5) : 0.0;
      ok = ok && std::fabs(direct[i] - want) <= 2e-6 && diffuse[i] == 0.0f;
    }
    CHECK(ok);
  }
  return summary();
}
