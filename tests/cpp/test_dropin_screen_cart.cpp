// ear::hip::ScreenHandler::apply_cartesian (libear_amd/host/ear/hip_screen.hpp): screenRef scaling and screenEdgeLock of
// Cartesian Objects metadata in front of ear::hip::AllocentricObjectsGainCalculator, written against the mirror headers and the
// C ABI (include/earhip.h group V) alone.  Compiles as C++14 with -Wall -Wextra -Werror.  `test_dropin_screen_cart host` runs
// what needs no device (the single-block form and the refusals); without an argument the batch form and the calculator run
// too, on a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include <ear/bs2051.hpp>
#include <ear/hip_allo_objects.hpp>
#include <ear/hip_screen.hpp>

#include "dropin_check.h"

using namespace ear;
using ear::hip::ScreenHandler;

static const Screen kScreen30 = PolarScreen{1.78, PolarPosition(0.0, 0.0, 1.0), 30.0};
static const Screen kPolar15 = PolarScreen{1.5, PolarPosition(-20.0, 10.0, 2.0), 40.0};
static const Screen kCart = CartesianScreen{1.78, CartesianPosition(0.0, 1.0, 0.0), 1.0};

static ObjectsTypeMetadata at(double x, double y, double z, bool screen_ref = true, const Screen &reference = getDefaultScreen()) {
  ObjectsTypeMetadata m;
  m.position = CartesianPosition(x, y, z);
  m.cartesian = true;
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
static bool same_position(const ObjectsTypeMetadata &a, const ObjectsTypeMetadata &b) {
  const CartesianPosition &p = a.position.cartesian, &q = b.position.cartesian;
  return a.position.isCartesian && b.position.isCartesian && same_bits(p.X, q.X) && same_bits(p.Y, q.Y) && same_bits(p.Z, q.Z);
}

static earhip_screen c_polar(double aspect, double az, double el, double d, double width) {
  earhip_screen s = earhip_screen();
  s.aspect_ratio = aspect, s.azimuth = az, s.elevation = el, s.distance = d, s.width_azimuth = width;
  return s;
}

// the C entry point on one position: reference, reproduction (either may be NULL), flags
static bool matches_c(const ObjectsTypeMetadata &got, const ObjectsTypeMetadata &in, const earhip_screen *reference,
                      const earhip_screen *reproduction, unsigned char lh, unsigned char lv) {
  const CartesianPosition &p = in.position.cartesian, &g = got.position.cartesian;
  const unsigned char ref = in.screenRef ? 1 : 0;
  double x, y, z;
  if (earhip_screen_apply_cartesian(reference, reproduction, 1, &p.X, &p.Y, &p.Z, &ref, &lh, &lv, &x, &y, &z) != EARHIP_OK) return false;
  return same_bits(g.X, x) && same_bits(g.Y, y) && same_bits(g.Z, z);
}

static std::string refusal(const ScreenHandler &h, const ObjectsTypeMetadata &m) {
  try {
    h.apply_cartesian(m);
  } catch (const ear::not_implemented &e) {
    return e.what();
  }
  return "";
}

template <typename Calc>
static std::string calculator_refusal(const Calc &calc, const std::vector<ObjectsTypeMetadata> &blocks, bool device) {
  std::vector<std::vector<float>> direct, diffuse;
  try {
    if (device)
      calc.calculate_device(blocks, direct, diffuse);
    else
      calc.calculate(blocks, direct, diffuse);
  } catch (const ear::not_implemented &e) {
    return e.what();
  }
  return "";
}

int main(int argc, char **argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "host") == 0;
  const earhip_screen c30 = c_polar(1.78, 0.0, 0.0, 1.0, 30.0), c15 = c_polar(1.5, -20.0, 10.0, 2.0, 40.0);
  earhip_screen ccart = earhip_screen();
  ccart.cartesian = 1, ccart.aspect_ratio = 1.78, ccart.y = 1.0, ccart.width_x = 1.0;

  // the single form: the C entry point's bits; screenRef cleared; extent and every other field untouched
  {
    const ScreenHandler to30(kScreen30), to15(kPolar15);
    ObjectsTypeMetadata m = at(-0.4, 0.9, 0.3);
    m.gain = 0.5, m.diffuse = 0.25, m.width = 0.2, m.height = 0.1, m.depth = 0.3;
    m.channelLock.flag = true;
    m.objectDivergence = CartesianObjectDivergence{0.5, 0.125};
    ObjectsTypeMetadata r = to30.apply_cartesian(m);
    CHECK(matches_c(r, m, nullptr, &c30, 0, 0));
    CHECK(!same_position(r, m) && std::fabs(r.position.cartesian.X - m.position.cartesian.X) > 1e-3);
    CHECK(!r.screenRef && m.screenRef && r.cartesian && r.position.isCartesian);
    CHECK(r.gain == 0.5 && r.diffuse == 0.25 && r.width == 0.2 && r.height == 0.1 && r.depth == 0.3 && r.channelLock.flag);
    CHECK(r.objectDivergence.isCartesian && r.objectDivergence.divergence == 0.5 && r.objectDivergence.range == 0.125);
    // a reference screen of the block's own; locks, with and without screenRef
    r = to15.apply_cartesian(at(0.7, -0.2, -0.6, true, kCart));
    CHECK(matches_c(r, at(0.7, -0.2, -0.6), &ccart, &c15, 0, 0));
    r = to15.apply_cartesian(at(0.7, -0.2, -0.6, true, kCart), lock("left", "top"));
    CHECK(matches_c(r, at(0.7, -0.2, -0.6), &ccart, &c15, 1, 2));
    r = to30.apply_cartesian(at(0.7, -0.2, -0.6, false), lock("right", nullptr));
    CHECK(matches_c(r, at(0.7, -0.2, -0.6, false), nullptr, &c30, 2, 0) && !r.screenRef);
    r = to30.apply_cartesian(at(0.7, -0.2, -0.6, false), lock(nullptr, "bottom"));
    CHECK(matches_c(r, at(0.7, -0.2, -0.6, false), nullptr, &c30, 0, 1));
    // a block with neither screenRef nor a lock keeps its bits, on a loudspeaker plane too; the origin stays the origin
    m = at(1.0, -0.0, 0.123456789, false);
    CHECK(same_position(to30.apply_cartesian(m), m));
    r = to15.apply_cartesian(at(0.0, 0.0, 0.0), lock("left", "top"));
    CHECK(r.position.cartesian.X == 0.0 && r.position.cartesian.Y == 0.0 && r.position.cartesian.Z == 0.0);
    // equal screens: there and back
    r = ScreenHandler(getDefaultScreen()).apply_cartesian(at(-0.4, 0.9, 0.3));
    CHECK(std::fabs(r.position.cartesian.X + 0.4) <= 1e-9 && std::fabs(r.position.cartesian.Y - 0.9) <= 1e-9 &&
          std::fabs(r.position.cartesian.Z - 0.3) <= 1e-9);
  }
  // the default-constructed handler has no reproduction screen: positions pass through bit for bit, screenRef cleared
  {
    const ScreenHandler none;
    const ObjectsTypeMetadata m = at(0.3, -0.7, 0.9);
    const ObjectsTypeMetadata r = none.apply_cartesian(m, lock("left", "top"));
    CHECK(same_position(r, m) && !r.screenRef);
  }
  // what is refused
  {
    const ScreenHandler to30(kScreen30);
    ObjectsTypeMetadata polar;
    polar.position = PolarPosition(10.0, 5.0, 1.0);
    polar.screenRef = true;
    CHECK(refusal(to30, polar) == "not implemented: position: polar");
    polar.cartesian = true;
    CHECK(refusal(to30, polar) == "not implemented: position: polar");
    ObjectsTypeMetadata unflagged = at(0.1, 0.9, 0.0);
    unflagged.cartesian = false;
    CHECK(refusal(to30, unflagged) == "not implemented: cartesian == false");
    // ScreenHandler::apply keeps refusing Cartesian metadata
    bool threw = false;
    try {
      to30.apply(at(0.1, 0.9, 0.0));
    } catch (const ear::not_implemented &e) {
      threw = std::string(e.what()) == "not implemented: cartesian";
    }
    CHECK(threw);
    for (int k = 0; k < 3; k++) {
      const ScreenEdgeLock bad_lock = k == 0 ? lock("top", nullptr) : (k == 1 ? lock(nullptr, "left") : lock("Left", nullptr));
      CHECK_THROWS_AS(to30.apply_cartesian(at(0.1, 0.9, 0.0), bad_lock), ear::adm_error);
    }
    CHECK_THROWS_AS(to30.apply_cartesian(at(std::numeric_limits<double>::quiet_NaN(), 0.9, 0.0)), ear::invalid_argument);
    CHECK_THROWS_AS(to30.apply_cartesian(at(0.1, std::numeric_limits<double>::infinity(), 0.0, false), lock("left", nullptr)),
                    ear::invalid_argument);
    // ... and is nobody's business in a block with no flag
    CHECK(std::isnan(to30.apply_cartesian(at(std::numeric_limits<double>::quiet_NaN(), 0.9, 0.0, false)).position.cartesian.X));
    // a reference screen across the rear seam
    const Screen seam = PolarScreen{1.78, PolarPosition(170.0, 0.0, 1.0), 58.0};
    CHECK_THROWS_AS(to30.apply_cartesian(at(0.1, 0.9, 0.0, true, seam)), ear::invalid_argument);
  }
  if (host_only) {
    return summary("host");
  }

  // the batch form: one device launch per reference screen, over two distinct ones; against the single form
  {
    const ScreenHandler to15(kPolar15);
    const char *hs[3] = {nullptr, "left", "right"}, *vs[3] = {nullptr, "bottom", "top"};
    std::vector<ObjectsTypeMetadata> blocks;
    std::vector<ScreenEdgeLock> locks;
    for (int i = 0; i < 203; i++) {
      // a spiral through the cube and beyond it: neighbours are at least 1e-2 apart, so a permuted index cannot hide
      const double t = 0.37 * i;
      ObjectsTypeMetadata m = at((0.3 + 0.008 * i) * std::sin(t), (0.3 + 0.008 * i) * std::cos(t), -1.5 + 0.015 * i, i % 3 != 0,
                                 i % 5 == 0 ? kCart : getDefaultScreen());
      m.gain = 0.01 * i, m.width = 0.001 * i;
      blocks.push_back(m);
      locks.push_back(lock(hs[i % 3], vs[(i / 3) % 3]));
    }
    double nearest = 1e9;
    for (size_t i = 0; i < blocks.size(); i++)
      for (size_t j = 0; j < i; j++) {
        const CartesianPosition &p = blocks[i].position.cartesian, &q = blocks[j].position.cartesian;
        nearest = std::fmin(nearest, std::fmax(std::fabs(p.X - q.X), std::fmax(std::fabs(p.Y - q.Y), std::fabs(p.Z - q.Z))));
      }
    CHECK(nearest >= 1e-2);
    for (int with_locks = 1; with_locks >= 0; with_locks--) {
      std::vector<ObjectsTypeMetadata> batch = blocks;
      if (with_locks)
        to15.apply_cartesian(batch, locks);
      else
        to15.apply_cartesian(batch);
      size_t differ = 0, untouched_differ = 0;
      double worst = 0.0;
      for (size_t i = 0; i < blocks.size(); i++) {
        const ObjectsTypeMetadata one = with_locks ? to15.apply_cartesian(blocks[i], locks[i]) : to15.apply_cartesian(blocks[i]);
        const CartesianPosition &p = one.position.cartesian, &q = batch[i].position.cartesian;
        const double d = std::fmax(std::fabs(p.X - q.X), std::fmax(std::fabs(p.Y - q.Y), std::fabs(p.Z - q.Z)));
        worst = std::fmax(worst, d);
        if (!(d <= 1e-6) || batch[i].screenRef || batch[i].gain != blocks[i].gain || batch[i].width != blocks[i].width) differ++;
        const bool flagged = blocks[i].screenRef || (with_locks && (locks[i].horizontal || locks[i].vertical));
        if (!flagged && !same_position(batch[i], blocks[i])) untouched_differ++;
      }
      std::printf("batch vs single (%s): %zu of %zu blocks differ, worst %.3g\n", with_locks ? "locks" : "no locks", differ,
                  blocks.size(), worst);
      CHECK(differ == 0);
      CHECK(untouched_differ == 0);
    }
    // an empty batch; the default-constructed handler
    std::vector<ObjectsTypeMetadata> none;
    to15.apply_cartesian(none);
    CHECK(none.empty());
    std::vector<ObjectsTypeMetadata> batch = blocks;
    ScreenHandler().apply_cartesian(batch, locks);
    size_t differ = 0;
    for (size_t i = 0; i < blocks.size(); i++)
      if (!same_position(batch[i], blocks[i]) || batch[i].screenRef) differ++;
    CHECK(differ == 0);
    // the batch refuses what the single form refuses, names a bad block and writes nothing
    batch = blocks;
    batch[77] = at(0.1, std::numeric_limits<double>::infinity(), 0.2);
    bool threw = false;
    try {
      to15.apply_cartesian(batch, locks);
    } catch (const ear::invalid_argument &e) {
      threw = std::string(e.what()).find("metadata block 77") != std::string::npos;
    }
    CHECK(threw && batch[0].screenRef == blocks[0].screenRef && same_position(batch[1], blocks[1]) && same_position(batch[202], blocks[202]));
    batch = blocks;
    batch[5].position = PolarPosition(0.0, 0.0, 1.0);
    CHECK_THROWS_AS(to15.apply_cartesian(batch, locks), ear::not_implemented);
    CHECK(same_position(batch[0], blocks[0]) && batch[1].screenRef == blocks[1].screenRef);
    batch = blocks;
    CHECK_THROWS_AS(to15.apply_cartesian(batch, std::vector<ScreenEdgeLock>(3)), ear::invalid_argument);
    std::vector<ScreenEdgeLock> bad_locks = locks;
    bad_locks[100] = lock("top", nullptr);
    CHECK_THROWS_AS(to15.apply_cartesian(batch, bad_locks), ear::adm_error);
    CHECK(same_position(batch[0], blocks[0]) && batch[1].screenRef == blocks[1].screenRef);

    // in front of the allocentric calculator: it refuses the raw blocks by field name and accepts the handler's result
    const Layout layout = getLayout("9+10+3");
    const ear::hip::AllocentricObjectsGainCalculator calc(layout);
    CHECK(calculator_refusal(calc, blocks, true) == "not implemented: screenRef");
    CHECK(calculator_refusal(calc, blocks, false) == "not implemented: screenRef");
    batch = blocks;
    to15.apply_cartesian(batch, locks);
    CHECK(calculator_refusal(calc, batch, true).empty());
    std::vector<std::vector<float>> direct, diffuse, host_direct, host_diffuse;
    calc.calculate_device(batch, direct, diffuse);
    calc.calculate(batch, host_direct, host_diffuse);
    CHECK(direct.size() == blocks.size() && direct[0].size() == layout.channels().size());
    double worst = 0.0;
    bool finite = true;
    for (size_t i = 0; i < direct.size(); i++)
      for (size_t c = 0; c < direct[i].size(); c++) {
        finite = finite && std::isfinite(direct[i][c]);
        worst = std::fmax(worst, std::fabs((double)direct[i][c] - host_direct[i][c]));
      }
    std::printf("calculate_device vs calculate on the handler's result: worst %.3g\n", worst);
    CHECK(finite && worst <= 2e-6);
  }
  return summary();
}
