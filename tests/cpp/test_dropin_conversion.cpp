// Drop-in test of ear::conversion: a libear application's lines, compiled against the C++14 mirror headers only
// (libear_amd/host/ear/...), restating the reference's own Catch2 cases (tests/conversion_tests.cpp) without
// Eigen/Catch2.  The single-element functions run on the calling thread and need no GPU; the batch overloads of
// toPolar / toCartesian need one, and without it they throw (no CPU fallback).
// Build (one line): g++ -std=c++14 -Iinclude -Ilibear_amd/host tests/cpp/test_dropin_conversion.cpp
//            -Llibear_amd/lib -learhip -Wl,-rpath,$PWD/libear_amd/lib -o test_dropin_conversion
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include <ear/conversion.hpp>

#include "dropin_check.h"

using namespace ear;
using namespace ear::conversion;


static bool near(double a, double b, double margin = 1e-6) { return std::fabs(a - b) <= margin; }
static bool polar_eq(const PolarPosition &a, const PolarPosition &b, double m = 1e-6) {
  return near(a.azimuth, b.azimuth, m) && near(a.elevation, b.elevation, m) && near(a.distance, b.distance, m);
}
static bool cart_eq(const CartesianPosition &a, const CartesianPosition &b, double m = 1e-6) {
  return near(a.X, b.X, m) && near(a.Y, b.Y, m) && near(a.Z, b.Z, m);
}
static bool extent_eq(const ExtentParams &a, const ExtentParams &b, double m = 1e-6) {
  return near(a.width, b.width, m) && near(a.height, b.height, m) && near(a.depth, b.depth, m);
}
static ExtentParams get_extent(const ObjectsTypeMetadata &otm) { return ExtentParams{otm.width, otm.height, otm.depth}; }

static void test_reference() {
  auto res = extentPolarToCart(PolarPosition{10.0, 20.0, 0.3}, ExtentParams{40.0, 50.0, 0.6});
  CHECK(cart_eq(res.first, CartesianPosition{-0.08972503721988338, 0.3, 0.1732050807568877}));
  CHECK(extent_eq(res.second, ExtentParams{0.35166171614357594, 0.4470181645863707, 0.5762749096794243}));
  auto res2 = extentCartToPolar(CartesianPosition{0.9, 0.8, 0.1}, ExtentParams{0.3, 0.5, 0.4});
  CHECK(polar_eq(res2.first, PolarPosition{-34.85107611658391, 4.226794497273273, 0.9000000000000001}));
  CHECK(extent_eq(res2.second, ExtentParams{76.50724453298275, 104.9708107421662, 0.1756348204517474}));
}

static void test_points() {
  for (double az : {0.0, -10.0, 10.0, 90.0, -90.0, 150.0, -150.0})
    for (double el : {0.0, -10.0, 10.0, -45.0, 45.0})
      for (double dist : {0.5, 1.0}) CHECK(polar_eq(pointCartToPolar(pointPolarToCart({az, el, dist})), {az, el, dist}));
  for (double sign : {-1.0, 1.0}) {
    CHECK(cart_eq(pointPolarToCart({0.0, sign * 90.0, 2.0}), {0.0, 0.0, sign * 2.0}));
    CHECK(polar_eq(pointCartToPolar({0.0, 0.0, sign * 2.0}), {0.0, sign * 90.0, 2.0}));
  }
  CHECK(near(pointCartToPolar({0.0, 0.0, 0.0}).distance, 0.0));
  // libear throws internal_error for a NaN azimuth; an infinite one is refused here (libear does not return)
  CHECK_THROWS_AS(pointPolarToCart({std::numeric_limits<double>::quiet_NaN(), 0.0, 1.0}), internal_error);
  CHECK_THROWS_AS(pointPolarToCart({std::numeric_limits<double>::infinity(), 0.0, 1.0}), invalid_argument);
}

static void test_wrappers() {
  {  // polar to cart
    ObjectsTypeMetadata otm;
    otm.position = PolarPosition{10.0, 20.0, 0.3};
    otm.cartesian = false;
    otm.width = 40.0, otm.height = 50.0, otm.depth = 0.6;
    ObjectsTypeMetadata otm_cart = otm;
    toCartesian(otm_cart);
    auto res = extentPolarToCart(otm.position.polar, get_extent(otm));
    CHECK(otm_cart.position.isCartesian && cart_eq(otm_cart.position.cartesian, res.first));
    CHECK(extent_eq(get_extent(otm_cart), res.second));
    CHECK(otm_cart.cartesian);
  }
  {  // fix cart flag, polar
    ObjectsTypeMetadata otm;
    otm.position = PolarPosition{10.0, 20.0, 0.3};
    otm.cartesian = true;
    toCartesian(otm);
    CHECK(otm.cartesian && otm.position.isCartesian);
  }
  {  // cart to polar
    ObjectsTypeMetadata otm;
    otm.position = CartesianPosition{0.9, 0.8, 0.1};
    otm.cartesian = true;
    otm.width = 0.3, otm.height = 0.5, otm.depth = 0.4;
    ObjectsTypeMetadata otm_polar = otm;
    toPolar(otm_polar);
    auto res = extentCartToPolar(otm.position.cartesian, get_extent(otm));
    CHECK(!otm_polar.position.isCartesian && polar_eq(otm_polar.position.polar, res.first));
    CHECK(extent_eq(get_extent(otm_polar), res.second));
    CHECK(!otm_polar.cartesian);
  }
  {  // fix cart flag, Cartesian
    ObjectsTypeMetadata otm;
    otm.position = CartesianPosition{0.9, 0.8, 0.1};
    otm.cartesian = false;
    toPolar(otm);
    CHECK(!otm.cartesian && !otm.position.isCartesian);
  }
}

// the batch overloads against single calls: positions and extents within 1e-9 (device and host transcendentals
// differ in the last bits), flags and variants as the single calls leave them
static void test_batch() {
  hip::Context ctx(0);
  std::vector<ObjectsTypeMetadata> md, single;
  unsigned s = 12345u;
  auto rnd = [&]() { return (s = s * 1664525u + 1013904223u) / 4294967296.0; };
  for (int i = 0; i < 4096; i++) {
    ObjectsTypeMetadata m;
    if (i % 3 == 0) {
      m.position = PolarPosition{rnd() * 360.0 - 180.0, rnd() * 180.0 - 90.0, rnd()};
      m.width = rnd() * 90.0, m.height = rnd() * 90.0;
      m.cartesian = (i % 2) == 0;  // wrong on purpose for half of them: the variant decides
    } else {
      m.position = CartesianPosition{rnd() * 2.0 - 1.0, rnd() * 2.0 - 1.0, rnd() * 2.0 - 1.0};
      m.width = rnd() * 0.9, m.height = rnd() * 0.9, m.depth = rnd() * 0.9;
      m.cartesian = (i % 2) == 1;
    }
    md.push_back(m);
  }
  single = md;
  for (auto &m : single) toPolar(m);
  std::vector<ObjectsTypeMetadata> batch = md;
  toPolar(batch, ctx);
  int bad = 0;
  for (size_t i = 0; i < md.size(); i++) {
    const ObjectsTypeMetadata &a = batch[i], &b = single[i];
    if (a.cartesian || a.position.isCartesian || !polar_eq(a.position.polar, b.position.polar, 1e-9) ||
        !extent_eq(get_extent(a), get_extent(b), 1e-9))
      bad++;
  }
  CHECK(bad == 0);
  std::vector<ObjectsTypeMetadata> back = batch, back_single = batch;
  toCartesian(back, ctx);
  for (auto &m : back_single) toCartesian(m);
  bad = 0;
  for (size_t i = 0; i < md.size(); i++)
    if (!back[i].cartesian || !back[i].position.isCartesian ||
        !cart_eq(back[i].position.cartesian, back_single[i].position.cartesian, 1e-9) ||
        !extent_eq(get_extent(back[i]), get_extent(back_single[i]), 1e-9))
      bad++;
  CHECK(bad == 0);
  // a failing element stops the batch, naming the metadata block
  std::vector<ObjectsTypeMetadata> broken(3);
  broken[2].position = PolarPosition{std::numeric_limits<double>::infinity(), 0.0, 1.0};
  bool thrown = false;
  try {
    toCartesian(broken, ctx);
  } catch (const invalid_argument &e) {
    thrown = std::string(e.what()).find("block 2") != std::string::npos;
  }
  CHECK(thrown);
}

int main() {
  try {
    test_reference();
    test_points();
    test_wrappers();
  } catch (const std::exception &e) {
    g_failed++;
    std::printf("FAILED: exception %s\n", e.what());
  }
  summary("single-element");
  try {
    test_batch();
  } catch (const std::exception &e) {
    g_failed++;
    std::printf("FAILED: batch: exception %s\n", e.what());
  }
  return summary();
}
