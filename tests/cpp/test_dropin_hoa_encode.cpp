// ear::hip::HOAEncoder (libear_amd/host/ear/hip_hoa.hpp): Objects metadata -> the gain vectors of an Ambisonics bus, and the
// rotation of the bus, written against the mirror headers alone.  The expected values are the known answers of
// include/earhip.h group Q.  Compiles as C++14 with -Wall -Wextra -Werror.  `test_dropin_hoa_encode host` runs what needs no
// device (the single-element path, the refusals, the rotation); without an argument the batch path runs too, on a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <ear/hip_hoa.hpp>

#include "dropin_check.h"

using namespace ear;
using ear::hip::HOAEncoder;


static void acn(int order, std::vector<int> &orders, std::vector<int> &degrees) {
  for (int n = 0; n <= order; n++)
    for (int m = -n; m <= n; m++) orders.push_back(n), degrees.push_back(m);
}

static ObjectsTypeMetadata at(double az, double el, double gain = 1.0) {
  ObjectsTypeMetadata m;
  m.position = PolarPosition(az, el, 1.0);
  m.gain = gain;
  return m;
}

static bool refuses(const HOAEncoder &enc, const ObjectsTypeMetadata &m) {
  std::vector<float> g;
  try {
    enc.calculate(m, g);
  } catch (const ear::not_implemented &) {
    return true;
  }
  return false;
}

static bool refuses_batch(const HOAEncoder &enc, const ObjectsTypeMetadata &m) {
  std::vector<std::vector<float>> g;
  try {
    enc.calculate(std::vector<ObjectsTypeMetadata>(3, m), g);
  } catch (const ear::not_implemented &) {
    return true;
  }
  return false;
}

static std::vector<ObjectsTypeMetadata> refused_blocks() {
  std::vector<ObjectsTypeMetadata> v;
  ObjectsTypeMetadata m = at(10.0, 5.0);
  m.position = CartesianPosition(0.1, 0.9, 0.0);
  v.push_back(m);
  m = at(10.0, 5.0), m.cartesian = true, v.push_back(m);
  m = at(10.0, 5.0), m.width = 20.0, v.push_back(m);
  m = at(10.0, 5.0), m.height = 20.0, v.push_back(m);
  m = at(10.0, 5.0), m.depth = 0.2, v.push_back(m);
  m = at(10.0, 5.0), m.diffuse = 0.5, v.push_back(m);
  m = at(10.0, 5.0), m.channelLock.flag = true, v.push_back(m);
  m = at(10.0, 5.0), m.objectDivergence = PolarObjectDivergence(0.5, 30.0), v.push_back(m);
  m = at(10.0, 5.0), m.zoneExclusion.zones.push_back(PolarExclusionZone{-30.0f, 30.0f, -10.0f, 10.0f, 0.0f, 2.0f, "front"}), v.push_back(m);
  m = at(10.0, 5.0), m.screenRef = true, v.push_back(m);
  return v;
}

int main(int argc, char **argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "host") == 0;
  const float ulp1 = 1.1920929e-7f;  // the float32 spacing at 1
  std::vector<int> o1, d1, o3, d3, o7, d7;
  acn(1, o1, d1), acn(3, o3, d3), acn(7, o7, d7);

  // W for the three norms; the gain multiplies
  for (const char *norm : {"N3D", "SN3D", "FuMa"}) {
    const HOAEncoder w(std::vector<int>{0}, std::vector<int>{0}, norm);
    std::vector<float> g;
    w.calculate(at(-70.0, 40.0, 0.5), g);
    const float want = std::strcmp(norm, "FuMa") == 0 ? (float)(0.5 / std::sqrt(2.0)) : 0.5f;
    CHECK(g.size() == 1 && g[0] == want);
  }
  // N3D at az 90, el 0: Y_1^-1 = sqrt3, Y_1^0 and Y_1^1 vanish to the floor
  {
    const HOAEncoder enc(o1, d1, "N3D");
    std::vector<double> g;
    enc.calculate(at(90.0, 0.0), g);
    CHECK(g.size() == 4 && g[0] == 1.0);
    CHECK(std::fabs(g[1] - std::sqrt(3.0)) <= 2.0 * ulp1);
    CHECK(std::fabs(g[2]) <= std::ldexp(1.0, -43) && std::fabs(g[3]) <= std::ldexp(1.0, -43));
  }
  // FuMa W X Y Z, permuted, with a repeated channel: X front, Y left, Z up
  {
    const HOAEncoder enc(std::vector<int>{1, 0, 1, 0, 1}, std::vector<int>{0, 0, -1, 0, 1}, "FuMa");  // Z W Y W X
    std::vector<float> g;
    enc.calculate(at(30.0, 20.0), g);
    const double a = 30.0 * M_PI / 180.0, e = 20.0 * M_PI / 180.0;
    CHECK(g.size() == 5 && g[1] == g[3] && g[1] == (float)(1.0 / std::sqrt(2.0)));
    CHECK(std::fabs(g[0] - std::sin(e)) <= ulp1);
    CHECK(std::fabs(g[2] - std::sin(a) * std::cos(e)) <= ulp1);
    CHECK(std::fabs(g[4] - std::cos(a) * std::cos(e)) <= ulp1);
  }
  // what the bus cannot carry is refused, not dropped
  {
    const HOAEncoder enc(o3, d3);
    CHECK(!refuses(enc, at(10.0, 5.0)));
    for (const ObjectsTypeMetadata &m : refused_blocks()) CHECK(refuses(enc, m));
    // a zero divergence and a zero extent are no divergence and no extent
    ObjectsTypeMetadata m = at(10.0, 5.0);
    m.objectDivergence = PolarObjectDivergence(0.0, 30.0);
    CHECK(!refuses(enc, m));
  }
  // status codes as exceptions
  {
    CHECK_THROWS_AS(HOAEncoder bad(o1, d1, "foo"), ear::adm_error);
    CHECK_THROWS_AS(HOAEncoder bad(std::vector<int>{4}, std::vector<int>{0}, "FuMa"), ear::invalid_argument);
    CHECK_THROWS_AS(HOAEncoder bad(std::vector<int>{1, 1}, std::vector<int>{0}), ear::invalid_argument);
    const HOAEncoder enc(o1, d1);
    std::vector<float> g;
    CHECK_THROWS_AS(enc.calculate(at(10.0, 91.0), g), ear::invalid_argument);
  }
  // rotation(): a yaw of 90 degrees against the closed form enc(az + 90), order 7 N3D; and a q that is no rotation
  {
    const HOAEncoder enc(o7, d7, "N3D");
    const double q[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    const std::vector<std::vector<double>> R = enc.rotation<double>(q);
    CHECK(R.size() == 64 && R[0].size() == 64);
    const double src[4][2] = {{20.0, 10.0}, {-135.0, -40.0}, {75.0, 80.0}, {179.0, 0.0}};
    double worst = 0.0;
    for (const double *p : src) {
      std::vector<double> e, want;
      enc.calculate(at(p[0], p[1]), e);
      enc.calculate(at(p[0] + 90.0, p[1]), want);
      for (size_t i = 0; i < 64; i++) {
        double got = 0.0, mag = 0.0;
        for (size_t j = 0; j < 64; j++) got += R[i][j] * e[j], mag += std::fabs(R[i][j] * e[j]);
        const double bar = std::ldexp(mag, -22) + std::ldexp(std::fabs(want[i]), -23) + 1e-10;
        worst = std::fmax(worst, std::fabs(got - want[i]) / bar);
      }
    }
    std::printf("yaw 90: worst error %.3f of the bar\n", worst);
    CHECK(worst <= 1.0);
    bool cross_zero = true;
    for (size_t i = 0; i < 64; i++)
      for (size_t j = 0; j < 64; j++)
        if (o7[i] != o7[j] && R[i][j] != 0.0) cross_zero = false;
    CHECK(cross_zero);
    const double mirror[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0};
    CHECK_THROWS_AS(enc.rotation(mirror), ear::invalid_argument);
  }
  if (host_only) {
    return summary("host");
  }

  // the batch path (one device launch) equals the single-element path bit for bit, at fixed positions: the two run one core
  // and differ only in the math library, whose results differ by an ulp of a double at most — far inside a float's rounding
  {
    const HOAEncoder enc(o7, d7, "SN3D");
    std::vector<ObjectsTypeMetadata> blocks;
    for (int i = 0; i < 131; i++) blocks.push_back(at(-180.0 + 2.75 * i, -90.0 + 1.375 * i, 0.25 + 0.01 * i));
    std::vector<std::vector<float>> batch;
    enc.calculate(blocks, batch);
    CHECK(batch.size() == blocks.size());
    size_t differ = 0;
    for (size_t i = 0; i < blocks.size() && i < batch.size(); i++) {
      std::vector<float> one;
      enc.calculate(blocks[i], one);
      if (batch[i].size() != 64 || std::memcmp(one.data(), batch[i].data(), 64 * sizeof(float)) != 0) differ++;
    }
    std::printf("batch vs single: %zu of %zu rows differ\n", differ, blocks.size());
    CHECK(differ == 0);
    // the batch refuses what the single form refuses, and names a bad element
    for (const ObjectsTypeMetadata &m : refused_blocks()) CHECK(refuses_batch(enc, m));
    blocks[77] = at(0.0, 90.0000001);
    bool threw = false;
    try {
      enc.calculate(blocks, batch);
    } catch (const ear::invalid_argument &e) {
      threw = std::string(e.what()).find("metadata block 77") != std::string::npos;
    }
    CHECK(threw);
    std::vector<std::vector<double>> none;
    enc.calculate(std::vector<ObjectsTypeMetadata>(), none);
    CHECK(none.empty());
  }
  return summary();
}
