// The plain parts of libear_amd/host/ear/hip_batch.hpp on the host, under ASan and UBSan, with no library to link: the carver
// over malloc'ed memory with the array lists of the five device batches (the `Arrays` of hip_allo.hpp, hip_allo_objects.hpp,
// hip_hoa.hpp, hip_screen.hpp and conversion.hpp themselves), the scatter of a layout binding and the zone conversion.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <ear/conversion.hpp>
#include <ear/hip_allo.hpp>
#include <ear/hip_allo_objects.hpp>
#include <ear/hip_hoa.hpp>
#include <ear/hip_screen.hpp>

#include "dropin_check.h"

using namespace ear;
using ear::detail::Carver;

struct Span {
  const void *p;
  size_t bytes, align;
};
template <typename T>
static Span span(const T *p, size_t count) {
  return Span{p, count * sizeof(T), alignof(T)};
}

static std::vector<Span> spans(const hip::AllocentricGainCalculator::Arrays &a, size_t n, size_t nf) {
  return {span(a.x, n),        span(a.y, n),      span(a.z, n),      span(a.gain, n), span(a.diffuse, n),
          span(a.excluded, n), span(a.status, n), span(a.d, n * nf), span(a.f, n * nf)};
}
static std::vector<Span> spans(const hip::AllocentricObjectsGainCalculator::Arrays &a, size_t n, size_t nf) {
  std::vector<Span> s;
  for (double *v : a.v) s.push_back(span(v, n));
  for (const Span &t : {span(a.excluded, n), span(a.status, n), span(a.d, n * nf), span(a.f, n * nf), span(a.lock, n)}) s.push_back(t);
  return s;
}
static std::vector<Span> spans(const hip::HOAEncoder::Arrays &a, size_t n, size_t nc) {
  return {span(a.az, n), span(a.el, n), span(a.gain, n), span(a.out, n * nc), span(a.status, n)};
}
static std::vector<Span> spans(const hip::ScreenHandler::Arrays &a, size_t n) {
  return {span(a.az, n), span(a.el, n), span(a.status, n), span(a.ref, n), span(a.h, n), span(a.v, n)};
}
static std::vector<Span> spans(const conversion::detail::Arrays &a, size_t n) {
  std::vector<Span> s;
  for (double *v : a.a) s.push_back(span(v, n));
  s.push_back(span(a.status, n));
  return s;
}

// One site: its block sized by its own takes, carved, every array written.  asked: the byte count of the expression the site
// had before there was a carver.
template <typename Arrays, typename... Sizes>
static void check_site(size_t asked, Sizes... sizes) {
  const size_t bytes = Carver::bytes_for<Arrays>(sizes...);
  CHECK(bytes <= asked);
  unsigned char *mem = static_cast<unsigned char *>(std::malloc(bytes));
  Carver carver(mem, bytes);
  const Arrays arrays(carver, sizes...);
  CHECK(carver.used() == bytes);
  const unsigned char *next = mem;
  for (const Span &s : spans(arrays, sizes...)) {
    CHECK(reinterpret_cast<uintptr_t>(s.p) % s.align == 0);
    CHECK(s.p == next);  // in order, nothing between them, none over another
    std::memset(const_cast<void *>(s.p), 0xa5, s.bytes);
    next += s.bytes;
  }
  CHECK(next == mem + bytes);
  // the block is used up: one more byte is refused
  CHECK_THROWS_AS(carver.take<unsigned char>(1), internal_error);
  std::free(mem);
}

struct Misordered {  // a byte array of 3, then doubles
  explicit Misordered(Carver &c) : bytes(c.take<uint8_t>(3)), doubles(c.take<double>(1)) {}
  uint8_t *bytes;
  double *doubles;
};

int main() {
  const size_t nf = 11, nc = 9;  // odd, so that only the order of the arrays keeps the 8-byte ones aligned
  for (size_t n : {1u, 3u, 67u}) {
    check_site<hip::AllocentricGainCalculator::Arrays>(n * (5 * sizeof(double) + sizeof(uint32_t) + sizeof(int) + 2 * nf * sizeof(float)), n, nf);
    check_site<hip::AllocentricObjectsGainCalculator::Arrays>(
        n * (11 * sizeof(double) + sizeof(uint32_t) + sizeof(int) + 2 * nf * sizeof(float) + 1), n, nf);
    check_site<hip::HOAEncoder::Arrays>(n * (3 * sizeof(double) + sizeof(int) + nc * sizeof(float)), n, nc);
    check_site<hip::ScreenHandler::Arrays>(n * (2 * sizeof(double) + sizeof(int) + 3), n);
    check_site<conversion::detail::Arrays>(n * (6 * sizeof(double) + sizeof(int)), n);
  }
  // a list in the wrong order is refused when it is sized and when it is carved, not handed out
  CHECK_THROWS_AS(Carver::bytes_for<Misordered>(), internal_error);
  {
    void *mem = std::malloc(16);
    Carver carver(mem, 16);
    CHECK_THROWS_AS(Misordered m(carver), internal_error);
    CHECK(carver.used() == 3);
    std::free(mem);
  }
  // the layout binding: rows of the native layout's 3 channels -> the caller's 2, in the caller's order
  {
    detail::LayoutBinding b;
    b.keep = {2, 0}, b.n_full = 3;
    const float rows[6] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f};
    std::vector<std::vector<double>> out(5, std::vector<double>(7, -1.0));
    b.scatter(2, rows, out);
    CHECK(out == (std::vector<std::vector<double>>{{3.0, 1.0}, {6.0, 4.0}}));
    b.scatter(0, rows, out);
    CHECK(out.empty());
    b.check_size(2, 2);
    CHECK_THROWS_AS(b.check_size(3, 2), invalid_argument);
    CHECK_THROWS_AS(b.check_size(2, 1), invalid_argument);
  }
  // the zone conversion fills all ten bounds, whichever kind the zone is
  {
    ExclusionZone z(CartesianExclusionZone{5.0f, 6.0f, 7.0f, 8.0f, 9.0f, 10.0f, "c"});
    z.polar = PolarExclusionZone{1.0f, 2.0f, 3.0f, 4.0f, 0.0f, 1.0f, "p"};
    earhip_exclusion_zone c = detail::to_c(z);
    CHECK(c.cartesian == 1 && c.min_azimuth == 1.0 && c.max_azimuth == 2.0 && c.min_elevation == 3.0 && c.max_elevation == 4.0);
    CHECK(c.min_x == 5.0 && c.max_x == 6.0 && c.min_y == 7.0 && c.max_y == 8.0 && c.min_z == 9.0 && c.max_z == 10.0);
    z.isCartesian = false;
    c = detail::to_c(z);
    CHECK(c.cartesian == 0 && c.min_azimuth == 1.0 && c.max_elevation == 4.0 && c.min_x == 5.0 && c.max_z == 10.0);
  }
  return summary();
}
