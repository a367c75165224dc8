// libear_amd/csrc/screen_cart.h on the host: apply_cart_one on the fixed points of group V's tests (the origin, the axes, the
// corners of the cube, -0.0 components, either side of the conversion's 1e-10 centre rule, the sector seams) against the three
// cores it composes called one after the other here, the pass-through of an element with no flag set, and the refusal codes.
// Built with hipcc (the headers are __host__ __device__ code), run on the CPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "screen_cart.h"

using namespace earhip;
using namespace earhip::screen;

static long g_checked = 0, g_failed = 0;

static void expect(bool ok, const char *what, const double p[3], const double got[3]) {
  g_checked++;
  if (!ok && g_failed++ < 20)
    std::printf("FAILED %s at (%.17g, %.17g, %.17g): got (%.17g, %.17g, %.17g)\n", what, p[0], p[1], p[2], got[0], got[1], got[2]);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same_bits3(const double a[3], const double b[3]) {
  return same_bits(a[0], b[0]) && same_bits(a[1], b[1]) && same_bits(a[2], b[2]);
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double points[][3] = {
      {0, 0, 0}, {0, 0, 1}, {0, 0, -1}, {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0},
      {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}, {-1, 1, 1}, {-1, 1, -1}, {-1, -1, 1}, {-1, -1, -1},
      {1, 1, 0}, {1, -1, 0}, {-1, 1, 0}, {-1, -1, 0},
      {-0.0, 1, 0}, {0.5, -0.0, 0.25}, {-0.0, -0.0, -0.0}, {0.3, 0.4, -0.0}, {-0.0, -0.0, 0.75},
      {1e-300, 1, 0}, {0, -1, 1e-12}, {5e-11, 5e-11, 0.5}, {2e-10, 0, 0.5},
      {0, 0.5, 0.3}, {0.5, 0.5, 0.3}, {-0.5, 0.5, -0.3}, {1.5, -1.5, 0.25}, {-1.5, -1.5, -2}, {0, -0.75, 0.1}};
  // edges: left, right, bottom, top.  The default screen, a 30 degree screen, an off-centre one, a narrow high one
  const double screens[4][4] = {{29.0, -29.0, -17.29708889245067, 17.29708889245067},
                                {15.0, -15.0, -8.560644163419065, 8.560644163419065},
                                {0.283559454529715, -40.283559454529716, -3.639039283545732, 23.63903928354573},
                                {-54.0, -66.0, 19.5, 30.25}};
  for (int r = 0; r < 4; r++)
    for (int p = 0; p < 4; p++) {
      const Map m = make_map(screens[r], screens[p]);
      for (const double *q : points) {
        for (unsigned ref = 0; ref < 2; ref++)
          for (unsigned lh = 0; lh < 3; lh++)
            for (unsigned lv = 0; lv < 3; lv++) {
              double got[3] = {7, 7, 7};
              const int st = apply_cart_one(m, q[0], q[1], q[2], ref, lh, lv, got);
              if (!ref && !lh && !lv) {
                expect(st == EARHIP_OK && same_bits3(got, q), "no flag: the input's bits", q, got);
                continue;
              }
              // the composition, spelt out
              double polar[3], az, el, want[3];
              const bool ok = conv::point_cart_to_polar(q[0], q[1], q[2], polar) == EARHIP_OK &&
                              apply_one(m, polar[0], polar[1], ref, lh, lv, az, el) == 0 &&
                              conv::point_polar_to_cart(az, el, polar[2], want) == EARHIP_OK;
              expect(ok && st == EARHIP_OK && same_bits3(got, want), "the three cores chained", q, got);
              expect(std::isfinite(got[0]) && std::isfinite(got[1]) && std::isfinite(got[2]), "finite", q, got);
              if (lh == 0 && lv == 0 && r == p) {  // equal screens: the two conversions undo each other
                expect(std::fabs(got[0] - q[0]) <= 1e-9 && std::fabs(got[1] - q[1]) <= 1e-9 && std::fabs(got[2] - q[2]) <= 1e-9,
                       "equal screens", q, got);
              }
              if (q[0] == 0 && q[1] == 0 && q[2] == 0) expect(got[0] == 0 && got[1] == 0 && got[2] == 0, "the origin", q, got);
              if (q[0] == 0 && q[1] == 0 && q[2] != 0 && lv == 0)
                expect(got[0] == 0 && got[1] == 0 && same_bits(got[2], q[2]), "the z axis", q, got);
            }
      }
      // an element with no flag set is not looked at; with a flag it is refused, and its outputs are its inputs
      const double odd[][3] = {{nan, 1, 0}, {0, inf, 0}, {0, 0, -inf}, {nan, nan, nan}};
      for (const double *q : odd) {
        double got[3] = {7, 7, 7};
        expect(apply_cart_one(m, q[0], q[1], q[2], 0, 0, 0, got) == EARHIP_OK && same_bits3(got, q), "no flag: not looked at", q, got);
        expect(apply_cart_one(m, q[0], q[1], q[2], 1, 0, 0, got) == EARHIP_INVALID_ARGUMENT && same_bits3(got, q), "refused", q, got);
        expect(apply_cart_one(m, q[0], q[1], q[2], 0, 2, 0, got) == EARHIP_INVALID_ARGUMENT, "refused under a lock", q, got);
        expect(apply_cart_one(m, q[0], q[1], q[2], 0, 0, 1, got) == EARHIP_INVALID_ARGUMENT, "refused under a lock", q, got);
        expect(apply_cart_one(identity_map(), q[0], q[1], q[2], 1, 3, 3, got) == EARHIP_OK && same_bits3(got, q), "identity", q, got);
      }
      const double q[3] = {0.25, 0.5, 0.125};
      double got[3];
      expect(apply_cart_one(m, q[0], q[1], q[2], 0, 3, 0, got) == EARHIP_INVALID_ARGUMENT && same_bits3(got, q), "lock code 3", q, got);
      expect(apply_cart_one(m, q[0], q[1], q[2], 1, 0, 255, got) == EARHIP_INVALID_ARGUMENT, "lock code 255", q, got);
      expect(apply_cart_one(m, q[0], q[1], q[2], 1, 2, 2, got) == EARHIP_OK, "lock code 2", q, got);
    }
  std::printf("%ld checked, %ld failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
