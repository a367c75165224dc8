// libear_amd/csrc/screen.h on the host: the segment the piecewise-linear maps choose at and next to every breakpoint, the
// clamps at 180 and 90, the reduction of the azimuth, and apply_one's rules for flags, locks and refused elements — against a
// plain search over the breakpoints written here.  Built with hipcc (the header is __host__ __device__ code), run on the CPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "screen.h"

using namespace earhip::screen;

static long g_checked = 0, g_failed = 0;

static void expect(bool ok, const char *what, double x, double got, double want) {
  g_checked++;
  if (!ok && g_failed++ < 20) std::printf("FAILED %s at %.17g: got %.17g, want %.17g\n", what, x, got, want);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the value by definition: the last breakpoint <= x, by a search from the top over all four
static double by_definition(const double bx[4], const double by[4], double x) {
  if (x >= bx[3]) return bx[3];
  int k = 2;
  while (k > 0 && !(bx[k] <= x)) k--;
  const double slope = (by[k + 1] - by[k]) / (bx[k + 1] - bx[k]);
  return std::fma(slope, x - bx[k], by[k]);
}

static void check_map(const Segment s[3], const double bx[4], const double by[4], const char *what) {
  const double inf = std::numeric_limits<double>::infinity();
  for (int k = 0; k < 4; k++) {
    // at the breakpoint: exactly the image breakpoint; the segment that starts there (the last one ends the range)
    expect(same_bits(map_value(s, bx[3], bx[k]), by[k]), what, bx[k], map_value(s, bx[3], bx[k]), by[k]);
    if (k < 3) expect(segment_of(s, bx[k]) == k, "segment at a breakpoint", bx[k], segment_of(s, bx[k]), k);
    // next to it, below and above
    const double lo = std::nextafter(bx[k], -inf), hi = std::nextafter(bx[k], inf);
    if (k > 0) {
      expect(segment_of(s, lo) == k - 1, "segment below a breakpoint", lo, segment_of(s, lo), k - 1);
      expect(same_bits(map_value(s, bx[3], lo), by_definition(bx, by, lo)), what, lo, map_value(s, bx[3], lo),
             by_definition(bx, by, lo));
    }
    if (k < 3) {
      expect(segment_of(s, hi) == k, "segment above a breakpoint", hi, segment_of(s, hi), k);
      expect(same_bits(map_value(s, bx[3], hi), by_definition(bx, by, hi)), what, hi, map_value(s, bx[3], hi),
             by_definition(bx, by, hi));
    } else {
      expect(map_value(s, bx[3], hi) == bx[3], "clamp above the range", hi, map_value(s, bx[3], hi), bx[3]);
    }
  }
  // a sweep of the whole range: the definition's bits, and the map never leaves the range or runs backwards
  double prev = by[0];
  for (int i = 0; i <= 7200; i++) {
    const double x = bx[0] + (bx[3] - bx[0]) * i / 7200.0;
    const double y = map_value(s, bx[3], x);
    expect(same_bits(y, by_definition(bx, by, x)), what, x, y, by_definition(bx, by, x));
    expect(y >= by[0] && y <= by[3] && y >= prev - 1e-12, "monotone and in range", x, y, prev);
    prev = y;
  }
}

int main() {
  // edges: left, right, bottom, top.  The default screen, a 30 degree screen, an off-centre one, a narrow high one
  const double screens[4][4] = {{29.0, -29.0, -17.29708889245067, 17.29708889245067},
                                {15.0, -15.0, -8.560644163419065, 8.560644163419065},
                                {0.283559454529715, -40.283559454529716, -3.639039283545732, 23.63903928354573},
                                {-54.0, -66.0, 19.5, 30.25}};
  for (int r = 0; r < 4; r++)
    for (int p = 0; p < 4; p++) {
      const double *ref = screens[r], *rep = screens[p];
      const Map m = make_map(ref, rep);
      const double ax[4] = {-180.0, ref[1], ref[0], 180.0}, ay[4] = {-180.0, rep[1], rep[0], 180.0};
      const double ex[4] = {-90.0, ref[2], ref[3], 90.0}, ey[4] = {-90.0, rep[2], rep[3], 90.0};
      check_map(m.az, ax, ay, "azimuth map");
      check_map(m.el, ex, ey, "elevation map");

      double az, el;
      // scaled: the seam and the poles, a reference edge, an azimuth beyond a turn
      expect(apply_one(m, 180.0, 90.0, 1, 0, 0, az, el) == 0 && az == 180.0 && el == 90.0, "seam and pole", 180.0, az, 180.0);
      expect(apply_one(m, -180.0, -90.0, 1, 0, 0, az, el) == 0 && az == -180.0 && el == -90.0, "seam and pole", -180.0, az, -180.0);
      expect(apply_one(m, ref[0], ref[3], 1, 0, 0, az, el) == 0 && az == rep[0] && el == rep[3], "edge to edge", ref[0], az, rep[0]);
      expect(apply_one(m, ref[1] + 720.0, ref[2], 1, 0, 0, az, el) == 0 && el == rep[2], "edge to edge", ref[2], el, rep[2]);
      const double turned = std::fmod(ref[1] + 720.0, 360.0) - 360.0;  // ref[1] < 0: the fmod lands above 180
      expect(same_bits(az, by_definition(ax, ay, turned)), "beyond a turn", ref[1] + 720.0, az, by_definition(ax, ay, turned));
      // locks after the scale; an untouched component keeps its bits
      expect(apply_one(m, 400.0, 12.0, 0, 0, 2, az, el) == 0 && az == 400.0 && el == rep[3], "vertical lock alone", 400.0, az, 400.0);
      expect(apply_one(m, 400.0, 12.0, 0, 1, 0, az, el) == 0 && az == rep[0] && el == 12.0, "horizontal lock alone", 12.0, el, 12.0);
      expect(apply_one(m, 10.0, 12.0, 1, 2, 1, az, el) == 0 && az == rep[1] && el == rep[2], "both locks", 10.0, az, rep[1]);
      // refused, and only when a flag is set
      const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
      expect(apply_one(m, nan, 0.0, 1, 0, 0, az, el) == 1, "NaN azimuth", nan, 0, 1);
      expect(apply_one(m, inf, 0.0, 0, 1, 0, az, el) == 1, "infinite azimuth", inf, 0, 1);
      expect(apply_one(m, 2.0 * kMaxAzimuth, 0.0, 1, 0, 0, az, el) == 1, "huge azimuth", 2.0 * kMaxAzimuth, 0, 1);
      expect(apply_one(m, kMaxAzimuth, 0.0, 1, 0, 0, az, el) == 0, "2^40", kMaxAzimuth, 1, 0);
      expect(apply_one(m, 0.0, std::nextafter(90.0, inf), 1, 0, 0, az, el) == 1, "elevation above 90", 90.0, 0, 1);
      expect(apply_one(m, 0.0, nan, 0, 0, 1, az, el) == 1, "NaN elevation", nan, 0, 1);
      expect(apply_one(m, 0.0, 0.0, 0, 3, 0, az, el) == 1 && apply_one(m, 0.0, 0.0, 1, 0, 3, az, el) == 1, "lock code 3", 3, 0, 1);
      expect(apply_one(m, nan, inf, 0, 0, 0, az, el) == 0 && std::isnan(az) && el == inf, "no flag: not looked at", nan, az, nan);
      const Map id = identity_map();
      expect(apply_one(id, nan, 123.0, 1, 3, 3, az, el) == 0 && std::isnan(az) && el == 123.0, "identity", nan, az, nan);
    }
  // the reduction: into [-180, 180], exact, the seam kept where it is
  const double in[] = {0.0, 180.0, -180.0, 180.00000000000003, 360.0, 389.0, -389.0, 540.0, -540.0, 1e9 + 0.5, 1099511627776.0};
  const double out[] = {0.0, 180.0, -180.0, -179.99999999999997, 0.0, 29.0, -29.0, 180.0, -180.0, 280.5 - 360.0, 16.0};
  for (unsigned i = 0; i < sizeof in / sizeof *in; i++)
    expect(reduce_azimuth(in[i]) == out[i], "reduce_azimuth", in[i], reduce_azimuth(in[i]), out[i]);
  std::printf("%ld checked, %ld failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
