// libear_amd/csrc/true_peak.h on the CPU: the table a meter or a limiter is made with (tp_table_make) — annex 2's for the rates
// it serves, a caller's table of every admitted shape, h filled for the 4 x 12 shape alone, and every refusal with its message.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "true_peak.h"

using namespace earhip;

static int bad = 0;

static void expect(bool ok, const char *what) {
  if (!ok) printf("FAILED: %s\n", what), bad++;
}

static bool h_is_zero(const TpTable &t) {
  for (int p = 0; p < 4; p++)
    for (int k = 0; k < 12; k++)
      if (t.h[p][k] != 0.0f || std::signbit(t.h[p][k])) return false;
  return true;
}

// a caller's phases x taps table of distinct values that are not floats: it must come back rounded to float, in order
static void round_trip(int phases, int taps) {
  std::vector<double> c((size_t)phases * (size_t)taps);
  for (size_t i = 0; i < c.size(); i++) c[i] = 0.1 * (double)(i + 1) - 3.0;
  const earhip_true_peak tp = {phases, taps, c.data()};
  TpTable t;
  const char *why = tp_table_make(&tp, 96000, &t);  // (a caller's table serves any rate)
  expect(why == nullptr, "a caller's table of an admitted shape is accepted");
  if (why) return;
  expect(t.phases == phases && t.taps == taps && t.v.size() == c.size(), "the shape round-trips");
  bool same = true;
  for (size_t i = 0; i < c.size(); i++) same = same && t.v[i] == (float)c[i];
  expect(same, "the coefficients round-trip, rounded to float");
  if (phases == 4 && taps == 12) expect(std::memcmp(t.h, t.v.data(), sizeof(t.h)) == 0, "h holds a 4 x 12 table");
  else expect(h_is_zero(t), "h is zero for a shape other than 4 x 12");
}

static void refused(const earhip_true_peak *tp, int rate, const char *message, const char *what) {
  TpTable t;
  const char *why = tp_table_make(tp, rate, &t);
  expect(why != nullptr && std::strcmp(why, message) == 0, what);
  if (why && std::strcmp(why, message) != 0) printf("  got: %s\n", why);
}

int main() {
  double want[4][12];
  true_peak_default_table(want);
  const earhip_true_peak no_coeffs = {7, 99, nullptr};  // (phases and taps are ignored without coefficients)
  const earhip_true_peak *builtin[2] = {nullptr, &no_coeffs};
  for (int rate : {44100, 48000})
    for (const earhip_true_peak *tp : builtin) {
      TpTable t;
      expect(tp_table_make(tp, rate, &t) == nullptr, "the built-in table serves 44100 and 48000 Hz");
      expect(t.phases == 4 && t.taps == 12 && t.v.size() == 48, "the built-in table is 4 x 12");
      bool same = t.v.size() == 48;
      for (int i = 0; same && i < 48; i++) same = t.v[(size_t)i] == (float)want[i / 12][i % 12] && t.h[i / 12][i % 12] == t.v[(size_t)i];
      expect(same, "the built-in table is true_peak_default_table rounded to float, in v and in h");
    }

  round_trip(8, 64);
  round_trip(1, 1);
  round_trip(4, 12);
  round_trip(2, 24);

  std::vector<double> c((size_t)9 * 65, 0.25);
  const char *const phases_msg = "true peak: phases must be in [1, 8]", *const taps_msg = "true peak: taps must be in [1, 64]";
  const char *const finite_msg = "true peak: coefficients must be finite";
  for (int phases : {0, 9}) {
    const earhip_true_peak tp = {phases, 12, c.data()};
    refused(&tp, 48000, phases_msg, "phases outside [1, 8] are refused");
  }
  for (int taps : {0, 65}) {
    const earhip_true_peak tp = {4, taps, c.data()};
    refused(&tp, 48000, taps_msg, "taps outside [1, 64] are refused");
  }
  {
    std::vector<double> n(48, 0.25);
    n[47] = std::numeric_limits<double>::quiet_NaN();
    const earhip_true_peak tp = {4, 12, n.data()};
    refused(&tp, 48000, finite_msg, "a NaN is refused");
    n[47] = 0.25, n[0] = 1e39;  // finite as double, infinite as float
    refused(&tp, 48000, finite_msg, "a double that overflows float is refused");
    n[0] = -std::numeric_limits<double>::infinity();
    refused(&tp, 48000, finite_msg, "an infinity is refused");
  }
  refused(nullptr, 96000, "the built-in true-peak table is 4x oversampling for 44100 and 48000 Hz: another rate must bring its own",
          "96000 Hz without a table is refused");
  refused(&no_coeffs, 96000, "the built-in true-peak table is 4x oversampling for 44100 and 48000 Hz: another rate must bring its own",
          "96000 Hz with a table without coefficients is refused");
  printf("true-peak tables: %d problem(s)\n", bad);
  return bad ? 1 : 0;
}
