// libear_amd/csrc/hoa_encode.h on the host: encode_position (every channel of a list in one walk: what the host form and the
// kernel run) gives each channel exactly once and, bit for bit, the value encode_one computes for that channel alone with
// legendre_nm — for ACN lists, subsets, permutations and repetitions of every length up to 64, the three norms, random
// positions and the poles.  Built with hipcc (the header is __host__ __device__ code), run on the CPU.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hoa_encode.h"

using namespace earhip::hoa;

int main() {
  std::mt19937_64 rng(64);
  std::uniform_real_distribution<double> uaz(-400.0, 400.0), uel(-90.0, 90.0), ug(-2.0, 2.0);
  long checked = 0, failed = 0;
  for (int trial = 0; trial < 400; trial++) {
    const HoaNorm norm = (HoaNorm)(trial % 3);
    const int max_order = norm == kFuMa ? 3 : kMaxOrder;
    const int n_coef = trial < 64 ? trial + 1 : 1 + (int)(rng() % kMaxCoef);
    int orders[kMaxCoef], degrees[kMaxCoef];
    for (int c = 0; c < n_coef; c++) {
      if (trial % 5 == 0 && c < (max_order + 1) * (max_order + 1)) {  // ACN
        int n = 0;
        while ((n + 1) * (n + 1) <= c) n++;
        orders[c] = n, degrees[c] = c - n * n - n;
      } else {  // anything, repetitions included
        orders[c] = (int)(rng() % (unsigned)(max_order + 1));
        degrees[c] = (int)(rng() % (unsigned)(2 * orders[c] + 1)) - orders[c];
      }
    }
    Table t;
    fill_table(t, n_coef, orders, degrees, norm);
    for (int k = 0; k < 8; k++) {
      const double az = k == 0 ? 1e6 : uaz(rng), el = k == 1 ? 90.0 : (k == 2 ? -90.0 : uel(rng)), gain = k == 3 ? 1.0 : ug(rng);
      double got[kMaxCoef];
      int seen[kMaxCoef] = {0};
      encode_position(t, az, el, gain, [&](int c, double v) { got[c] = v, seen[c]++; });
      for (int c = 0; c < n_coef; c++) {
        const double want = encode_one(t.ch[c], az, el, gain);
        checked++;
        if (seen[c] != 1 || std::memcmp(&got[c], &want, sizeof want) != 0) {
          if (failed++ < 10)
            std::printf("FAILED trial %d: channel %d (%d, %d) at az %g el %g: seen %d, %.17g != %.17g\n", trial, c, orders[c],
                        degrees[c], az, el, seen[c], got[c], want);
        }
      }
    }
  }
  std::printf("%ld checked, %ld failed\n", checked, failed);
  return failed ? 1 : 0;
}
