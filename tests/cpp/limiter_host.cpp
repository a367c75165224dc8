// limiter_host.cpp — libear_amd/csrc/limiter.h compiled for the host alone (g++, no HIP, under ASan and UBSan): the required
// gain, the order of the smoothing sum and the final min the device kernels call, the detector on true_peak.h's dot products,
// and histories carried like theirs.  tests/limiter_model.py writes the input file and reads the output file:
//   in:  int32 C, L, H, detect, phases, taps, ncalls; float32 c; uint64 n; float64 table[phases][taps] (none: the default);
//        uint64 calls[ncalls]; float32 x[C][n]
//   out: float32 out[C][n]; float32 g[n]; float32 min_gain; 4 bytes of padding; uint64 limited_samples
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../libear_amd/csrc/limiter.h"

namespace {
template <typename T>
bool get(std::FILE *f, T *p, size_t count) {
  return count == 0 || std::fread(p, sizeof(T), count, f) == count;
}
template <typename T>
bool put(std::FILE *f, const T *p, size_t count) {
  return count == 0 || std::fwrite(p, sizeof(T), count, f) == count;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[7];
  float c;
  uint64_t n;
  if (!get(f, hdr, 7) || !get(f, &c, 1) || !get(f, &n, 1)) return 2;
  const int C = hdr[0], L = hdr[1], H = hdr[2], detect = hdr[3], ncalls = hdr[6];
  int phases = hdr[4], taps = hdr[5];
  if (const char *why = earhip::limiter_check_config(C, 48000, c, L, H, detect, 1)) {
    std::printf("refused: %s\n", why);
    return 3;
  }
  std::vector<double> table((size_t)phases * (size_t)taps);
  std::vector<uint64_t> calls((size_t)ncalls);
  std::vector<float> x((size_t)C * n);
  if (!get(f, table.data(), table.size()) || !get(f, calls.data(), calls.size()) || !get(f, x.data(), x.size())) return 2;
  std::fclose(f);
  if (table.empty()) {
    double h[4][12];
    earhip::true_peak_default_table(h);
    phases = 4, taps = 12;
    table.assign(&h[0][0], &h[0][0] + 48);
  }
  earhip::LimiterRef lim(C, c, L, H, detect, phases, taps, table.data());
  std::vector<float> out((size_t)C * n + 1), g(n + 1);
  size_t at = 0;
  for (uint64_t len : calls) {
    if (at + len > n) return 2;
    lim.process((size_t)len, x.data() + at, (size_t)n, out.data() + at, (size_t)n, g.data() + at);
    at += (size_t)len;
  }
  if (at != n) return 2;
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  const uint32_t pad = 0;
  const uint64_t limited = lim.limited;
  const bool ok = put(f, out.data(), (size_t)C * n) && put(f, g.data(), (size_t)n) && put(f, &lim.min_gain, 1) && put(f, &pad, 1) &&
                  put(f, &limited, 1);
  return std::fclose(f) == 0 && ok ? 0 : 2;
}
