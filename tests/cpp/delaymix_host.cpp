// delaymix_host.cpp — libear_amd/csrc/delaymix.h compiled for the host alone (g++, no HIP, under ASan and UBSan): the checks, the
// tables, the history rule and the host form of the delay matrix (the header's chain with std::fmaf).  Every call gets input and
// output rows of exactly its own length, each an allocation of its own, and a row no route reads gets a NULL pointer: a read or
// a write beside a row, or a look at an unread row, is an error of the sanitizer.
// tests/delaymix_model.py writes the input file and reads the output file:
//   in:  int32 n_in, n_out, R, ncalls; uint64 n; R x (int32 in, out, delay, n_taps; float32 taps[32]); uint64 calls[ncalls];
//        float32 x[n_in][n]
//   out: float32 y[n_out][n]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../libear_amd/csrc/delaymix.h"

namespace {
template <typename T>
bool get(std::FILE *f, T *p, size_t count) {
  return count == 0 || std::fread(p, sizeof(T), count, f) == count;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  uint64_t n;
  if (!get(f, hdr, 4) || !get(f, &n, 1)) return 2;
  const int n_in = hdr[0], n_out = hdr[1], R = hdr[2], ncalls = hdr[3];
  if (const char *why = earhip::delaymix_check_shape(n_in, n_out, R, 1)) {
    std::printf("refused: %s\n", why);
    return 3;
  }
  static_assert(sizeof(earhip::DelaymixRoute) == 4 * sizeof(int32_t) + 32 * sizeof(float), "the file's route record");
  std::vector<earhip::DelaymixRoute> routes((size_t)R);
  if (!get(f, routes.data(), routes.size())) return 2;
  if (const char *why = earhip::delaymix_check_routes(n_in, n_out, R, routes.data())) {
    std::printf("refused: %s\n", why);
    return 3;
  }
  std::vector<uint64_t> calls((size_t)ncalls);
  std::vector<float> x((size_t)n_in * n), y((size_t)n_out * n);
  if (!get(f, calls.data(), calls.size()) || !get(f, x.data(), x.size())) return 2;
  std::fclose(f);
  earhip::DelaymixRef dm(n_in, n_out, R, routes.data());
  size_t at = 0;
  for (uint64_t len : calls) {
    if (at + len > n) return 2;
    std::vector<std::vector<float>> in((size_t)n_in), out((size_t)n_out, std::vector<float>((size_t)len));
    std::vector<const float *> ip((size_t)n_in, nullptr);
    std::vector<float *> op((size_t)n_out);
    for (int c = 0; c < n_in; c++) {
      if (!(dm.tables().reads >> c & 1)) continue;
      in[(size_t)c].assign(x.begin() + (size_t)c * n + at, x.begin() + (size_t)c * n + at + (size_t)len);
      ip[(size_t)c] = in[(size_t)c].data();
    }
    for (int k = 0; k < n_out; k++) op[(size_t)k] = out[(size_t)k].data();
    dm.process((size_t)len, ip.data(), op.data());
    for (int k = 0; k < n_out; k++) std::copy(out[(size_t)k].begin(), out[(size_t)k].end(), y.begin() + (size_t)k * n + at);
    at += (size_t)len;
  }
  if (at != n || dm.clock() != n) return 2;
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  const bool ok = y.empty() || std::fwrite(y.data(), sizeof(float), y.size(), f) == y.size();
  return std::fclose(f) == 0 && ok ? 0 : 2;
}
