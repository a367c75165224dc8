// iir_host.cpp — libear_amd/csrc/iir.h compiled for the host alone (g++, no HIP, under ASan and UBSan): the cascade step, the
// matrix powers, the chunk plan and the two host forms of the bank (sample by sample, and chunked in the kernels' order of
// operations).  tests/iir_model.py writes the input file and reads the output file:
//   in:  int32 n_in, n_out, R, mode (0 sequential | 1 chunked), ncalls, 0; uint64 n;
//        R x { int32 in, out, S, 0; float64 gain; float64 c[8][5] }; uint64 calls[ncalls]; float32 x[n_in][n]
//   out: float32 out[n_out][n]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../libear_amd/csrc/iir.h"

namespace {
template <typename T>
bool get(std::FILE *f, T *p, size_t count) {
  return count == 0 || std::fread(p, sizeof(T), count, f) == count;
}
template <typename T>
bool put(std::FILE *f, const T *p, size_t count) {
  return count == 0 || std::fwrite(p, sizeof(T), count, f) == count;
}
struct RouteRecord {
  int32_t in, out, S, pad;
  double gain;
  double c[earhip::kIirMaxSections][5];
};
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[6];
  uint64_t n;
  if (!get(f, hdr, 6) || !get(f, &n, 1)) return 2;
  const int n_in = hdr[0], n_out = hdr[1], R = hdr[2], mode = hdr[3], ncalls = hdr[4];
  if (const char *why = earhip::iir_check_shape(n_in, n_out, R, 1)) {
    std::printf("refused: %s\n", why);
    return 3;
  }
  std::vector<RouteRecord> rec((size_t)R);
  if (!get(f, rec.data(), rec.size())) return 2;
  std::vector<earhip::IirRoute> routes((size_t)R);
  for (int r = 0; r < R; r++) {
    earhip::IirRoute &d = routes[(size_t)r];
    d.in = rec[(size_t)r].in, d.out = rec[(size_t)r].out, d.S = rec[(size_t)r].S, d.gain = rec[(size_t)r].gain;
    for (int s = 0; s < earhip::kIirMaxSections; s++)
      for (int i = 0; i < 5; i++) d.c[s][i] = rec[(size_t)r].c[s][i];
    if (const char *why = earhip::iir_check_route(d, n_in, n_out)) {
      std::printf("refused: %s\n", why);
      return 3;
    }
  }
  std::vector<uint64_t> calls((size_t)ncalls);
  std::vector<float> x((size_t)n_in * n + 1);
  if (!get(f, calls.data(), calls.size()) || !get(f, x.data(), (size_t)n_in * n)) return 2;
  std::fclose(f);
  earhip::IirBankRef bank(n_in, n_out, routes);
  std::vector<float> out((size_t)n_out * n + 1);
  size_t at = 0;
  for (uint64_t len : calls) {
    if (at + len > n) return 2;
    if (mode)
      bank.process_chunked((size_t)len, x.data() + at, (size_t)n, out.data() + at, (size_t)n);
    else
      bank.process_sequential((size_t)len, x.data() + at, (size_t)n, out.data() + at, (size_t)n);
    at += (size_t)len;
  }
  if (at != n) return 2;
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  const bool ok = put(f, out.data(), (size_t)n_out * n);
  return std::fclose(f) == 0 && ok ? 0 : 2;
}
