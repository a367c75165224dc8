// src_host.cpp — libear_amd/csrc/src.h compiled for the host alone (g++, no HIP, under ASan and UBSan): the index arithmetic, the
// history rule, the table and the host form of the converter (the header's chain with std::fmaf).  Every call gets input and
// output buffers of exactly its own lengths, so a read or a write beside them is an error of the sanitizer.
// tests/src_model.py writes the input file and reads the output file:
//   in:  int32 C, L, M, T, ncalls, 0; uint64 n; float64 h[L T]; uint64 calls[ncalls]; float32 x[C][n]
//   out: uint64 total; uint64 count[ncalls] (the outputs of every call); float32 y[C][total]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../libear_amd/csrc/src.h"

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
  int32_t hdr[6];
  uint64_t n;
  if (!get(f, hdr, 6) || !get(f, &n, 1)) return 2;
  const int C = hdr[0], L = hdr[1], M = hdr[2], T = hdr[3], ncalls = hdr[4];
  if (const char *why = earhip::src_check_shape(C, L, M, T, 1)) {
    std::printf("refused: %s\n", why);
    return 3;
  }
  std::vector<double> h((size_t)L * T);
  if (!get(f, h.data(), h.size())) return 2;
  if (const char *why = earhip::src_check_taps(h.data(), h.size())) {
    std::printf("refused: %s\n", why);
    return 3;
  }
  std::vector<uint64_t> calls((size_t)ncalls), counts;
  std::vector<float> x((size_t)C * n);
  if (!get(f, calls.data(), calls.size()) || !get(f, x.data(), x.size())) return 2;
  std::fclose(f);
  earhip::SrcRef src(C, L, M, T, h.data());
  std::vector<std::vector<float>> y((size_t)C);
  size_t at = 0;
  for (uint64_t len : calls) {
    if (at + len > n) return 2;
    std::vector<float> in((size_t)C * len);
    for (int c = 0; c < C; c++)
      for (size_t i = 0; i < len; i++) in[(size_t)c * len + i] = x[(size_t)c * n + at + i];
    const size_t expect = src.next_out((size_t)len);
    std::vector<float> out((size_t)C * expect);
    const size_t got = src.process((size_t)len, in.data(), (size_t)len, out.data(), expect);
    if (got != expect) return 4;
    for (int c = 0; c < C; c++) y[(size_t)c].insert(y[(size_t)c].end(), out.begin() + (size_t)c * got, out.begin() + (size_t)(c + 1) * got);
    counts.push_back(got);
    at += (size_t)len;
  }
  if (at != n || src.clock() != n) return 2;
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  const uint64_t total = y[0].size();
  bool ok = put(f, &total, 1) && put(f, counts.data(), counts.size());
  for (int c = 0; c < C; c++) ok = ok && put(f, y[(size_t)c].data(), y[(size_t)c].size());
  return std::fclose(f) == 0 && ok ? 0 : 2;
}
