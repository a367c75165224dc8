// The float -> PCM conversion of libear_amd/csrc/pcm_convert.h — the function the device kernel k_rows_to_pcm runs — compiled for
// the host.  Reads records from stdin: "<fmt 1|2|3> <dither 0|1> <seed> <t> <n> <x bits, hex>" and prints "<q> <clipped> <h hex>"
// per record: tests/test_render_pcm_out_cpu.py compares them with the numpy model, bit for bit.
// Build: g++ -std=c++17 -O2 -ffp-contract=off -Ilibear_amd/csrc tests/cpp/test_pcm_convert.cpp -o test_pcm_convert
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "pcm_convert.h"

using namespace earhip;

int main() {
  int fmt, dither;
  unsigned seed, n, xb;
  long long t;
  while (std::scanf("%d %d %u %lld %u %x", &fmt, &dither, &seed, &t, &n, &xb) == 6) {
    float x;
    std::memcpy(&x, &xb, 4);
    const uint32_t h = pcm_dither_hash(seed, (uint64_t)t, n);
    const float d = pcm_dither_value(h);
    bool clipped = false;
    int32_t q = 0;
    if (fmt == kPcmS16 && dither) q = pcm_from_float<kPcmS16, true>(x, d, &clipped);
    else if (fmt == kPcmS16) q = pcm_from_float<kPcmS16, false>(x, 0.f, &clipped);
    else if (fmt == kPcmS24) q = pcm_from_float<kPcmS24, false>(x, 0.f, &clipped);
    else if (fmt == kPcmS32) q = pcm_from_float<kPcmS32, false>(x, 0.f, &clipped);
    else return 2;
    std::printf("%" PRId32 " %d %08" PRIx32 "\n", q, clipped ? 1 : 0, h);
  }
  return 0;
}
