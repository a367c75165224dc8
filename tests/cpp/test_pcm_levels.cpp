// libear_amd/csrc/pcm_convert.h on the CPU: the host fold of the levels the PCM-out kernel keeps (pcm_levels_fold, what
// earhip_render_output_levels and earhip_limiter_output_levels return): per channel the largest bit pattern and the sum of the counts.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcm_convert.h"

using namespace earhip;

static unsigned bits_of(float f) {
  unsigned u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

int main() {
  const int slots = 64, C = 3;
  std::vector<unsigned> pk((size_t)slots * C, 0u);
  std::vector<unsigned long long> cl((size_t)slots * C, 0ull);
  // channel 0: peaks scattered over the slots, the largest (1.5) in the middle, one denormal; counts whose sum passes 2^32
  // channel 1: never touched
  // channel 2: the largest peak in the last slot (infinity: the largest pattern a non-NaN magnitude has), one count in the first
  for (int k = 0; k < slots; k++) pk[(size_t)k * C + 0] = bits_of(0.001f * (float)(k % 17));
  pk[(size_t)37 * C + 0] = bits_of(1.5f);
  pk[(size_t)5 * C + 0] = 1u;
  uint64_t want0 = 0;
  for (int k = 0; k < slots; k++) {
    cl[(size_t)k * C + 0] = k == 11 ? (5ull << 32) + 7ull : (unsigned long long)(k * 1000);
    want0 += cl[(size_t)k * C + 0];
  }
  pk[(size_t)0 * C + 2] = bits_of(0.75f);
  pk[(size_t)(slots - 1) * C + 2] = 0x7F800000u;
  cl[(size_t)0 * C + 2] = 1;

  float peak[C] = {-1.0f, -1.0f, -1.0f};
  uint64_t clipped[C] = {99, 99, 99};
  pcm_levels_fold(slots, C, pk.data(), cl.data(), peak, clipped);

  int bad = 0;
  if (bits_of(peak[0]) != bits_of(1.5f) || clipped[0] != want0 || want0 <= (1ull << 32)) bad++;
  if (bits_of(peak[1]) != 0u || clipped[1] != 0) bad++;  // (+0.0f exactly)
  if (bits_of(peak[2]) != 0x7F800000u || clipped[2] != 1) bad++;
  printf("peaks %a %a %a, clipped %" PRIu64 " %" PRIu64 " %" PRIu64 ": %d problem(s)\n", peak[0], peak[1], peak[2], clipped[0], clipped[1],
         clipped[2], bad);
  return bad ? 1 : 0;
}
