// firmix_host.cpp — libear_amd/csrc/firmix.h compiled for the host alone (g++ under ASan + UBSan, no HIP): the plan of the FIR
// filter matrix that the device kernels and the C ABI use — partition counts, lists of non-zero pairs, ring slots over calls
// of any length, the configurations that are refused.  tests/test_firmix_cpu.py builds and runs it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../libear_amd/csrc/firmix.h"

using namespace earhip;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    g_checks++;                                                     \
    if (!(cond)) {                                                  \
      g_failed++;                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                               \
  } while (0)

static void partitions() {
  const int B = 64;
  CHECK(firmix_partitions(1, B) == 1);
  CHECK(firmix_partitions(B - 1, B) == 1);
  CHECK(firmix_partitions(B, B) == 1);
  CHECK(firmix_partitions(B + 1, B) == 2);
  CHECK(firmix_partitions(64 * B, B) == 64);
  CHECK(firmix_partitions(4097, 4096) == 2);
  CHECK(firmix_ring_slots(1, 1) == 1 && firmix_ring_slots(64, 1) == 64 && firmix_ring_slots(4, 1024) == 1027);
}

static void refused() {
  CHECK(firmix_check_config(24, 2, 512, 2048, 1024) == nullptr);
  CHECK(firmix_check_config(1, 1, 64, 1, 1) == nullptr);
  CHECK(firmix_check_config(64, 64, 4096, 64 * 4096, 1) == nullptr);
  CHECK(firmix_check_config(0, 2, 512, 8, 1) != nullptr);
  CHECK(firmix_check_config(65, 2, 512, 8, 1) != nullptr);
  CHECK(firmix_check_config(2, 0, 512, 8, 1) != nullptr);
  CHECK(firmix_check_config(2, 65, 512, 8, 1) != nullptr);
  CHECK(firmix_check_config(-1, -1, 512, 8, 1) != nullptr);
  for (int B : {0, -64, 1, 32, 63, 65, 96, 480, 960, 4095, 8192, 1 << 30}) CHECK(firmix_check_config(2, 2, B, 8, 1) != nullptr);
  for (int B : {64, 128, 256, 512, 1024, 2048, 4096}) {
    CHECK(firmix_check_config(2, 2, B, 8, 1) == nullptr);
    CHECK(firmix_check_config(2, 2, B, 64 * B, 1) == nullptr);
    CHECK(firmix_check_config(2, 2, B, 64 * B + 1, 1) != nullptr);
  }
  CHECK(firmix_check_config(2, 2, 512, 0, 1) != nullptr);
  CHECK(firmix_check_config(2, 2, 512, -5, 1) != nullptr);
  CHECK(firmix_check_config(2, 2, 4096, std::numeric_limits<int>::max(), 1) != nullptr);
  CHECK(firmix_check_config(2, 2, 512, 8, 0) != nullptr);
  CHECK(firmix_check_config(2, 2, 512, 8, -1) != nullptr);
  std::vector<float> taps(100, 0.25f);
  CHECK(firmix_taps_finite(taps.data(), taps.size()));
  taps[99] = std::numeric_limits<float>::infinity();
  CHECK(!firmix_taps_finite(taps.data(), taps.size()));
  taps[99] = 0.0f, taps[0] = std::nanf("");
  CHECK(!firmix_taps_finite(taps.data(), taps.size()));
}

static void check_plan_invariants(const FirmixPlan &p, const std::vector<float> &taps) {
  int pairs = 0;
  for (int k = 0; k < p.n_out; k++) {
    std::vector<int> want;
    for (int c = 0; c < p.n_in; c++) {
      bool any = false;
      for (int j = 0; j < p.n_taps; j++) any = any || taps[((size_t)k * p.n_in + c) * p.n_taps + j] != 0.0f;
      const int idx = p.pair_index[(size_t)k * p.n_in + c];
      CHECK(any == (idx >= 0));
      if (any) {
        CHECK(idx == pairs);
        pairs++;
        want.push_back(c);
      }
    }
    CHECK(p.pairs[(size_t)k] == want);
  }
  CHECK(p.n_pairs == pairs);
  CHECK((int)p.group_start.size() == p.groups() + 1 && p.group_start.back() == (int)p.entries.size());
  for (int g = 0; g < p.groups(); g++) {
    int last_row = -1;
    for (int e = p.group_start[g]; e < p.group_start[g + 1]; e++) {
      const FirmixEntry &en = p.entries[(size_t)e];
      CHECK(en.row > last_row && en.row < (int)p.used.size());  // ascending channels, each with a ring row
      last_row = en.row;
      const int c = p.used[(size_t)en.row];
      CHECK(en.h0 == p.pair_index[(size_t)(2 * g) * p.n_in + c]);
      CHECK(en.h1 == (2 * g + 1 < p.n_out ? p.pair_index[(size_t)(2 * g + 1) * p.n_in + c] : -1));
      CHECK(en.h0 >= 0 || en.h1 >= 0);
      CHECK(en.h0 < p.n_pairs && en.h1 < p.n_pairs);
    }
  }
  for (int c = 0; c < p.n_in; c++) {
    const int r = p.row_of[(size_t)c];
    CHECK(r < (int)p.used.size());
    if (r >= 0) CHECK(p.used[(size_t)r] == c);
  }
}

static void pair_lists() {
  {  // dense 3 x 5
    std::vector<float> taps(3 * 5 * 7, 1.0f);
    const FirmixPlan p = firmix_make_plan(5, 3, 64, 7, 4, taps.data());
    CHECK(p.n_pairs == 15 && p.used.size() == 5 && p.groups() == 2 && p.entries.size() == 10);
    CHECK(p.partitions == 1 && p.ring == 4);
    CHECK(p.spectra_elems() == 15u * 64u && p.ring_elems() == 5u * 4u * 64u && p.state_elems() == 2u * 5u * 64u);
    check_plan_invariants(p, taps);
  }
  {  // diagonal 24 x 24 and an extra input and output without a pair; the only non-zero tap may be the last, -0.0 is zero
    const int D = 24, J = 130;
    std::vector<float> taps((size_t)(D + 1) * (D + 1) * J, 0.0f);
    for (int k = 0; k < D; k++) taps[((size_t)k * (D + 1) + k) * J + (J - 1)] = 0.5f;
    taps[((size_t)3 * (D + 1) + 7) * J + 5] = -0.0f;
    const FirmixPlan p = firmix_make_plan(D + 1, D + 1, 64, J, 2, taps.data());
    CHECK(p.n_pairs == D && (int)p.used.size() == D && p.row_of[D] == -1 && p.pairs[D].empty());
    CHECK(p.partitions == 3 && p.ring == 4);
    CHECK((int)p.entries.size() == D);
    CHECK(p.group_start[p.groups()] - p.group_start[p.groups() - 1] == 0);  // the last group is output 24 alone: no entry
    check_plan_invariants(p, taps);
  }
  {  // all zero
    std::vector<float> taps(2 * 3 * 9, 0.0f);
    const FirmixPlan p = firmix_make_plan(3, 2, 64, 9, 1, taps.data());
    CHECK(p.n_pairs == 0 && p.used.empty() && p.entries.empty() && p.groups() == 1);
    CHECK(p.spectra_elems() == 0 && p.ring_elems() == 0);
    check_plan_invariants(p, taps);
  }
  {  // sparse: channel 1 only for output 2 (an odd output count: the last group has one output)
    std::vector<float> taps(3 * 2 * 4, 0.0f);
    taps[(2 * 2 + 1) * 4 + 2] = 1.0f;
    taps[(0 * 2 + 0) * 4 + 0] = 2.0f;
    const FirmixPlan p = firmix_make_plan(2, 3, 64, 4, 1, taps.data());
    CHECK(p.n_pairs == 2 && p.entries.size() == 2);
    CHECK(p.entries[0].row == 0 && p.entries[0].h0 == 0 && p.entries[0].h1 == -1);
    CHECK(p.entries[1].row == 1 && p.entries[1].h0 == 1 && p.entries[1].h1 == -1);
    check_plan_invariants(p, taps);
  }
}

// the ring over calls of any length: the slot of block t - p always still holds block t - p
static void ring(int P, int max_blocks, const std::vector<int> &calls) {
  const int R = firmix_ring_slots(P, max_blocks);
  std::vector<long long> holds((size_t)R, -1);
  unsigned long long clock = 0;
  for (int n : calls) {
    CHECK(n >= 1 && n <= max_blocks);
    const int slot0 = (int)(clock % (unsigned long long)R);
    // the spectra pass writes the call's slots ...
    for (int i = 0; i < n; i++) {
      const int s = firmix_ring_slot(slot0, i, 0, R);
      CHECK(s >= 0 && s < R);
      holds[(size_t)s] = (long long)clock + i;
    }
    // ... then the multiply pass reads, for every block, the live partitions
    for (int i = 0; i < n; i++) {
      const int live = firmix_live_partitions(P, i, clock);
      CHECK(live == (int)std::min<unsigned long long>((unsigned long long)P, clock + (unsigned long long)i + 1ull));
      for (int p = 0; p < live; p++) {
        const int s = firmix_ring_slot(slot0, i, p, R);
        CHECK(s >= 0 && s < R);
        CHECK(holds[(size_t)s] == (long long)clock + i - p);
      }
    }
    clock += (unsigned long long)n;
  }
}

int main() {
  partitions();
  refused();
  pair_lists();
  ring(1, 1, {1, 1, 1});
  ring(8, 1, std::vector<int>(40, 1));            // calls shorter than P - 1 blocks
  ring(8, 3, {1, 2, 1, 3, 1, 1, 2, 3, 3, 1, 2});  // the same, mixed
  ring(64, 70, {70, 1, 69, 2});
  ring(4, 1024, {1024, 1, 1023, 512});
  ring(2, 5, {5, 5, 1, 4, 3});
  std::printf("%d passed, %d failed\n", g_checks - g_failed, g_failed);
  return g_failed ? 1 : 0;
}
