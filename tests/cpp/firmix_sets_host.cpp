// firmix_sets_host.cpp — the filter-set part of libear_amd/csrc/firmix.h compiled for the host alone (g++ under ASan + UBSan, no
// HIP): the per-set pair lists at full width, the walk over the merged lists of two sets that the fade kernel takes, and the
// fade schedule — which blocks of a feed are fade blocks, q of each, the ramp, the refusal rules of select and load_set.
// tests/test_firmix_sets_cpu.py builds and runs it.
#include <cstdio>
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

static void check_lists(int C, int K, int J, const std::vector<float> *taps) {
  const FirmixSetLists s = firmix_make_set_lists(C, K, J, taps ? taps->data() : nullptr);
  const int groups = (K + 1) / 2;
  CHECK((int)s.group_start.size() == groups + 1 && s.group_start[0] == 0 && s.group_start.back() == (int)s.entries.size());
  CHECK(s.entries.size() <= firmix_set_entries_room(C, K));
  int pairs = 0;
  for (int g = 0; g < groups; g++) {
    int e = s.group_start[g];
    for (int c = 0; c < C; c++) {
      bool z[2];
      for (int o = 0; o < 2; o++) {
        const int k = 2 * g + o;
        z[o] = false;
        if (k >= K) continue;
        if (!taps) z[o] = true;
        else
          for (int j = 0; j < J; j++) z[o] = z[o] || (*taps)[((size_t)k * C + c) * J + j] != 0.0f;
        pairs += z[o];
      }
      if (!z[0] && !z[1]) continue;
      CHECK(e < s.group_start[g + 1]);
      if (e >= s.group_start[g + 1]) continue;
      const FirmixEntry &en = s.entries[(size_t)e++];
      CHECK(en.row == c);  // every channel has a ring row: row = channel
      CHECK(en.h0 == (z[0] ? (2 * g) * C + c : -1));
      CHECK(en.h1 == (z[1] ? (2 * g + 1) * C + c : -1));
      CHECK(en.h0 < K * C && en.h1 < K * C);
    }
    CHECK(e == s.group_start[g + 1]);
  }
  CHECK(s.n_pairs == pairs);
}

static void set_lists() {
  {
    std::vector<float> dense(3 * 5 * 7, 1.0f);
    check_lists(5, 3, 7, &dense);
    check_lists(5, 3, 7, nullptr);  // device taps: nothing dropped
    CHECK(firmix_make_set_lists(5, 3, 7, nullptr).n_pairs == 15);
    CHECK(firmix_make_set_lists(5, 3, 7, nullptr).entries.size() == firmix_set_entries_room(5, 3));
  }
  {  // diagonal, the only non-zero tap the last one; -0.0 is zero
    const int D = 4, J = 9;
    std::vector<float> taps((size_t)D * D * J, 0.0f);
    for (int k = 0; k < D; k++) taps[((size_t)k * D + k) * J + J - 1] = 0.5f;
    taps[((size_t)1 * D + 2) * J + 3] = -0.0f;
    check_lists(D, D, J, &taps);
    CHECK(firmix_make_set_lists(D, D, J, taps.data()).n_pairs == D);
    // anti-diagonal without the last output's pair
    std::vector<float> anti((size_t)D * D * J, 0.0f);
    for (int k = 0; k + 1 < D; k++) anti[((size_t)k * D + (D - 1 - k)) * J] = 1.0f;
    check_lists(D, D, J, &anti);
  }
  {
    std::vector<float> zero(2 * 3 * 4, 0.0f);
    check_lists(3, 2, 4, &zero);
    CHECK(firmix_make_set_lists(3, 2, 4, zero.data()).entries.empty());
  }
}

// the merged walk visits the union of both lists' channels once each, ascending, with each list's spectra where it has them
static void merged(const std::vector<FirmixEntry> &a, const std::vector<FirmixEntry> &b) {
  int ia = 0, ib = 0, last = -1, steps = 0;
  std::vector<int> seen_a, seen_b;
  while (ia < (int)a.size() || ib < (int)b.size()) {
    const FirmixMerged m = firmix_merge_step(a.data(), ia, (int)a.size(), b.data(), ib, (int)b.size());
    CHECK(m.row > last);
    last = m.row;
    steps++;
    bool in_a = false, in_b = false;
    for (const FirmixEntry &e : a)
      if (e.row == m.row) {
        in_a = true;
        CHECK(m.a0 == e.h0 && m.a1 == e.h1);
      }
    for (const FirmixEntry &e : b)
      if (e.row == m.row) {
        in_b = true;
        CHECK(m.b0 == e.h0 && m.b1 == e.h1);
      }
    CHECK(in_a || in_b);
    if (!in_a) CHECK(m.a0 == -1 && m.a1 == -1);
    if (!in_b) CHECK(m.b0 == -1 && m.b1 == -1);
    if (steps > 1000) break;
  }
  CHECK(ia == (int)a.size() && ib == (int)b.size());
  size_t both = 0;
  for (const FirmixEntry &e : a)
    for (const FirmixEntry &f : b) both += e.row == f.row;
  CHECK((size_t)steps == a.size() + b.size() - both);
}

static void merges() {
  const std::vector<FirmixEntry> none, a = {{0, 0, 4}, {2, 2, -1}, {3, -1, 7}}, b = {{1, 1, 5}, {2, -1, 6}}, c = {{5, 5, 9}};
  merged(none, none);
  merged(a, none);
  merged(none, a);
  merged(a, a);
  merged(a, b);
  merged(b, a);
  merged(a, c);
  merged(c, b);
}

static bool same(const FirmixFade &f, int current, int from, int done, int total) {
  return f.current == current && f.from == from && f.done == done && f.total == total;
}

static void schedule() {
  const int n_sets = 3;
  const char loaded[3] = {1, 1, 0};
  FirmixFade f;
  CHECK(same(f, 0, -1, 0, 0));
  // refusals change nothing (the check is separate from the change)
  CHECK(firmix_select_check(f, n_sets, loaded, 2, 1) != nullptr);   // unloaded
  CHECK(firmix_select_check(f, n_sets, loaded, 3, 1) != nullptr);   // out of range
  CHECK(firmix_select_check(f, n_sets, loaded, -1, 1) != nullptr);
  CHECK(firmix_select_check(f, n_sets, loaded, 1, 65) != nullptr);  // F out of range
  CHECK(firmix_select_check(f, n_sets, loaded, 1, -1) != nullptr);
  CHECK(firmix_select_check(f, n_sets, loaded, 1, 0) == nullptr && firmix_select_check(f, n_sets, loaded, 1, 64) == nullptr);
  // selecting the current set while no fade runs is a no-op
  CHECK(firmix_select_check(f, n_sets, loaded, 0, 5) == nullptr);
  firmix_select_apply(f, 0, 5);
  CHECK(same(f, 0, -1, 0, 0));
  CHECK(firmix_fade_blocks(f.from, f.done, f.total, 7) == 0);
  // a fade of 3 blocks over feeds of 2 and 4: blocks q = 0, 1 of the first feed, q = 2 of the second, then steady
  firmix_select_apply(f, 1, 3);
  CHECK(same(f, 1, 0, 0, 3));
  CHECK(firmix_set_in_use(f, 0) && firmix_set_in_use(f, 1) && !firmix_set_in_use(f, 2));
  CHECK(firmix_select_check(f, n_sets, loaded, 0, 2) == nullptr);  // not started yet: may be replaced
  int nf = firmix_fade_blocks(f.from, f.done, f.total, 2);
  CHECK(nf == 2 && f.done == 0);  // q0 of the feed
  firmix_fade_advance(f, nf);
  CHECK(same(f, 1, 0, 2, 3));
  CHECK(firmix_select_check(f, n_sets, loaded, 0, 2) != nullptr);  // started and not finished
  CHECK(firmix_select_check(f, n_sets, loaded, 1, 0) != nullptr);
  nf = firmix_fade_blocks(f.from, f.done, f.total, 4);
  CHECK(nf == 1 && f.done == 2);
  firmix_fade_advance(f, nf);
  CHECK(same(f, 1, -1, 0, 0));
  CHECK(!firmix_set_in_use(f, 0) && firmix_set_in_use(f, 1));
  CHECK(firmix_select_check(f, n_sets, loaded, 0, 2) == nullptr);
  // a select before any block of the previous one replaces it: from stays
  firmix_select_apply(f, 0, 4);
  CHECK(same(f, 0, 1, 0, 4));
  firmix_select_apply(f, 0, 2);
  CHECK(same(f, 0, 1, 0, 2));
  firmix_select_apply(f, 1, 2);  // back to where it came from: nothing to fade
  CHECK(same(f, 1, -1, 0, 0));
  firmix_select_apply(f, 0, 4);
  firmix_select_apply(f, 0, 0);  // replaced by a hard switch
  CHECK(same(f, 0, -1, 0, 0));
  // F = 0
  firmix_select_apply(f, 1, 0);
  CHECK(same(f, 1, -1, 0, 0) && firmix_fade_blocks(f.from, f.done, f.total, 3) == 0);
  // reset in mid-fade: the target is current
  firmix_select_apply(f, 0, 64);
  firmix_fade_advance(f, firmix_fade_blocks(f.from, f.done, f.total, 10));
  CHECK(same(f, 0, 1, 10, 64));
  firmix_fade_end(f);
  CHECK(same(f, 0, -1, 0, 0));
  // a fade that ends exactly with a feed, and feeds of one block
  firmix_select_apply(f, 1, 2);
  for (int q = 0; q < 2; q++) {
    CHECK(f.done == q && firmix_fade_blocks(f.from, f.done, f.total, 1) == 1);
    firmix_fade_advance(f, 1);
  }
  CHECK(same(f, 1, -1, 0, 0));
}

static void ramp() {
  for (int B : {64, 512, 4096})
    for (int F : {1, 2, 3, 64}) {
      CHECK(firmix_fade_gain(0, 0, F, B) == 0.0f);
      CHECK(firmix_fade_gain(F - 1, B - 1, F, B) < 1.0f);
      float last = -1.0f;
      for (int q = 0; q < F; q++)
        for (int n = 0; n < B; n += (B / 16)) {
          const float a = firmix_fade_gain(q, n, F, B);
          CHECK(a > last && a == (float)(q * B + n) / (float)(F * B));
          last = a;
        }
    }
}

int main() {
  set_lists();
  merges();
  schedule();
  ramp();
  std::printf("%d passed, %d failed\n", g_checks - g_failed, g_failed);
  return g_failed ? 1 : 0;
}
