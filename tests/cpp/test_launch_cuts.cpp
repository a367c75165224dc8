// libear_amd/csrc/launch_cuts.h on the CPU (ASan + UBSan): a call cut into launches, and the two halves of a carried state.
#include <cstdio>
#include <vector>

#include "launch_cuts.h"

using namespace earhip;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond);    \
      failures++;                                                        \
    }                                                                    \
  } while (0)

static void check_cuts(size_t n, size_t most) {
  std::vector<size_t> at, len, out_at;
  // (the output moves 2 per input and 1 per launch: a stage whose outputs are not its inputs, as the rate converter's)
  for_each_launch(n, most, [&](size_t a, size_t k, size_t o) {
    at.push_back(a), len.push_back(k), out_at.push_back(o);
    return 2 * k + 1;
  });
  size_t sum = 0, out = 0;
  for (size_t i = 0; i < len.size(); i++) {
    CHECK(at[i] == sum);      // in order, nothing left out
    CHECK(out_at[i] == out);  // the output where the launches before it left it
    CHECK(len[i] >= 1 && len[i] <= most);
    CHECK(i + 1 == len.size() || len[i] == most);  // all of `most` but the last
    sum += len[i], out += 2 * len[i] + 1;
  }
  CHECK(sum == n);
  CHECK(len.size() == (n + most - 1) / most);
  if (failures) std::printf("  (n = %zu, most = %zu)\n", n, most);
}

int main() {
  for (size_t most : {(size_t)1, (size_t)7, (size_t)1 << 24})
    for (size_t n : {(size_t)0, (size_t)1, most - 1, most, most + 1, 2 * most + 1}) check_cuts(n, most);

  // four flips of two halves of 5: read and written halves are different, in bounds, and swap at each flip
  Halves h{5, 0};
  std::vector<int> buf(2 * h.half, 0);
  for (int flip = 0; flip < 4; flip++) {
    CHECK(h.in() == (size_t)(flip & 1) * 5 && h.out() == (size_t)((flip & 1) ^ 1) * 5);
    for (size_t i = 0; i < h.half; i++) {
      CHECK(buf[h.in() + i] == flip);  // what the launch before wrote
      buf[h.out() + i] = flip + 1;
    }
    const size_t was_out = h.out();
    h.flip();
    CHECK(h.in() == was_out);
  }
  CHECK(h.par == 0);
  // (a state of no elements: both halves are the empty range at 0)
  Halves none;
  CHECK(none.in() == 0 && none.out() == 0);

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
