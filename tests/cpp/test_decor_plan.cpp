// libear_amd/csrc/decor_plan.h on the CPU: the decisions of the renderer's decorrelator stage — partition size, partitions, run
// length, which kernel — and the wave kernel's run length, against tests/golden/decor_plan.txt (argv[1]), the values the
// renderer's own code gave before these decisions had a header.  Lines of the fixture:
//   W T N num_cus R                                                   wave_run_len(T, N, num_cus) with 4 runs to a workgroup
//   P B n_taps K2_OWN_BLOCK K2_WG RUN Bk Lk NP run_len run_len_set wave   two buses; RUN -1: the option is not set
#include <cstdio>

#include "decor_plan.h"

using namespace earhip;

int main(int argc, char **argv) {
  if (argc != 2) return printf("usage: test_decor_plan tests/golden/decor_plan.txt\n"), 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return printf("cannot open %s\n", argv[1]), 2;
  int bad = 0, nw = 0, np = 0;
  char line[256];
  while (fgets(line, sizeof line, f)) {
    int v[11];
    if (sscanf(line, "W %d %d %d %d", &v[0], &v[1], &v[2], &v[3]) == 4) {
      const int R = wave_run_len(v[0], v[1], v[2], 4);
      if (R != v[3]) printf("FAILED: wave_run_len(%d, %d, %d) = %d, was %d\n", v[0], v[1], v[2], R, v[3]), bad++;
      nw++;
    } else if (sscanf(line, "P %d %d %d %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9],
                      &v[10]) == 11) {
      const DecorPlan p = decor_plan(2, v[0], v[1], v[2] != 0, v[4] >= 0, v[4] >= 0 ? v[4] : 0);
      const int wave = decor_wave_kernel(p, v[3] != 0) ? 1 : 0;
      if (p.Bk != v[5] || p.Lk != v[6] || p.NP != v[7] || p.run_len != v[8] || (p.run_len_set ? 1 : 0) != v[9] || wave != v[10])
        printf("FAILED: %s   now %d %d %d %d %d %d\n", line, p.Bk, p.Lk, p.NP, p.run_len, p.run_len_set ? 1 : 0, wave), bad++;
      np++;
    } else {
      printf("FAILED: a line of the fixture that is neither: %s", line), bad++;
    }
  }
  fclose(f);
  // (12 call lengths x 4 loudspeaker counts x 3 chips; 9 block sizes x 5 FIR lengths x 2 x 2 x 3 options)
  if (nw != 144 || np != 540) printf("FAILED: %d + %d lines, the fixture has 144 + 540\n", nw, np), bad++;
  printf("%d run lengths, %d plans, %d failed\n", nw, np, bad);
  return bad ? 1 : 0;
}
