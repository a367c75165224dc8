// Host unit test of ColumnPlan::make (libear_amd/csrc/curves.h): the column tiling at the widths where it makes more than one
// column group, against known answers typed in from the rule by hand (the table of tests/wide_bus_cases.py) — 48 columns, the widest
// BS.2051 case, is the last width of one group.  Built like test_plan_table.cpp (curves.h needs the HIP headers); no HIP call is
// made: runs without a GPU.
#include <cstdio>

#include "curves.h"

using namespace earhip;

struct Want {
  int ncols, nout, ngroups, nz, nct, mgroups, mnz, row;
};

static const Want kWant[] = {
    {48, 24, 2, 1, 3, 1, 1, 48},   {49, 24, 3, 1, 3, 2, 1, 96},   {50, 24, 3, 1, 3, 2, 1, 96},    {64, 24, 3, 1, 3, 2, 1, 96},
    {96, 24, 4, 1, 3, 2, 1, 96},   {98, 24, 5, 1, 3, 3, 1, 144},  {194, 24, 8, 2, 3, 5, 1, 384},  {386, 24, 8, 3, 3, 8, 2, 768},
};

int main() {
  int failures = 0;
  for (const Want &w : kWant) {
    const ColumnPlan p = ColumnPlan::make(w.ncols);
    const bool ok = p.nout == w.nout && p.ngroups == w.ngroups && p.nz == w.nz && p.nct == w.nct && p.mgroups == w.mgroups &&
                    p.mnz == w.mnz && p.row == w.row;
    printf("%d columns: nout %d ngroups %d nz %d nct %d mgroups %d mnz %d row %d%s\n", w.ncols, p.nout, p.ngroups, p.nz, p.nct, p.mgroups,
           p.mnz, p.row, ok ? "" : "  <-- not the known answer");
    failures += !ok;
    // what the kernels rely on: both tilings cover every column inside the padded row, whose float4 copies need a multiple of 4
    if (p.nz * p.ngroups * p.nout < w.ncols || p.mnz * p.mgroups * p.nct * 16 < w.ncols || p.nz * p.ngroups * p.nout > p.row ||
        p.mnz * p.mgroups * p.nct * 16 > p.row || p.row % 4 != 0) {
      printf("%d columns: a tiling does not cover the columns inside the row\n", w.ncols);
      failures++;
    }
  }
  return failures != 0;
}
