// true_peak_host.cpp — libear_amd/csrc/true_peak.h and the loudness range of loudness.h compiled for the host alone (g++, no
// HIP): the float32 dot products (tp_dot_n<12> for a 4 x 12 table, tp_dot for any other: the functions the two device kernels
// call), the NaN-ignoring maximum they share and a carried history like theirs, behind a C
// interface that tests/true_peak_model.py loads with ctypes.
#include <cstddef>

#include "../../libear_amd/csrc/true_peak.h"

extern "C" {

void tp_default_table(double *out48) {
  double h[4][12];
  earhip::true_peak_default_table(h);
  for (int i = 0; i < 48; i++) out48[i] = h[i / 12][i % 12];
}

// one channel through the meter, fed in calls of the given lengths; table NULL = the default.  Returns the number of finished
// steps, the first `cap` of which are written to tp_steps / sp_steps; open[0], open[1] = the true and sample peak of the
// unfinished step.
size_t tp_run(int phases, int taps, const double *table, int step, const float *x, const size_t *calls, size_t ncalls,
              float *tp_steps, float *sp_steps, size_t cap, float *open) {
  double h[4][12];
  if (!table) {
    earhip::true_peak_default_table(h);
    table = &h[0][0], phases = 4, taps = 12;
  }
  earhip::TruePeakChannelRef m(phases, taps, table, step);
  size_t at = 0;
  for (size_t c = 0; c < ncalls; c++) {
    m.process(x + at, calls[c]);
    at += calls[c];
  }
  for (size_t i = 0; i < m.tp_steps.size() && i < cap; i++) tp_steps[i] = m.tp_steps[i], sp_steps[i] = m.sp_steps[i];
  open[0] = m.tp_open, open[1] = m.sp_open;
  return m.tp_steps.size();
}

}  // extern "C"
