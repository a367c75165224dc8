// loudness_host.cpp — libear_amd/csrc/loudness.h compiled for the host alone (g++, no HIP): the sequential K-weighting cascade
// and the chunked form the device kernels run (zero-state pass, propagation by powers of Phi, second pass), behind a C
// interface that tests/test_loudness_cpu.py and tests/loudness_model.py load with ctypes.
#include <cstddef>

#include "../../libear_amd/csrc/loudness.h"

extern "C" {

// y[n] of the cascade on x[n] from the zero state (built-in 48 kHz coefficients), float64
void loud_filter(const float *x, size_t n, double *y) {
  earhip::KCoeffs<double> k;
  for (int s = 0; s < 2; s++)
    for (int i = 0; i < 5; i++) k.c[s][i] = earhip::kLoudnessCoeffs48k[s][i];
  earhip::KState<double> st{{0, 0, 0, 0}};
  for (size_t i = 0; i < n; i++) y[i] = earhip::k_weight_step(k, st, (double)x[i]);
}

// one channel through the meter, fed in calls of the given lengths; chunked != 0: the decomposition.  Returns the number of
// finished steps, the first `cap` of which are written to steps_out.
size_t loud_run(int chunked, int step, int chunk, const float *x, const size_t *calls, size_t ncalls, double *steps_out,
                size_t cap) {
  earhip::LoudnessChannelRef m(earhip::kLoudnessCoeffs48k, step, chunk);
  size_t at = 0;
  for (size_t c = 0; c < ncalls; c++) {
    if (chunked) m.process_chunked(x + at, calls[c]);
    else m.process_sequential(x + at, calls[c]);
    at += calls[c];
  }
  for (size_t i = 0; i < m.steps.size() && i < cap; i++) steps_out[i] = m.steps[i];
  return m.steps.size();
}

int loud_chunk_length(int step, int most) { return earhip::loudness_chunk_length(step, most); }

}  // extern "C"
