// loudness.h — the maths of the programme loudness meter (include/earhip.h, group L: ITU-R BS.1770-4) as plain C++ that the
// device kernels (loudness_kernels.h), the host functions of the C ABI (api_loudness.hip) and a plain C++ program on the CPU
// (tests/cpp/loudness_host.cpp) all compile: what is tested against the float64 model on the CPU is the code the kernels
// run.  No HIP header is needed to include it.
//
//   - the K-weighting cascade: two biquads in transposed direct form II, float64 arithmetic on float32 samples.  The cascade's
//     state is FOUR numbers (s1, s2 of each stage), and the state after a run of samples is LINEAR in the state before it:
//         S_end = Phi^len * S_start + e,      e = the end state of the same run started from the zero state.
//     That is what lets the time axis be cut into chunks that run in parallel: pass 1 runs every chunk from zero and keeps e,
//     the propagation carries the true state across the chunks with Phi^L, pass 2 reruns every chunk from its true state;
//   - the powers of Phi (made once, in long double, by running the cascade on the unit states with no input);
//   - the gating of BS.1770-4 over 100 ms step energies, and the channel weights of a BS.2051 layout.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EARHIP_LOUD_HD __host__ __device__
#else
#define EARHIP_LOUD_HD
#endif

namespace earhip {

// BS.1770-4's coefficients at 48 kHz: [stage][b0 b1 b2 a1 a2]
static const double kLoudnessCoeffs48k[2][5] = {
    {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585},
    {1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621},
};

template <typename T>
struct KCoeffs {
  T c[2][5];  // [stage][b0 b1 b2 a1 a2]
};
template <typename T>
struct KState {
  T s[4];  // s1, s2 of stage 1; s1, s2 of stage 2
};

// One sample through the cascade.  y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2] per stage, in the
// transposed form: y = b0 x + s1; s1 = b1 x - a1 y + s2; s2 = b2 x - a2 y.
template <typename T>
EARHIP_LOUD_HD inline T k_weight_step(const KCoeffs<T> &k, KState<T> &st, T x) {
  using std::fma;  // (every multiply-add is ONE rounding, on the host as on the device: 12 operations a sample instead of 20)
  const T y1 = fma(k.c[0][0], x, st.s[0]);
  st.s[0] = fma(-k.c[0][3], y1, fma(k.c[0][1], x, st.s[1]));
  st.s[1] = fma(-k.c[0][4], y1, k.c[0][2] * x);
  const T y2 = fma(k.c[1][0], y1, st.s[2]);
  st.s[2] = fma(-k.c[1][3], y2, fma(k.c[1][1], y1, st.s[3]));
  st.s[3] = fma(-k.c[1][4], y2, k.c[1][2] * y1);
  return y2;
}

// A run of samples: advances st, returns the sum of y^2 (added in sample order to `acc`).
EARHIP_LOUD_HD inline double k_weight_run(const KCoeffs<double> &k, KState<double> &st, const float *x, size_t n, double acc) {
  for (size_t i = 0; i < n; i++) {
    const double y = k_weight_step(k, st, (double)x[i]);
    acc = std::fma(y, y, acc);
  }
  return acc;
}

// S' = M * S + e for a row-major 4x4 M
EARHIP_LOUD_HD inline KState<double> k_state_advance(const double *M, const KState<double> &S, const KState<double> &e) {
  KState<double> r;
  for (int i = 0; i < 4; i++) {
    double v = e.s[i];
    for (int j = 0; j < 4; j++) v = std::fma(M[4 * i + j], S.s[j], v);
    r.s[i] = v;
  }
  return r;
}

// Phi^j for j = 0 .. count - 1, row-major 4x4 each: column q of Phi^j is the state j samples after the unit state q with no
// input.  Made in long double and rounded once.
inline void k_state_powers(const double coeffs[2][5], size_t count, size_t stride_samples, double *out) {
  // out[i] = Phi^(i * stride_samples)
  KCoeffs<long double> k;
  for (int s = 0; s < 2; s++)
    for (int i = 0; i < 5; i++) k.c[s][i] = (long double)coeffs[s][i];
  KState<long double> col[4];
  for (int q = 0; q < 4; q++)
    for (int i = 0; i < 4; i++) col[q].s[i] = i == q ? 1.0L : 0.0L;
  for (size_t j = 0; j < count; j++) {
    for (int q = 0; q < 4; q++)
      for (int i = 0; i < 4; i++) out[16 * j + 4 * i + q] = (double)col[q].s[i];
    if (j + 1 < count)
      for (size_t t = 0; t < stride_samples; t++)
        for (int q = 0; q < 4; q++) (void)k_weight_step(k, col[q], 0.0L);
  }
}

// The chunk length of the decomposition: the largest divisor of the 100 ms step that is at most `most` samples.
inline int loudness_chunk_length(int step, int most) {
  int best = 1;
  for (int d = 1; d <= most && d <= step; d++)
    if (step % d == 0) best = d;
  return best;
}

// The meter on the CPU, in the two forms the tests compare.  One channel each; both carry their state from call to call.
// `open` is the sum of y^2 of the unfinished step; finished steps are appended to `steps` as MEAN squares.
struct LoudnessChannelRef {
  KCoeffs<double> k;
  KState<double> st{{0, 0, 0, 0}};
  double open = 0.0;
  size_t clock = 0;
  int step = 4800, L = 240;
  std::vector<double> powers;  // Phi^0 .. Phi^L
  std::vector<double> steps;

  LoudnessChannelRef(const double coeffs[2][5], int step_samples, int chunk) : step(step_samples), L(chunk) {
    for (int s = 0; s < 2; s++)
      for (int i = 0; i < 5; i++) k.c[s][i] = coeffs[s][i];
    powers.resize(16 * (size_t)(L + 1));
    k_state_powers(coeffs, (size_t)L + 1, 1, powers.data());
  }

  // sample by sample
  void process_sequential(const float *x, size_t n) {
    for (size_t i = 0; i < n; i++) {
      open = k_weight_run(k, st, x + i, 1, open);
      if (++clock % (size_t)step == 0) {
        steps.push_back(open / (double)step);
        open = 0.0;
      }
    }
  }

  // the decomposition the kernels run: chunks on the meter's own clock grid (so that a chunk lies inside one step); pass 1 from
  // the zero state, propagation, pass 2 from the true states, then the chunks of a step summed in ascending order
  void process_chunked(const float *x, size_t n) {
    if (n == 0) return;
    const size_t t0 = clock, k0 = t0 / (size_t)L, k1 = (t0 + n - 1) / (size_t)L, nch = k1 - k0 + 1;
    std::vector<KState<double>> e(nch), start(nch + 1);
    std::vector<size_t> lo(nch), len(nch);
    for (size_t c = 0; c < nch; c++) {
      const size_t a = (k0 + c) * (size_t)L, b = a + (size_t)L;
      lo[c] = a > t0 ? a - t0 : 0;
      len[c] = (b < t0 + n ? b - t0 : n) - lo[c];
      KState<double> z{{0, 0, 0, 0}};
      (void)k_weight_run(k, z, x + lo[c], len[c], 0.0);
      e[c] = z;
    }
    start[0] = st;
    for (size_t c = 0; c < nch; c++) start[c + 1] = k_state_advance(&powers[16 * len[c]], start[c], e[c]);
    double acc = open;
    for (size_t c = 0; c < nch; c++) {
      KState<double> s = start[c];
      acc += k_weight_run(k, s, x + lo[c], len[c], 0.0);
      if ((t0 + lo[c] + len[c]) % (size_t)step == 0) {
        steps.push_back(acc / (double)step);
        acc = 0.0;
      }
    }
    open = acc;
    st = start[nch];
    clock += n;
  }
};

// ---- gating (BS.1770-4 section 5.1 over 100 ms steps) ------------------------------------------------------------------------
// energy [n_steps][n_channels] mean squares, weights [n_channels].  Windows of `w` consecutive steps, hop one step.
inline double loudness_window_power(const double *energy, int n_channels, const double *weights, size_t first, int w) {
  double p = 0.0;
  for (int c = 0; c < n_channels; c++) {
    double z = 0.0;
    for (int i = 0; i < w; i++) z += energy[(first + (size_t)i) * (size_t)n_channels + c];
    p += weights[c] * (z / (double)w);
  }
  return p;
}
inline double loudness_of_power(double p) {
  return p > 0.0 ? -0.691 + 10.0 * std::log10(p) : -std::numeric_limits<double>::infinity();
}
inline void loudness_gate(size_t n_steps, int n_channels, const double *energy, const double *weights, double *integrated,
                          double *max_momentary, double *max_short_term) {
  const double ninf = -std::numeric_limits<double>::infinity();
  double L = ninf, mom = ninf, st = ninf;
  if (n_steps >= 4) {
    const size_t nb = n_steps - 3;
    std::vector<double> P(nb), l(nb);
    for (size_t j = 0; j < nb; j++) {
      P[j] = loudness_window_power(energy, n_channels, weights, j, 4);
      l[j] = loudness_of_power(P[j]);
      if (l[j] > mom) mom = l[j];
    }
    double sum = 0.0;
    size_t cnt = 0;
    for (size_t j = 0; j < nb; j++)
      if (l[j] > -70.0) sum += P[j], cnt++;
    if (cnt) {
      const double gamma_r = loudness_of_power(sum / (double)cnt) - 10.0;
      sum = 0.0, cnt = 0;
      for (size_t j = 0; j < nb; j++)
        if (l[j] > -70.0 && l[j] > gamma_r) sum += P[j], cnt++;
      if (cnt) L = loudness_of_power(sum / (double)cnt);
    }
  }
  if (n_steps >= 30)
    for (size_t j = 0; j + 30 <= n_steps; j++) {
      const double v = loudness_of_power(loudness_window_power(energy, n_channels, weights, j, 30));
      if (v > st) st = v;
    }
  if (integrated) *integrated = L;
  if (max_momentary) *max_momentary = mom;
  if (max_short_term) *max_short_term = st;
}

// ---- loudness range (EBU Tech 3342) over the same step energies --------------------------------------------------------------
// Short-term windows (30 steps, hop one), gated at -70 LKFS and at 20 LU below the level of the mean power of what passed that;
// the survivors sorted, LRA = the 95th less the 10th percentile, each the element at floor((n - 1) p + 0.5).
inline void loudness_range(size_t n_steps, int n_channels, const double *energy, const double *weights, double *lra, double *low,
                           double *high) {
  const double ninf = -std::numeric_limits<double>::infinity();
  double r = 0.0, lo = ninf, hi = ninf;
  if (n_steps >= 30) {
    const size_t nw = n_steps - 29;
    std::vector<double> P(nw), l(nw);
    double sum = 0.0;
    size_t cnt = 0;
    for (size_t j = 0; j < nw; j++) {
      P[j] = loudness_window_power(energy, n_channels, weights, j, 30);
      l[j] = loudness_of_power(P[j]);
      if (l[j] > -70.0) sum += P[j], cnt++;
    }
    if (cnt) {
      const double gamma = loudness_of_power(sum / (double)cnt) - 20.0;
      std::vector<double> s;
      for (size_t j = 0; j < nw; j++)
        if (l[j] > -70.0 && l[j] > gamma) s.push_back(l[j]);
      if (!s.empty()) {
        std::sort(s.begin(), s.end());
        const double n1 = (double)(s.size() - 1);
        lo = s[(size_t)std::floor(n1 * 0.10 + 0.5)];
        hi = s[(size_t)std::floor(n1 * 0.95 + 0.5)];
        r = hi - lo;
      }
    }
  }
  if (lra) *lra = r;
  if (low) *low = lo;
  if (high) *high = hi;
}

// the weight G of a channel at a nominal position (BS.1770-4 table 4): 0 for an LFE channel, 1.41 where |elevation| < 30 and
// 60 <= |azimuth| <= 120, else 1
inline double loudness_channel_weight(double azimuth, double elevation, bool is_lfe) {
  if (is_lfe) return 0.0;
  const double az = std::fabs(azimuth), el = std::fabs(elevation);
  return (el < 30.0 && az >= 60.0 && az <= 120.0) ? 1.41 : 1.0;
}

}  // namespace earhip
