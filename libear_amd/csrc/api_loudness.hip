// api_loudness.hip — group L of include/earhip.h: programme loudness (ITU-R BS.1770-4), true peak (its annex 2) and loudness
// range (EBU Tech 3342) measured on the device.  The kernels: loudness_kernels.h, true_peak_kernels.h; the maths they share
// with the host functions and the CPU tests: loudness.h, true_peak.h.
#include <cstring>
#include <memory>

#include "common.h"
#include "layout_registry.h"
#include "loudness_kernels.h"
#include "true_peak_kernels.h"

using namespace earhip;

struct earhip_loudness {
  earhip_ctx *ctx = nullptr;
  int C = 0, rate = 0, step = 0, L = 0;
  size_t max_steps = 0;
  KCoeffs<double> k;
  unsigned long long clock = 0;  // samples since create / reset (the kernels get what they need of it as arguments)
  int par = 0;                   // which `open` word holds the sum of the unfinished step
  // everything a process call touches, made at create
  DevBuf<double> e, start, q, state, open, steps, P, Q;
  // host rows: pieces of kStage samples per channel through these
  static constexpr size_t kStage = 65536;
  PinBuf<float> p_stage;
  DevBuf<float> d_stage;
  // true peak (a meter made with a table): also made at create
  bool tp_on = false;
  int tp_phases = 0, tp_taps = 0;
  float tp_h[4][12];                // the table where its shape is 4 x 12
  DevBuf<float> tp_table, tp_hist;  // [phases][taps]; [2][C][kTpHist], read [par], written [par ^ 1]
  DevBuf<unsigned> tp_steps, sp_steps;  // [max_steps + 1][C]: the row behind the finished steps is the open step's
  DevBuf<unsigned> tp_totals;           // [2][C]: what earhip_loudness_peaks reduces the stores to
  PinBuf<float> p_totals;

  size_t max_launch() const { return (size_t)(kLoudMaxChunks - 1) * (size_t)L; }
  size_t num_steps() const { return (size_t)(clock / (unsigned long long)step); }

  void check_room(size_t nsamples) const {
    if ((clock + nsamples) / (unsigned long long)step > max_steps)
      fail_invalid("the call would pass the loudness meter's max_steps (nothing was consumed)");
  }

  void zero() {
    EARHIP_HIP(hipMemsetAsync(state.p, 0, sizeof(double) * state.n, ctx->stream));
    EARHIP_HIP(hipMemsetAsync(open.p, 0, sizeof(double) * open.n, ctx->stream));
    EARHIP_HIP(hipMemsetAsync(steps.p, 0, sizeof(double) * steps.n, ctx->stream));
    if (tp_on) {
      EARHIP_HIP(hipMemsetAsync(tp_hist.p, 0, sizeof(float) * tp_hist.n, ctx->stream));
      EARHIP_HIP(hipMemsetAsync(tp_steps.p, 0, sizeof(unsigned) * tp_steps.n, ctx->stream));
      EARHIP_HIP(hipMemsetAsync(sp_steps.p, 0, sizeof(unsigned) * sp_steps.n, ctx->stream));
    }
    clock = 0;
    par = 0;
  }

  // the true-peak pass over one launch's samples: it reads what the loudness passes read and shares nothing else with them
  void launch_true_peak(size_t n, const float *rows, size_t stride) {
    TpArgs t;
    t.rows = rows;
    t.stride = stride;
    t.n = (unsigned)n;
    t.C = C;
    t.r0 = (unsigned)(clock % (unsigned long long)step);
    t.step = (unsigned)step;
    t.step0 = clock / (unsigned long long)step;
    t.hist_in = tp_hist.p + (size_t)par * (size_t)C * kTpHist;
    t.hist_out = tp_hist.p + (size_t)(par ^ 1) * (size_t)C * kTpHist;
    t.tp = tp_steps.p, t.sp = sp_steps.p;
    t.phases = tp_phases, t.taps = tp_taps;
    t.table = tp_table.p;
    std::memcpy(t.h, tp_h, sizeof(tp_h));
    if (tp_phases == 4 && tp_taps == 12)
      hipLaunchKernelGGL(k_true_peak_4x12, dim3((unsigned)((n + kTpBlockTile - 1) / kTpBlockTile), (unsigned)C), dim3(64 * kTpWaves), 0,
                         ctx->stream, t);
    else
      hipLaunchKernelGGL(k_true_peak_any, dim3((unsigned)((n + kTpAnyTile - 1) / kTpAnyTile), (unsigned)C), dim3(kTpAnyTile), 0,
                         ctx->stream, t);
  }

  void launch(size_t n, const float *rows, size_t stride) {
    LoudArgs a;
    a.rows = rows;
    a.stride = stride;
    a.n = (unsigned)n;
    a.off0 = (unsigned)(clock % (unsigned long long)L);
    a.nchunks = (unsigned)((a.off0 + n + (size_t)L - 1) / (size_t)L);
    a.L = L;
    a.C = C;
    a.k = k;
    a.e = e.p, a.start = start.p, a.q = q.p, a.state = state.p, a.P = P.p, a.Q = Q.p;
    a.open = open.p;
    a.par = par;
    a.cps = (unsigned)(step / L);
    a.chunk0_in_step = (unsigned)((clock / (unsigned long long)L) % a.cps);
    a.step0 = clock / (unsigned long long)step;
    a.steps = steps.p;
    a.step_samples = (double)step;
    if (a.nchunks > (unsigned)kLoudMaxChunks) fail_internal("loudness launch beyond its scratch");
    if (tp_on) launch_true_peak(n, rows, stride);
    const unsigned touched = (a.chunk0_in_step + a.nchunks + a.cps - 1) / a.cps;
    const dim3 grid((a.nchunks + 63) / 64, (unsigned)C);
    hipLaunchKernelGGL(k_loudness_pass<false>, grid, dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_loudness_propagate, dim3((unsigned)C), dim3(kLoudPropThreads), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_loudness_pass<true>, grid, dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_loudness_steps, dim3((touched * (unsigned)C + 63) / 64), dim3(64), 0, ctx->stream, a, touched);
    EARHIP_HIP(hipGetLastError());
    clock += n;
    par ^= 1;
  }

  // device rows; the caller has checked the room
  void feed(size_t nsamples, const float *rows, size_t stride) {
    const size_t most = max_launch();
    for (size_t at = 0; at < nsamples;) {
      const size_t n = std::min(most, nsamples - at);
      launch(n, rows + at, stride);
      at += n;
    }
  }
};

namespace earhip {
void loudness_check_room(const earhip_loudness *m, size_t nsamples) { m->check_room(nsamples); }
void loudness_feed(earhip_loudness *m, size_t nsamples, const float *rows, size_t stride) { m->feed(nsamples, rows, stride); }
const earhip_ctx *loudness_ctx(const earhip_loudness *m) { return m->ctx; }
int loudness_channels(const earhip_loudness *m) { return m->C; }
}  // namespace earhip

extern "C" {

int earhip_loudness_create(earhip_ctx *ctx, int n_channels, int sample_rate, const double *coeffs, size_t max_steps,
                           earhip_loudness **out) {
  return earhip_loudness_create_tp(ctx, n_channels, sample_rate, coeffs, max_steps, nullptr, out);
}

int earhip_loudness_create_tp(earhip_ctx *ctx, int n_channels, int sample_rate, const double *coeffs, size_t max_steps,
                              const earhip_true_peak *tp, earhip_loudness **out) {
  return guarded([&] {
    require(ctx != nullptr && out != nullptr, "ctx and out must not be NULL");
    require(n_channels >= 1 && n_channels <= 65535, "n_channels must be in [1, 65535]");
    require(sample_rate >= 10 && sample_rate % 10 == 0, "sample_rate must be a positive multiple of 10");
    require(coeffs != nullptr || sample_rate == 48000,
            "the built-in K-weighting coefficients are those of 48000 Hz: another rate must bring its own");
    require(max_steps >= 1 && max_steps <= ((size_t)1 << 32) / (size_t)n_channels, "max_steps out of range");
    TpTable table;
    if (tp)
      if (const char *why = tp_table_make(tp, sample_rate, &table)) fail_invalid(why);
    ctx->use();
    std::unique_ptr<earhip_loudness> m(new earhip_loudness);
    m->ctx = ctx;
    m->C = n_channels;
    m->rate = sample_rate;
    m->step = sample_rate / 10;
    m->L = loudness_chunk_length(m->step, 240);
    m->max_steps = max_steps;
    double c[2][5];
    for (int s = 0; s < 2; s++)
      for (int i = 0; i < 5; i++) {
        c[s][i] = coeffs ? coeffs[5 * s + i] : kLoudnessCoeffs48k[s][i];
        require(std::isfinite(c[s][i]), "coefficients must be finite");
        m->k.c[s][i] = c[s][i];
      }
    const size_t C = (size_t)n_channels;
    m->e.alloc(C * kLoudMaxChunks * 4);
    m->start.alloc(C * kLoudMaxChunks * 4);
    m->q.alloc(C * kLoudMaxChunks);
    m->state.alloc(C * 4);
    m->open.alloc(2 * C);
    m->steps.alloc(max_steps * C);
    std::vector<double> P(16 * (size_t)(m->L + 1)), Q(16 * 65);
    k_state_powers(c, (size_t)m->L + 1, 1, P.data());
    k_state_powers(c, 65, (size_t)m->L, Q.data());
    m->P.alloc(P.size());
    m->Q.alloc(Q.size());
    EARHIP_HIP(hipMemcpy(m->P.p, P.data(), sizeof(double) * P.size(), hipMemcpyHostToDevice));
    EARHIP_HIP(hipMemcpy(m->Q.p, Q.data(), sizeof(double) * Q.size(), hipMemcpyHostToDevice));
    if (tp) {
      m->tp_on = true;
      m->tp_phases = table.phases, m->tp_taps = table.taps;
      std::memcpy(m->tp_h, table.h, sizeof(m->tp_h));
      m->tp_table.alloc(table.v.size());
      EARHIP_HIP(hipMemcpy(m->tp_table.p, table.v.data(), sizeof(float) * table.v.size(), hipMemcpyHostToDevice));
      m->tp_hist.alloc(2 * C * kTpHist);
      m->tp_steps.alloc((max_steps + 1) * C);
      m->sp_steps.alloc((max_steps + 1) * C);
      m->tp_totals.alloc(2 * C);
      m->p_totals.reserve(2 * C);
    }
    m->p_stage.reserve(C * earhip_loudness::kStage);
    m->d_stage.alloc(C * earhip_loudness::kStage);
    m->zero();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    *out = m.release();
  });
}

int earhip_loudness_destroy(earhip_loudness *m) {
  return guarded([&] {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    delete m;
  });
}

int earhip_loudness_reset(earhip_loudness *m) {
  return guarded([&] {
    require(m != nullptr, "meter must not be NULL");
    m->ctx->use();
    m->zero();
  });
}

int earhip_loudness_process_device(earhip_loudness *m, size_t nsamples, const float *rows_dev, size_t stride) {
  return guarded([&] {
    require(m != nullptr, "meter must not be NULL");
    if (nsamples == 0) return;
    require(rows_dev != nullptr, "rows_dev must not be NULL");
    require(stride >= nsamples, "stride too small");
    m->check_room(nsamples);
    m->ctx->use();
    m->feed(nsamples, rows_dev, stride);
  });
}

int earhip_loudness_process(earhip_loudness *m, size_t nsamples, const float *const *rows) {
  return guarded([&] {
    require(m != nullptr, "meter must not be NULL");
    if (nsamples == 0) return;
    require(rows != nullptr, "rows must not be NULL");
    for (int c = 0; c < m->C; c++) require(rows[c] != nullptr, "a row pointer is NULL");
    m->check_room(nsamples);
    earhip_ctx *ctx = m->ctx;
    ctx->use();
    const size_t cap = earhip_loudness::kStage;
    for (size_t at = 0; at < nsamples;) {
      const size_t n = std::min(cap, nsamples - at);
      for (int c = 0; c < m->C; c++) std::memcpy(m->p_stage.p + (size_t)c * n, rows[c] + at, sizeof(float) * n);
      EARHIP_HIP(hipMemcpyAsync(m->d_stage.p, m->p_stage.p, sizeof(float) * n * m->C, hipMemcpyHostToDevice, ctx->stream));
      m->feed(n, m->d_stage.p, n);
      EARHIP_HIP(hipStreamSynchronize(ctx->stream));  // (the one staging buffer is free again)
      at += n;
    }
  });
}

int earhip_loudness_num_steps(earhip_loudness *m, size_t *steps) {
  return guarded([&] {
    require(m != nullptr && steps != nullptr, "meter and steps must not be NULL");
    m->ctx->use();
    EARHIP_HIP(hipStreamSynchronize(m->ctx->stream));
    *steps = m->num_steps();
  });
}

int earhip_loudness_steps(earhip_loudness *m, size_t first, size_t n, double *energy) {
  return guarded([&] {
    require(m != nullptr, "meter must not be NULL");
    require(first <= m->num_steps() && n <= m->num_steps() - first, "steps [first, first + n) are not all finished");
    if (n == 0) return;
    require(energy != nullptr, "energy must not be NULL");
    m->ctx->use();
    EARHIP_HIP(hipMemcpyAsync(energy, m->steps.p + first * (size_t)m->C, sizeof(double) * n * (size_t)m->C, hipMemcpyDeviceToHost,
                              m->ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(m->ctx->stream));
  });
}

int earhip_loudness_result(earhip_loudness *m, const double *weights, double *integrated, double *max_momentary,
                           double *max_short_term) {
  return guarded([&] {
    require(m != nullptr && weights != nullptr, "meter and weights must not be NULL");
    m->ctx->use();
    const size_t n = m->num_steps();
    std::vector<double> en(std::max<size_t>(n * (size_t)m->C, 1));
    if (n) EARHIP_HIP(hipMemcpyAsync(en.data(), m->steps.p, sizeof(double) * n * (size_t)m->C, hipMemcpyDeviceToHost, m->ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(m->ctx->stream));
    loudness_gate(n, m->C, en.data(), weights, integrated, max_momentary, max_short_term);
  });
}

int earhip_loudness_peaks(earhip_loudness *m, float *true_peak, float *sample_peak) {
  return guarded([&] {
    require(m != nullptr, "meter must not be NULL");
    require(m->tp_on, "the meter was made without true peak (earhip_loudness_create_tp)");
    m->ctx->use();
    // every finished step and the open one, reduced on the device: 2 x C numbers come back, whatever the programme's length
    const size_t C = (size_t)m->C;
    hipLaunchKernelGGL(k_true_peak_totals, dim3((unsigned)C, 2), dim3(256), 0, m->ctx->stream, m->tp_steps.p, m->sp_steps.p,
                       (unsigned long long)(m->num_steps() + 1), m->C, m->tp_totals.p);
    EARHIP_HIP(hipGetLastError());
    EARHIP_HIP(hipMemcpyAsync(m->p_totals.p, m->tp_totals.p, sizeof(float) * 2 * C, hipMemcpyDeviceToHost, m->ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(m->ctx->stream));
    if (true_peak) std::memcpy(true_peak, m->p_totals.p, sizeof(float) * C);
    if (sample_peak) std::memcpy(sample_peak, m->p_totals.p + C, sizeof(float) * C);
  });
}

int earhip_loudness_step_peaks(earhip_loudness *m, size_t first, size_t n, float *true_peak, float *sample_peak) {
  return guarded([&] {
    require(m != nullptr, "meter must not be NULL");
    require(m->tp_on, "the meter was made without true peak (earhip_loudness_create_tp)");
    require(first <= m->num_steps() && n <= m->num_steps() - first, "steps [first, first + n) are not all finished");
    if (n == 0) return;
    m->ctx->use();
    const size_t C = (size_t)m->C;
    if (true_peak)
      EARHIP_HIP(hipMemcpyAsync(true_peak, m->tp_steps.p + first * C, sizeof(float) * n * C, hipMemcpyDeviceToHost, m->ctx->stream));
    if (sample_peak)
      EARHIP_HIP(hipMemcpyAsync(sample_peak, m->sp_steps.p + first * C, sizeof(float) * n * C, hipMemcpyDeviceToHost, m->ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(m->ctx->stream));
  });
}

int earhip_loudness_range(size_t n_steps, int n_channels, const double *energy, const double *weights, double *lra, double *low,
                          double *high) {
  return guarded([&] {
    require(n_channels >= 1, "n_channels must be >= 1");
    require(weights != nullptr && (n_steps == 0 || energy != nullptr), "energy and weights must not be NULL");
    loudness_range(n_steps, n_channels, energy, weights, lra, low, high);
  });
}

int earhip_loudness_result_range(earhip_loudness *m, const double *weights, double *lra, double *low, double *high) {
  return guarded([&] {
    require(m != nullptr && weights != nullptr, "meter and weights must not be NULL");
    m->ctx->use();
    const size_t n = m->num_steps();
    std::vector<double> en(std::max<size_t>(n * (size_t)m->C, 1));
    if (n) EARHIP_HIP(hipMemcpyAsync(en.data(), m->steps.p, sizeof(double) * n * (size_t)m->C, hipMemcpyDeviceToHost, m->ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(m->ctx->stream));
    loudness_range(n, m->C, en.data(), weights, lra, low, high);
  });
}

int earhip_loudness_gate(size_t n_steps, int n_channels, const double *energy, const double *weights, double *integrated,
                         double *max_momentary, double *max_short_term) {
  return guarded([&] {
    require(n_channels >= 1, "n_channels must be >= 1");
    require(weights != nullptr && (n_steps == 0 || energy != nullptr), "energy and weights must not be NULL");
    loudness_gate(n_steps, n_channels, energy, weights, integrated, max_momentary, max_short_term);
  });
}

int earhip_loudness_layout_weights(const char *layout, double *weights) {
  return guarded([&] {
    require(layout != nullptr && weights != nullptr, "layout and weights must not be NULL");
    const LayoutEntry *L = &find_layout(layout);
    for (int c = 0; c < L->n; c++)
      weights[c] = loudness_channel_weight(L->channels[c].azimuth, L->channels[c].elevation, L->channels[c].is_lfe);
  });
}

}  // extern "C"
