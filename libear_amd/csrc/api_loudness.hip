// api_loudness.hip — group L of include/earhip.h: programme loudness (ITU-R BS.1770-4), true peak (its annex 2) and loudness
// range (EBU Tech 3342) measured on the device.  The kernels: loudness_kernels.h, true_peak_kernels.h; the maths they share
// with the host functions and the CPU tests: loudness.h, true_peak.h.
#include <cstring>
#include <memory>

#include "bus_stage.h"
#include "layout_registry.h"
#include "loudness_kernels.h"
#include "true_peak_kernels.h"

using namespace earhip;

struct earhip_loudness : BusStage {  // (n_in: the channels; n_out = 0: it only reads)
  static constexpr StageWords words = {
      "meter must not be NULL",
      "rows_dev must not be NULL", "",
      "stride too small", "",
      "rows must not be NULL", "",
      "a row pointer is NULL", ""};
  earhip_loudness() { noun = "meter", room_name = "max_steps"; }  // (room: the steps the store holds)
  int rate = 0, step = 0, L = 0;
  KCoeffs<double> k;
  unsigned long long clock = 0;  // samples since create / reset (the kernels get what they need of it as arguments)
  Halves par;                    // which `open` word holds the sum of the unfinished step, and which half of tp_hist is read
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
  DevBuf<float> tp_table;  // [phases][taps]
  DevBuf<float> tp_hist;   // [2][C][kTpHist], the halves taken by `par` as the `open` words are
  DevBuf<unsigned> tp_steps, sp_steps;  // [max_steps + 1][C]: the row behind the finished steps is the open step's
  DevBuf<unsigned> tp_totals;           // [2][C]: what earhip_loudness_peaks reduces the stores to
  PinBuf<float> p_totals;

  size_t max_launch() const { return (size_t)(kLoudMaxChunks - 1) * (size_t)L; }
  size_t num_steps() const { return (size_t)(clock / (unsigned long long)step); }

  void check_room(size_t nsamples) const override {
    if ((clock + nsamples) / (unsigned long long)step > room)
      fail_invalid("the call would pass the loudness meter's max_steps (nothing was consumed)");
  }

  void zero() override {
    EARHIP_HIP(hipMemsetAsync(state.p, 0, sizeof(double) * state.n, ctx->stream));
    EARHIP_HIP(hipMemsetAsync(open.p, 0, sizeof(double) * open.n, ctx->stream));
    EARHIP_HIP(hipMemsetAsync(steps.p, 0, sizeof(double) * steps.n, ctx->stream));
    if (tp_on) {
      EARHIP_HIP(hipMemsetAsync(tp_hist.p, 0, sizeof(float) * tp_hist.n, ctx->stream));
      EARHIP_HIP(hipMemsetAsync(tp_steps.p, 0, sizeof(unsigned) * tp_steps.n, ctx->stream));
      EARHIP_HIP(hipMemsetAsync(sp_steps.p, 0, sizeof(unsigned) * sp_steps.n, ctx->stream));
    }
    clock = 0;
    par.par = 0;
  }

  // the true-peak pass over one launch's samples: it reads what the loudness passes read and shares nothing else with them
  void launch_true_peak(size_t n, const float *rows, size_t stride) {
    TpArgs t;
    t.rows = rows;
    t.stride = stride;
    t.n = (unsigned)n;
    t.C = n_in;
    t.r0 = (unsigned)(clock % (unsigned long long)step);
    t.step = (unsigned)step;
    t.step0 = clock / (unsigned long long)step;
    t.hist_in = tp_hist.p + par.in(), t.hist_out = tp_hist.p + par.out();
    t.tp = tp_steps.p, t.sp = sp_steps.p;
    t.phases = tp_phases, t.taps = tp_taps;
    t.table = tp_table.p;
    std::memcpy(t.h, tp_h, sizeof(tp_h));
    if (tp_phases == 4 && tp_taps == 12)
      hipLaunchKernelGGL(k_true_peak_4x12, dim3((unsigned)((n + kTpBlockTile - 1) / kTpBlockTile), (unsigned)n_in), dim3(64 * kTpWaves), 0,
                         ctx->stream, t);
    else
      hipLaunchKernelGGL(k_true_peak_any, dim3((unsigned)((n + kTpAnyTile - 1) / kTpAnyTile), (unsigned)n_in), dim3(kTpAnyTile), 0,
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
    a.C = n_in;
    a.k = k;
    a.e = e.p, a.start = start.p, a.q = q.p, a.state = state.p, a.P = P.p, a.Q = Q.p;
    a.open = open.p;
    a.par = par.par;
    a.cps = (unsigned)(step / L);
    a.chunk0_in_step = (unsigned)((clock / (unsigned long long)L) % a.cps);
    a.step0 = clock / (unsigned long long)step;
    a.steps = steps.p;
    a.step_samples = (double)step;
    if (a.nchunks > (unsigned)kLoudMaxChunks) fail_internal("loudness launch beyond its scratch");
    if (tp_on) launch_true_peak(n, rows, stride);
    const unsigned touched = (a.chunk0_in_step + a.nchunks + a.cps - 1) / a.cps;
    const dim3 grid((a.nchunks + 63) / 64, (unsigned)n_in);
    hipLaunchKernelGGL(k_loudness_pass<false>, grid, dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_loudness_propagate, dim3((unsigned)n_in), dim3(kLoudPropThreads), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_loudness_pass<true>, grid, dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_loudness_steps, dim3((touched * (unsigned)n_in + 63) / 64), dim3(64), 0, ctx->stream, a, touched);
    EARHIP_HIP(hipGetLastError());
    clock += n;
    par.flip();
  }

  void feed(size_t nsamples, const float *rows, size_t stride, float *, size_t) override {
    for_each_launch(nsamples, max_launch(), [&](size_t at, size_t n, size_t) {
      launch(n, rows + at, stride);
      return n;
    });
  }
};

template <>
BusStage *earhip::as_stage<earhip_loudness>(earhip_loudness *h) {
  return h;
}

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
    m->n_in = n_channels;
    m->rate = sample_rate;
    m->step = sample_rate / 10;
    m->L = loudness_chunk_length(m->step, 240);
    m->room = max_steps;
    m->par.half = (size_t)n_channels * kTpHist;
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
    m->P.upload(P);
    m->Q.upload(Q);
    if (tp) {
      m->tp_on = true;
      m->tp_phases = table.phases, m->tp_taps = table.taps;
      std::memcpy(m->tp_h, table.h, sizeof(m->tp_h));
      m->tp_table.upload(table.v);
      m->tp_hist.alloc(2 * C * kTpHist);
      m->tp_steps.alloc((max_steps + 1) * C);
      m->sp_steps.alloc((max_steps + 1) * C);
      m->tp_totals.alloc(2 * C);
      m->p_totals.reserve(2 * C);
    }
    m->p_stage.reserve(C * earhip_loudness::kStage);
    m->d_stage.alloc(C * earhip_loudness::kStage);
    stage_ready(m, out);
  });
}

int earhip_loudness_destroy(earhip_loudness *m) { return stage_destroy(m); }
int earhip_loudness_reset(earhip_loudness *m) { return stage_reset(m); }

int earhip_loudness_process_device(earhip_loudness *m, size_t nsamples, const float *rows_dev, size_t stride) {
  return guarded([&] {
    if (!stage_admits(m, nsamples)) return;
    check_device_rows(earhip_loudness::words, nsamples, rows_dev, stride, 0, nullptr, 0);
    m->ctx->use();
    m->feed(nsamples, rows_dev, stride, nullptr, 0);
  });
}

// (a call has no longest length, so its rows go through the staging in pieces of kStage samples)
int earhip_loudness_process(earhip_loudness *m, size_t nsamples, const float *const *rows) {
  return guarded([&] {
    if (!stage_admits(m, nsamples)) return;
    check_host_rows(earhip_loudness::words, nsamples, rows, m->n_in, reads_every_row, 0, nullptr, 0);
    earhip_ctx *ctx = m->ctx;
    ctx->use();
    for_each_launch(nsamples, earhip_loudness::kStage, [&](size_t at, size_t n, size_t) {
      for (int c = 0; c < m->n_in; c++) std::memcpy(m->p_stage.p + (size_t)c * n, rows[c] + at, sizeof(float) * n);
      EARHIP_HIP(hipMemcpyAsync(m->d_stage.p, m->p_stage.p, sizeof(float) * n * m->n_in, hipMemcpyHostToDevice, ctx->stream));
      m->feed(n, m->d_stage.p, n, nullptr, 0);
      EARHIP_HIP(hipStreamSynchronize(ctx->stream));  // (the one staging buffer is free again)
      return n;
    });
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
    EARHIP_HIP(hipMemcpyAsync(energy, m->steps.p + first * (size_t)m->n_in, sizeof(double) * n * (size_t)m->n_in, hipMemcpyDeviceToHost,
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
    std::vector<double> en(std::max<size_t>(n * (size_t)m->n_in, 1));
    if (n) EARHIP_HIP(hipMemcpyAsync(en.data(), m->steps.p, sizeof(double) * n * (size_t)m->n_in, hipMemcpyDeviceToHost, m->ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(m->ctx->stream));
    loudness_gate(n, m->n_in, en.data(), weights, integrated, max_momentary, max_short_term);
  });
}

int earhip_loudness_peaks(earhip_loudness *m, float *true_peak, float *sample_peak) {
  return guarded([&] {
    require(m != nullptr, "meter must not be NULL");
    require(m->tp_on, "the meter was made without true peak (earhip_loudness_create_tp)");
    m->ctx->use();
    // every finished step and the open one, reduced on the device: 2 x C numbers come back, whatever the programme's length
    const size_t C = (size_t)m->n_in;
    hipLaunchKernelGGL(k_true_peak_totals, dim3((unsigned)C, 2), dim3(256), 0, m->ctx->stream, m->tp_steps.p, m->sp_steps.p,
                       (unsigned long long)(m->num_steps() + 1), m->n_in, m->tp_totals.p);
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
    const size_t C = (size_t)m->n_in;
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
    std::vector<double> en(std::max<size_t>(n * (size_t)m->n_in, 1));
    if (n) EARHIP_HIP(hipMemcpyAsync(en.data(), m->steps.p, sizeof(double) * n * (size_t)m->n_in, hipMemcpyDeviceToHost, m->ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(m->ctx->stream));
    loudness_range(n, m->n_in, en.data(), weights, lra, low, high);
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
