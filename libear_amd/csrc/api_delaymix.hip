// api_delaymix.hip — group S of include/earhip.h: a sparse matrix of delayed short FIRs on planar float32 rows in device
// memory.  The kernels: delaymix_kernels.h; the maths they share with the CPU tests: delaymix.h.
#include <algorithm>
#include <memory>

#include "common.h"
#include "delaymix_kernels.h"

using namespace earhip;

struct earhip_delaymix {
  earhip_ctx *ctx = nullptr;
  int n_in = 0, n_out = 0, n_routes = 0, H = 0, max_fan_in = 0, total_taps = 0;
  uint64_t reads = 0;
  size_t max_samples = 0;
  int par = 0;  // which half of hist holds the history in front of the next launch
  // everything a process call touches, made at create
  DevBuf<DelaymixEntry> entries;
  DevBuf<int> row_start;
  DevBuf<float> taps;
  DevBuf<float> hist;         // [2][n_in][H]
  DevBuf<float> d_in, d_out;  // the host form's rows: [n_in][max_samples], [n_out][max_samples]
  PinBuf<float> pin;          // the host form's staging: max(n_in, n_out) rows of max_samples

  size_t device_bytes() const {
    return sizeof(DelaymixEntry) * entries.n + sizeof(int) * row_start.n + sizeof(float) * (taps.n + hist.n + d_in.n + d_out.n);
  }

  void zero() {
    EARHIP_HIP(hipMemsetAsync(hist.p, 0, sizeof(float) * hist.n, ctx->stream));
    par = 0;
  }

  void launch(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    DelaymixArgs a;
    a.in = in, a.in_stride = in_stride, a.out = out, a.out_stride = out_stride;
    a.n = (int)n, a.H = H;
    a.entries = entries.p, a.row_start = row_start.p, a.taps = taps.p, a.reads = reads;
    const size_t half = (size_t)n_in * (size_t)H;
    a.hist_in = hist.p + (size_t)par * half, a.hist_out = hist.p + (size_t)(par ^ 1) * half;
    // (an output row that does not start on a 16-byte boundary has up to 3 samples of a tile in front of it)
    const unsigned tiles = (unsigned)((n + 3 + kDelaymixTile - 1) / kDelaymixTile);
    hipLaunchKernelGGL(k_delaymix, dim3(tiles, (unsigned)n_out), dim3(kDelaymixThreads), 0, ctx->stream, a);
    if (H > 0) {
      const unsigned blocks = (unsigned)((H + kDelaymixThreads - 1) / kDelaymixThreads);
      hipLaunchKernelGGL(k_delaymix_history, dim3(blocks, (unsigned)n_in), dim3(kDelaymixThreads), 0, ctx->stream, a);
      par ^= 1;
    }
    EARHIP_HIP(hipGetLastError());
  }

  // device rows; the caller has checked the length and the strides
  void feed(size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride) {
    for (size_t at = 0; at < nsamples;) {
      const size_t n = std::min(kDelaymixMaxLaunch, nsamples - at);
      launch(n, in + at, in_stride, out + at, out_stride);
      at += n;
    }
  }
};

extern "C" {

int earhip_delaymix_create(earhip_ctx *ctx, const earhip_delaymix_config *cfg, earhip_delaymix **out) {
  return guarded([&] {
    require(cfg != nullptr, "config must not be NULL");
    if (const char *why = delaymix_check_shape(cfg->n_in, cfg->n_out, cfg->n_routes, cfg->max_samples)) fail_invalid(why);
    require(cfg->routes != nullptr, "routes must not be NULL");
    std::vector<DelaymixRoute> routes((size_t)cfg->n_routes);
    for (int r = 0; r < cfg->n_routes; r++) {
      const earhip_delaymix_route &q = cfg->routes[r];
      routes[(size_t)r].in = q.in, routes[(size_t)r].out = q.out, routes[(size_t)r].delay = q.delay, routes[(size_t)r].n_taps = q.n_taps;
      std::copy(q.taps, q.taps + kDelaymixMaxTaps, routes[(size_t)r].taps);
    }
    if (const char *why = delaymix_check_routes(cfg->n_in, cfg->n_out, cfg->n_routes, routes.data())) fail_invalid(why);
    require(ctx != nullptr && out != nullptr, "ctx and out must not be NULL");
    ctx->use();
    const DelaymixTables t = delaymix_tables(cfg->n_out, cfg->n_routes, routes.data());
    std::unique_ptr<earhip_delaymix> s(new earhip_delaymix);
    s->ctx = ctx;
    s->n_in = cfg->n_in, s->n_out = cfg->n_out, s->n_routes = cfg->n_routes;
    s->H = t.history, s->max_fan_in = t.max_fan_in, s->total_taps = (int)t.taps.size(), s->reads = t.reads;
    s->max_samples = cfg->max_samples;
    s->entries.alloc(t.entries.size());
    s->row_start.alloc(t.row_start.size());
    s->taps.alloc(t.taps.size());
    EARHIP_HIP(hipMemcpy(s->entries.p, t.entries.data(), sizeof(DelaymixEntry) * t.entries.size(), hipMemcpyHostToDevice));
    EARHIP_HIP(hipMemcpy(s->row_start.p, t.row_start.data(), sizeof(int) * t.row_start.size(), hipMemcpyHostToDevice));
    EARHIP_HIP(hipMemcpy(s->taps.p, t.taps.data(), sizeof(float) * t.taps.size(), hipMemcpyHostToDevice));
    s->hist.alloc(2 * (size_t)s->n_in * (size_t)s->H);
    s->d_in.alloc((size_t)s->n_in * s->max_samples);
    s->d_out.alloc((size_t)s->n_out * s->max_samples);
    s->pin.reserve((size_t)std::max(s->n_in, s->n_out) * s->max_samples);
    s->zero();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    *out = s.release();
  });
}

int earhip_delaymix_destroy(earhip_delaymix *dm) {
  return guarded([&] {
    if (!dm) return;
    (void)hipSetDevice(dm->ctx->device);
    (void)hipStreamSynchronize(dm->ctx->stream);
    delete dm;
  });
}

int earhip_delaymix_reset(earhip_delaymix *dm) {
  return guarded([&] {
    require(dm != nullptr, "dm must not be NULL");
    dm->ctx->use();
    dm->zero();
  });
}

int earhip_delaymix_info(const earhip_delaymix *dm, earhip_delaymix_properties *info) {
  return guarded([&] {
    require(dm != nullptr && info != nullptr, "dm and info must not be NULL");
    info->tile_out = kDelaymixTile;
    info->launch_in = kDelaymixMaxLaunch;
    info->routes = dm->n_routes;
    info->history = dm->H;
    info->max_fan_in = dm->max_fan_in;
    info->total_taps = dm->total_taps;
    info->device_bytes = dm->device_bytes();
  });
}

int earhip_delaymix_process_device(earhip_delaymix *dm, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                                   size_t out_stride) {
  return guarded([&] {
    require(dm != nullptr, "dm must not be NULL");
    if (nsamples > dm->max_samples) fail_invalid("the call would pass the matrix's max_samples (nothing was consumed)");
    if (nsamples == 0) return;
    require(in_dev != nullptr && out_dev != nullptr, "in_dev and out_dev must not be NULL");
    require(in_stride >= nsamples && out_stride >= nsamples, "a stride is smaller than nsamples");
    dm->ctx->use();
    dm->feed(nsamples, in_dev, in_stride, out_dev, out_stride);
  });
}

int earhip_delaymix_process(earhip_delaymix *dm, size_t nsamples, const float *const *in, float *const *out) {
  return guarded([&] {
    require(dm != nullptr, "dm must not be NULL");
    if (nsamples > dm->max_samples) fail_invalid("the call would pass the matrix's max_samples (nothing was consumed)");
    if (nsamples == 0) return;
    require(in != nullptr && out != nullptr, "in and out must not be NULL");
    for (int c = 0; c < dm->n_in; c++) require(!(dm->reads >> c & 1) || in[c] != nullptr, "a row pointer is NULL");
    for (int k = 0; k < dm->n_out; k++) require(out[k] != nullptr, "a row pointer is NULL");
    earhip_ctx *ctx = dm->ctx;
    ctx->use();
    const size_t n = nsamples;
    float *pin = dm->pin.p;
    // (a row no route reads is not looked at: its staging keeps whatever it held, and no kernel reads it)
    for (int c = 0; c < dm->n_in; c++)
      if (dm->reads >> c & 1) std::copy(in[c], in[c] + n, pin + (size_t)c * n);
    EARHIP_HIP(hipMemcpyAsync(dm->d_in.p, pin, sizeof(float) * n * (size_t)dm->n_in, hipMemcpyHostToDevice, ctx->stream));
    dm->feed(n, dm->d_in.p, n, dm->d_out.p, n);
    EARHIP_HIP(hipMemcpyAsync(pin, dm->d_out.p, sizeof(float) * n * (size_t)dm->n_out, hipMemcpyDeviceToHost, ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < dm->n_out; k++) std::copy(pin + (size_t)k * n, pin + (size_t)(k + 1) * n, out[k]);
  });
}

int earhip_delaymix_fractional(double delay, int n_taps, double beta, int *whole, double *taps) {
  return guarded([&] {
    require(whole != nullptr && taps != nullptr, "whole and taps must not be NULL");
    if (const char *why = delaymix_fractional(delay, n_taps, beta, whole, taps)) fail_invalid(why);
  });
}

int earhip_delaymix_align(int n, const double *distance_m, double sample_rate, double speed_of_sound, double *delay_samples,
                          double *gain) {
  return guarded([&] {
    require(distance_m != nullptr && delay_samples != nullptr && gain != nullptr, "distance_m, delay_samples and gain must not be NULL");
    if (const char *why = delaymix_align(n, distance_m, sample_rate, speed_of_sound, delay_samples, gain)) fail_invalid(why);
  });
}

}  // extern "C"
