// api_delaymix.hip — group S of include/earhip.h: a sparse matrix of delayed short FIRs on planar float32 rows in device
// memory.  The kernels: delaymix_kernels.h; the maths they share with the CPU tests: delaymix.h.
#include <algorithm>
#include <memory>

#include "bus_stage.h"
#include "delaymix_kernels.h"

using namespace earhip;

struct earhip_delaymix : BusStage {
  static constexpr StageWords words = {
      "dm must not be NULL",
      "in_dev and out_dev must not be NULL", "in_dev and out_dev must not be NULL",
      "a stride is smaller than nsamples", "a stride is smaller than nsamples",
      "in and out must not be NULL", "in and out must not be NULL",
      "a row pointer is NULL", "a row pointer is NULL"};
  earhip_delaymix() { noun = "matrix", room_name = "max_samples"; }
  int n_routes = 0, H = 0, max_fan_in = 0, total_taps = 0;
  uint64_t reads = 0;
  // everything a process call touches, made at create
  DevBuf<DelaymixEntry> entries;
  DevBuf<int> row_start;
  DevBuf<float> taps;
  PingPong<float> hist;  // [2][n_in][H]
  HostRows host;         // [n_in][max_samples], [n_out][max_samples]

  size_t device_bytes() const {
    return sizeof(DelaymixEntry) * entries.n + sizeof(int) * row_start.n +
           sizeof(float) * (taps.n + hist.buf.n + host.d_in.n + host.d_out.n);
  }

  void zero() override { hist.zero(ctx->stream); }

  void launch(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    DelaymixArgs a;
    a.in = in, a.in_stride = in_stride, a.out = out, a.out_stride = out_stride;
    a.n = (int)n, a.H = H;
    a.entries = entries.p, a.row_start = row_start.p, a.taps = taps.p, a.reads = reads;
    a.hist_in = hist.in(), a.hist_out = hist.out();
    // (an output row that does not start on a 16-byte boundary has up to 3 samples of a tile in front of it)
    const unsigned tiles = (unsigned)((n + 3 + kDelaymixTile - 1) / kDelaymixTile);
    hipLaunchKernelGGL(k_delaymix, dim3(tiles, (unsigned)n_out), dim3(kDelaymixThreads), 0, ctx->stream, a);
    if (H > 0) {
      const unsigned blocks = (unsigned)((H + kDelaymixThreads - 1) / kDelaymixThreads);
      hipLaunchKernelGGL(k_delaymix_history, dim3(blocks, (unsigned)n_in), dim3(kDelaymixThreads), 0, ctx->stream, a);
      hist.flip();
    }
    EARHIP_HIP(hipGetLastError());
  }

  void feed(size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride) override {
    for_each_launch(nsamples, kDelaymixMaxLaunch, [&](size_t at, size_t n, size_t) {
      launch(n, in + at, in_stride, out + at, out_stride);
      return n;
    });
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
    s->room = cfg->max_samples;
    s->entries.upload(t.entries);
    s->row_start.upload(t.row_start);
    s->taps.upload(t.taps);
    s->hist.alloc((size_t)s->n_in * (size_t)s->H);
    s->host.alloc((size_t)s->n_in * s->room, (size_t)s->n_out * s->room);
    stage_ready(s, out);
  });
}

int earhip_delaymix_destroy(earhip_delaymix *dm) { return stage_destroy(dm); }
int earhip_delaymix_reset(earhip_delaymix *dm) { return stage_reset(dm); }

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
  return guarded([&] { stage_process_device(dm, nsamples, in_dev, in_stride, out_dev, out_stride); });
}

int earhip_delaymix_process(earhip_delaymix *dm, size_t nsamples, const float *const *in, float *const *out) {
  return guarded([&] { stage_process_host(dm, nsamples, in, out, [&](int c) { return (dm->reads >> c & 1) != 0; }); });
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
