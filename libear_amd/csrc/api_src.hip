// api_src.hip — group P of include/earhip.h: a polyphase sample-rate converter on planar float32 rows in device memory.  The
// kernels: src_kernels.h; the maths they share with the CPU tests: src.h.
#include <algorithm>
#include <memory>

#include "bus_stage.h"
#include "src_kernels.h"

using namespace earhip;

struct earhip_src : BusStage {  // (n_in = n_out = the channels)
  static constexpr StageWords words = {
      "src must not be NULL",
      "in_dev must not be NULL", "out_dev must not be NULL",
      "in_stride too small", "out_stride too small",
      "in must not be NULL", "out must not be NULL",
      "a row pointer is NULL", "a row pointer is NULL"};
  earhip_src() { noun = "converter", room_name = "max_samples"; }
  int L = 0, M = 0, T = 0, H = 0;
  SrcShape shape;
  size_t max_out = 0;
  uint64_t clock = 0;  // input samples since create / reset
  // everything a process call touches, made at create
  DevBuf<float> table;   // [L][pitch]
  PingPong<float> hist;  // [2][C][H]
  HostRows host;         // [C][max_samples], [C][max_out]

  void zero() override {
    hist.zero(ctx->stream);
    clock = 0;
  }

  size_t next_out(size_t nsamples) const { return src_outputs(nsamples, src_lead(clock, L, M), L, M); }

  // what a call of nsamples would write, after the checks that let it consume nothing
  size_t admit(size_t nsamples, size_t out_capacity) const {
    const size_t n_out = next_out(nsamples);
    if (n_out > out_capacity) fail_invalid("out_capacity is smaller than the call's outputs (nothing was consumed)");
    return n_out;
  }

  void launch(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    SrcArgs a;
    a.in = in, a.in_stride = in_stride, a.out = out, a.out_stride = out_stride;
    a.n = (unsigned)n, a.r0 = src_lead(clock, L, M);
    a.n_out = (unsigned)src_outputs(n, a.r0, L, M);
    a.L = L, a.M = M, a.T = T, a.H = H, a.pitch = shape.pitch;
    a.window_lds = shape.window_lds, a.table_lds = shape.table_lds, a.window = shape.window;
    a.table = table.p;
    a.hist_in = hist.in(), a.hist_out = hist.out();
    const unsigned tiles = (a.n_out + kSrcTile - 1) / kSrcTile;
    // enough workgroups for every CU several times over before a workgroup keeps its table for more than one tile
    a.tiles_per_wg = (int)std::min<unsigned>(8u, std::max<unsigned>(1u, tiles * (unsigned)n_in / (unsigned)(8 * std::max(ctx->num_cus, 1))));
    if (a.n_out > 0) {
      const dim3 grid((tiles + (unsigned)a.tiles_per_wg - 1) / (unsigned)a.tiles_per_wg, (unsigned)n_in);
      const size_t lds = shape.lds_bytes();
      if (shape.table_lds && shape.window_lds)
        hipLaunchKernelGGL((k_src<true, true>), grid, dim3(kSrcThreads), lds, ctx->stream, a);
      else if (shape.window_lds)
        hipLaunchKernelGGL((k_src<false, true>), grid, dim3(kSrcThreads), lds, ctx->stream, a);
      else if (shape.table_lds)
        hipLaunchKernelGGL((k_src<true, false>), grid, dim3(kSrcThreads), lds, ctx->stream, a);
      else
        hipLaunchKernelGGL((k_src<false, false>), grid, dim3(kSrcThreads), lds, ctx->stream, a);
    }
    if (H > 0) {
      hipLaunchKernelGGL(k_src_history, dim3((unsigned)n_in), dim3(kSrcThreads), 0, ctx->stream, a);
      hist.flip();
    }
    EARHIP_HIP(hipGetLastError());
    clock += n;
  }

  // (the caller has checked the capacity too)
  void feed(size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride) override {
    for_each_launch(nsamples, kSrcMaxLaunch, [&](size_t at, size_t n, size_t written) {
      const size_t n_out = next_out(n);
      launch(n, in + at, in_stride, out + written, out_stride);
      return n_out;
    });
  }
};

extern "C" {

int earhip_src_create(earhip_ctx *ctx, const earhip_src_config *cfg, earhip_src **out) {
  return guarded([&] {
    require(cfg != nullptr, "config must not be NULL");
    if (const char *why = src_check_shape(cfg->channels, cfg->up, cfg->down, cfg->taps_per_phase, cfg->max_samples)) fail_invalid(why);
    require(cfg->taps != nullptr, "taps must not be NULL");
    const int L = cfg->up, M = cfg->down, T = cfg->taps_per_phase;
    if (const char *why = src_check_taps(cfg->taps, (size_t)L * (size_t)T)) fail_invalid(why);
    require(ctx != nullptr && out != nullptr, "ctx and out must not be NULL");
    ctx->use();
    std::unique_ptr<earhip_src> s(new earhip_src);
    s->ctx = ctx;
    s->n_in = s->n_out = cfg->channels, s->L = L, s->M = M, s->T = T, s->H = T - 1;
    s->shape = src_shape(L, M, T);
    s->room = cfg->max_samples;
    s->max_out = src_max_outputs(cfg->max_samples, L, M);
    std::vector<float> table((size_t)L * s->shape.pitch);
    src_table_make(cfg->taps, L, T, table.data());
    s->table.upload(table);
    s->hist.alloc((size_t)s->n_in * (size_t)s->H);
    s->host.alloc((size_t)s->n_in * s->room, (size_t)s->n_in * s->max_out);
    stage_ready(s, out);
  });
}

int earhip_src_destroy(earhip_src *src) { return stage_destroy(src); }
int earhip_src_reset(earhip_src *src) { return stage_reset(src); }

int earhip_src_info(const earhip_src *src, earhip_src_properties *info) {
  return guarded([&] {
    require(src != nullptr && info != nullptr, "src and info must not be NULL");
    info->up = src->L, info->down = src->M, info->taps_per_phase = src->T;
    info->tile_out = kSrcTile, info->tile_in = src->shape.tile_in;
    info->table_in_lds = src->shape.table_lds > 0, info->window_in_lds = src->shape.window_lds > 0;
    info->max_out = src->max_out;
    const double span = (double)src->L * (double)src->T - 1.0;
    info->latency_prototype = span / 2.0;
    info->latency_in = span / (2.0 * (double)src->L);
    info->latency_out = span / (2.0 * (double)src->M);
  });
}

int earhip_src_next_out(const earhip_src *src, size_t nsamples, size_t *n_out) {
  return guarded([&] {
    require(src != nullptr && n_out != nullptr, "src and n_out must not be NULL");
    if (nsamples > src->room) fail_invalid("nsamples is beyond the converter's max_samples");
    *n_out = src->next_out(nsamples);
  });
}

// (a call may bring inputs and produce nothing, so an empty call is one without inputs: it still reports its 0 outputs)
int earhip_src_process_device(earhip_src *src, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                              size_t out_stride, size_t out_capacity, size_t *n_out) {
  return guarded([&] {
    const bool some = stage_admits(src, nsamples);
    const size_t produced = src->admit(nsamples, out_capacity);
    check_device_rows(earhip_src::words, nsamples, in_dev, in_stride, produced, out_dev, out_stride);
    if (n_out) *n_out = produced;
    if (!some) return;
    src->ctx->use();
    src->feed(nsamples, in_dev, in_stride, out_dev, out_stride);
  });
}

int earhip_src_process(earhip_src *src, size_t nsamples, const float *const *in, float *const *out, size_t out_capacity,
                       size_t *n_out) {
  return guarded([&] {
    const bool some = stage_admits(src, nsamples);
    const size_t produced = src->admit(nsamples, out_capacity);
    check_host_rows(earhip_src::words, nsamples, in, src->n_in, reads_every_row, produced, out, src->n_out);
    if (n_out) *n_out = produced;
    if (!some) return;
    hipStream_t stream = src->ctx->stream;
    src->ctx->use();
    src->host.to_device(in, src->n_in, nsamples, stream, reads_every_row);
    src->feed(nsamples, src->host.d_in.p, nsamples, src->host.d_out.p, std::max<size_t>(produced, 1));
    src->host.from_device(out, src->n_out, produced, stream);
  });
}

int earhip_src_design(int up, int down, int taps_per_phase, double beta, double cutoff, double *out) {
  return guarded([&] {
    require(out != nullptr, "out must not be NULL");
    if (const char *why = src_design(up, down, taps_per_phase, beta, cutoff, out)) fail_invalid(why);
  });
}

}  // extern "C"
