// api_src.hip — group P of include/earhip.h: a polyphase sample-rate converter on planar float32 rows in device memory.  The
// kernels: src_kernels.h; the maths they share with the CPU tests: src.h.
#include <algorithm>
#include <memory>

#include "common.h"
#include "src_kernels.h"

using namespace earhip;

struct earhip_src {
  earhip_ctx *ctx = nullptr;
  int C = 0, L = 0, M = 0, T = 0, H = 0;
  SrcShape shape;
  size_t max_samples = 0, max_out = 0;
  uint64_t clock = 0;  // input samples since create / reset
  int par = 0;         // which half of hist holds the history in front of the next launch
  // everything a process call touches, made at create
  DevBuf<float> table;        // [L][pitch]
  DevBuf<float> hist;         // [2][C][H]
  DevBuf<float> d_in, d_out;  // the host form's rows: [C][max_samples], [C][max_out]
  PinBuf<float> pin;          // the host form's staging: max(max_samples, max_out) per channel

  void zero() {
    EARHIP_HIP(hipMemsetAsync(hist.p, 0, sizeof(float) * hist.n, ctx->stream));
    clock = 0;
    par = 0;
  }

  size_t next_out(size_t nsamples) const { return src_outputs(nsamples, src_lead(clock, L, M), L, M); }

  // what a call of nsamples would write, after the checks that let it consume nothing
  size_t admit(size_t nsamples, size_t out_capacity) const {
    if (nsamples > max_samples) fail_invalid("the call would pass the converter's max_samples (nothing was consumed)");
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
    const size_t half = (size_t)C * (size_t)H;
    a.hist_in = hist.p + (size_t)par * half, a.hist_out = hist.p + (size_t)(par ^ 1) * half;
    const unsigned tiles = (a.n_out + kSrcTile - 1) / kSrcTile;
    // enough workgroups for every CU several times over before a workgroup keeps its table for more than one tile
    a.tiles_per_wg = (int)std::min<unsigned>(8u, std::max<unsigned>(1u, tiles * (unsigned)C / (unsigned)(8 * std::max(ctx->num_cus, 1))));
    if (a.n_out > 0) {
      const dim3 grid((tiles + (unsigned)a.tiles_per_wg - 1) / (unsigned)a.tiles_per_wg, (unsigned)C);
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
      hipLaunchKernelGGL(k_src_history, dim3((unsigned)C), dim3(kSrcThreads), 0, ctx->stream, a);
      par ^= 1;
    }
    EARHIP_HIP(hipGetLastError());
    clock += n;
  }

  // device rows; the caller has checked the room, the capacity and the strides
  void feed(size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride) {
    size_t written = 0;
    for (size_t at = 0; at < nsamples;) {
      const size_t n = std::min(kSrcMaxLaunch, nsamples - at);
      const size_t n_out = next_out(n);
      launch(n, in + at, in_stride, out + written, out_stride);
      at += n, written += n_out;
    }
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
    s->C = cfg->channels, s->L = L, s->M = M, s->T = T, s->H = T - 1;
    s->shape = src_shape(L, M, T);
    s->max_samples = cfg->max_samples;
    s->max_out = src_max_outputs(cfg->max_samples, L, M);
    std::vector<float> table((size_t)L * s->shape.pitch);
    src_table_make(cfg->taps, L, T, table.data());
    s->table.alloc(table.size());
    EARHIP_HIP(hipMemcpy(s->table.p, table.data(), sizeof(float) * table.size(), hipMemcpyHostToDevice));
    s->hist.alloc(2 * (size_t)s->C * (size_t)s->H);
    s->d_in.alloc((size_t)s->C * s->max_samples);
    s->d_out.alloc((size_t)s->C * s->max_out);
    s->pin.reserve((size_t)s->C * std::max(s->max_samples, s->max_out));
    s->zero();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    *out = s.release();
  });
}

int earhip_src_destroy(earhip_src *src) {
  return guarded([&] {
    if (!src) return;
    (void)hipSetDevice(src->ctx->device);
    (void)hipStreamSynchronize(src->ctx->stream);
    delete src;
  });
}

int earhip_src_reset(earhip_src *src) {
  return guarded([&] {
    require(src != nullptr, "src must not be NULL");
    src->ctx->use();
    src->zero();
  });
}

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
    if (nsamples > src->max_samples) fail_invalid("nsamples is beyond the converter's max_samples");
    *n_out = src->next_out(nsamples);
  });
}

int earhip_src_process_device(earhip_src *src, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                              size_t out_stride, size_t out_capacity, size_t *n_out) {
  return guarded([&] {
    require(src != nullptr, "src must not be NULL");
    const size_t produced = src->admit(nsamples, out_capacity);
    if (nsamples > 0) {
      require(in_dev != nullptr, "in_dev must not be NULL");
      require(in_stride >= nsamples, "in_stride too small");
    }
    if (produced > 0) {
      require(out_dev != nullptr, "out_dev must not be NULL");
      require(out_stride >= produced, "out_stride too small");
    }
    if (n_out) *n_out = produced;
    if (nsamples == 0) return;
    src->ctx->use();
    src->feed(nsamples, in_dev, in_stride, out_dev, out_stride);
  });
}

int earhip_src_process(earhip_src *src, size_t nsamples, const float *const *in, float *const *out, size_t out_capacity,
                       size_t *n_out) {
  return guarded([&] {
    require(src != nullptr, "src must not be NULL");
    const size_t produced = src->admit(nsamples, out_capacity);
    if (nsamples > 0) {
      require(in != nullptr, "in must not be NULL");
      for (int c = 0; c < src->C; c++) require(in[c] != nullptr, "a row pointer is NULL");
    }
    if (produced > 0) {
      require(out != nullptr, "out must not be NULL");
      for (int c = 0; c < src->C; c++) require(out[c] != nullptr, "a row pointer is NULL");
    }
    if (n_out) *n_out = produced;
    if (nsamples == 0) return;
    earhip_ctx *ctx = src->ctx;
    ctx->use();
    const size_t n = nsamples;
    float *pin = src->pin.p;
    for (int c = 0; c < src->C; c++) std::copy(in[c], in[c] + n, pin + (size_t)c * n);
    EARHIP_HIP(hipMemcpyAsync(src->d_in.p, pin, sizeof(float) * n * (size_t)src->C, hipMemcpyHostToDevice, ctx->stream));
    src->feed(n, src->d_in.p, n, src->d_out.p, std::max<size_t>(produced, 1));
    if (produced > 0)
      EARHIP_HIP(hipMemcpyAsync(pin, src->d_out.p, sizeof(float) * produced * (size_t)src->C, hipMemcpyDeviceToHost, ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < src->C; c++) std::copy(pin + (size_t)c * produced, pin + (size_t)(c + 1) * produced, out[c]);
  });
}

int earhip_src_design(int up, int down, int taps_per_phase, double beta, double cutoff, double *out) {
  return guarded([&] {
    require(out != nullptr, "out must not be NULL");
    if (const char *why = src_design(up, down, taps_per_phase, beta, cutoff, out)) fail_invalid(why);
  });
}

}  // extern "C"
