// api_limiter.hip — group N of include/earhip.h: a look-ahead true-peak limiter on planar float32 rows in device memory, one
// gain for all channels.  The kernels: limiter_kernels.h; the maths they share with the CPU tests: limiter.h, true_peak.h.
#include <cstring>
#include <memory>

#include "common.h"
#include "limiter_kernels.h"
#include "pcm_frames.h"

using namespace earhip;

struct earhip_limiter {
  earhip_ctx *ctx = nullptr;
  int C = 0;
  float c = 0.0f;
  int detect = 0;
  LimiterShape sh;
  size_t max_samples = 0;
  unsigned long long clock = 0;  // samples since create / reset: the output clock (the dither's t)
  int par = 0;                   // which half of xhist / rhist holds the history in front of the next launch
  float h[4][12];                // the table where its shape is 4 x 12
  // everything a process call touches, made at create
  DevBuf<float> table, xhist, rhist, ones, r;  // [phases][taps]; [2][C][HX]; [2][HR]; [HR] of 1.0f; [max launch]
  DevBuf<unsigned> stat_min;                   // [kLimSlots]
  DevBuf<unsigned long long> stat_count;       // [kLimSlots]
  DevBuf<float> d_in, d_out, d_gain;           // the host form's rows and the PCM form's: [C][max_samples] each, [max_samples]
  PcmLevels levels;                            // the PCM form's

  // a launch's sample indices are ints
  static constexpr size_t kMaxLaunch = (size_t)1 << 24;

  void zero_stats() {
    EARHIP_HIP(hipMemsetAsync(stat_min.p, 0, sizeof(unsigned) * stat_min.n, ctx->stream));
    EARHIP_HIP(hipMemsetAsync(stat_count.p, 0, sizeof(unsigned long long) * stat_count.n, ctx->stream));
  }
  void zero() {
    EARHIP_HIP(hipMemsetAsync(xhist.p, 0, sizeof(float) * xhist.n, ctx->stream));
    for (int b = 0; b < 2; b++)  // r = 1 before the clock starts
      EARHIP_HIP(hipMemcpyAsync(rhist.p + (size_t)b * (size_t)sh.r_hist(), ones.p, sizeof(float) * (size_t)sh.r_hist(),
                                hipMemcpyDeviceToDevice, ctx->stream));
    zero_stats();
    levels.zero(ctx->stream);
    clock = 0;
    par = 0;
  }

  void check_room(size_t nsamples) const {
    if (nsamples > max_samples) fail_invalid("the call would pass the limiter's max_samples (nothing was consumed)");
  }

  void launch(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride, float *gain) {
    LimArgs a;
    a.in = in, a.in_stride = in_stride, a.out = out, a.out_stride = out_stride, a.gain = gain;
    a.n = (unsigned)n, a.C = C, a.c = c;
    a.L = sh.L, a.M = sh.M, a.K = sh.K, a.D = sh.D, a.HX = sh.x_hist(), a.HR = sh.r_hist(), a.phases = sh.phases, a.taps = sh.taps;
    const size_t xh = (size_t)C * (size_t)a.HX, rh = (size_t)a.HR;
    a.xhist_in = xhist.p + (size_t)par * xh, a.xhist_out = xhist.p + (size_t)(par ^ 1) * xh;
    a.rhist_in = rhist.p + (size_t)par * rh, a.rhist_out = rhist.p + (size_t)(par ^ 1) * rh;
    a.r = r.p;
    a.stat_min = stat_min.p, a.stat_count = stat_count.p;
    a.table = table.p;
    std::memcpy(a.h, h, sizeof(h));
    if (!detect)
      hipLaunchKernelGGL(k_lim_detect_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a);
    else if (sh.phases == 4 && sh.taps == 12)
      hipLaunchKernelGGL(k_lim_detect_4x12, dim3((unsigned)((n + kTpWaveTile - 1) / kTpWaveTile)), dim3(64 * kLimDetWaves), 0,
                         ctx->stream, a);
    else
      hipLaunchKernelGGL(k_lim_detect_any, dim3((unsigned)((n + kLimAnyTile - 1) / kLimAnyTile)), dim3(kLimAnyTile), 0, ctx->stream, a);
    const int W = kLimTile + a.HR;
    const size_t lds = sizeof(float) * (size_t)(((W + 3) & ~3) + kLimTile + a.L);
    hipLaunchKernelGGL(k_lim_apply, dim3((unsigned)((n + kLimTile - 1) / kLimTile)), dim3(kLimThreads), lds, ctx->stream, a);
    EARHIP_HIP(hipGetLastError());
    clock += n;
    par ^= 1;
  }

  // device rows; the caller has checked the room and the strides
  void feed(size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride, float *gain) {
    const size_t most = std::min(kMaxLaunch, r.n);
    for (size_t at = 0; at < nsamples;) {
      const size_t n = std::min(most, nsamples - at);
      launch(n, in + at, in_stride, out + at, out_stride, gain ? gain + at : nullptr);
      at += n;
    }
  }
};

namespace earhip {
void limiter_check_room(const earhip_limiter *lim, size_t nsamples) { lim->check_room(nsamples); }
void limiter_feed(earhip_limiter *lim, size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride) {
  lim->feed(nsamples, in, in_stride, out, out_stride, nullptr);
}
const earhip_ctx *limiter_ctx(const earhip_limiter *lim) { return lim->ctx; }
int limiter_channels(const earhip_limiter *lim) { return lim->C; }
}  // namespace earhip

extern "C" {

int earhip_limiter_create(earhip_ctx *ctx, const earhip_limiter_config *cfg, earhip_limiter **out) {
  return guarded([&] {
    require(cfg != nullptr, "config must not be NULL");
    if (const char *why = limiter_check_config(cfg->n_channels, cfg->sample_rate, cfg->ceiling, cfg->lookahead, cfg->hold, cfg->detect,
                                               cfg->max_samples))
      fail_invalid(why);
    require(ctx != nullptr && out != nullptr, "ctx and out must not be NULL");
    TpTable table;  // (detect = 0: none)
    if (cfg->detect)
      if (const char *why = tp_table_make(cfg->tp, cfg->sample_rate, &table)) fail_invalid(why);
    ctx->use();
    std::unique_ptr<earhip_limiter> lim(new earhip_limiter);
    lim->ctx = ctx;
    lim->C = cfg->n_channels, lim->c = cfg->ceiling, lim->detect = cfg->detect;
    lim->sh = limiter_shape(cfg->lookahead, cfg->hold, cfg->detect, table.phases, table.taps);
    lim->max_samples = cfg->max_samples;
    std::memcpy(lim->h, table.h, sizeof(lim->h));
    const size_t C = (size_t)cfg->n_channels, HR = (size_t)lim->sh.r_hist();
    lim->table.alloc(table.v.size());
    if (!table.v.empty()) EARHIP_HIP(hipMemcpy(lim->table.p, table.v.data(), sizeof(float) * table.v.size(), hipMemcpyHostToDevice));
    lim->xhist.alloc(2 * C * (size_t)lim->sh.x_hist());
    lim->rhist.alloc(2 * HR);
    lim->ones.alloc(HR);
    const std::vector<float> ones(HR, 1.0f);
    EARHIP_HIP(hipMemcpy(lim->ones.p, ones.data(), sizeof(float) * HR, hipMemcpyHostToDevice));
    lim->r.alloc(std::min(cfg->max_samples, earhip_limiter::kMaxLaunch));
    lim->stat_min.alloc(kLimSlots);
    lim->stat_count.alloc(kLimSlots);
    lim->d_in.alloc(C * cfg->max_samples);
    lim->d_out.alloc(C * cfg->max_samples);
    lim->d_gain.alloc(cfg->max_samples);
    lim->levels.reserve(cfg->n_channels, ctx->stream);
    lim->zero();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    *out = lim.release();
  });
}

int earhip_limiter_destroy(earhip_limiter *lim) {
  return guarded([&] {
    if (!lim) return;
    (void)hipSetDevice(lim->ctx->device);
    (void)hipStreamSynchronize(lim->ctx->stream);
    delete lim;
  });
}

int earhip_limiter_reset(earhip_limiter *lim) {
  return guarded([&] {
    require(lim != nullptr, "limiter must not be NULL");
    lim->ctx->use();
    lim->zero();
  });
}

int earhip_limiter_latency(const earhip_limiter *lim, int *samples) {
  return guarded([&] {
    require(lim != nullptr && samples != nullptr, "limiter and samples must not be NULL");
    *samples = lim->sh.latency();
  });
}

int earhip_limiter_process_device(earhip_limiter *lim, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                                  size_t out_stride, float *gain_dev) {
  return guarded([&] {
    require(lim != nullptr, "limiter must not be NULL");
    lim->check_room(nsamples);
    if (nsamples == 0) return;
    require(in_dev != nullptr && out_dev != nullptr, "device pointers must not be NULL");
    require(in_stride >= nsamples && out_stride >= nsamples, "stride too small");
    lim->ctx->use();
    lim->feed(nsamples, in_dev, in_stride, out_dev, out_stride, gain_dev);
  });
}

int earhip_limiter_process(earhip_limiter *lim, size_t nsamples, const float *const *in, float *const *out, float *gain) {
  return guarded([&] {
    require(lim != nullptr, "limiter must not be NULL");
    lim->check_room(nsamples);
    if (nsamples == 0) return;
    require(in != nullptr && out != nullptr, "in and out must not be NULL");
    for (int c = 0; c < lim->C; c++) require(in[c] != nullptr && out[c] != nullptr, "a row pointer is NULL");
    earhip_ctx *ctx = lim->ctx;
    ctx->use();
    const size_t n = nsamples;
    rows_to_device(lim->d_in.p, in, lim->C, n, ctx->stream);
    lim->feed(n, lim->d_in.p, n, lim->d_out.p, n, gain ? lim->d_gain.p : nullptr);
    rows_from_device(out, lim->d_out.p, lim->C, n, ctx->stream);
    if (gain) EARHIP_HIP(hipMemcpyAsync(gain, lim->d_gain.p, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
  });
}

int earhip_limiter_process_pcm_device(earhip_limiter *lim, size_t nsamples, const float *in_dev, size_t in_stride, void *out_dev,
                                      size_t out_frame_bytes, size_t out_first_byte, const earhip_pcm_out *out) {
  return guarded([&] {
    require(lim != nullptr, "limiter must not be NULL");
    check_pcm_out_frame(lim->C, check_pcm_out(out), out_dev, out_frame_bytes, out_first_byte, "n_channels");
    lim->check_room(nsamples);
    if (nsamples == 0) return;
    require(in_dev != nullptr, "in_dev must not be NULL");
    require(in_stride >= nsamples, "stride too small");
    earhip_ctx *ctx = lim->ctx;
    ctx->use();
    const int64_t t0 = (int64_t)lim->clock;
    lim->feed(nsamples, in_dev, in_stride, lim->d_out.p, nsamples, nullptr);
    launch_rows_to_pcm(*out, lim->d_out.p, nsamples, lim->C, nsamples, static_cast<unsigned char *>(out_dev), out_frame_bytes,
                       out_first_byte, lim->levels.peak.p, lim->levels.clip.p, t0, ctx->stream);
  });
}

int earhip_limiter_output_levels(earhip_limiter *lim, float *peak, uint64_t *clipped, int reset) {
  return guarded([&] {
    require(lim != nullptr, "limiter must not be NULL");
    require(peak != nullptr && clipped != nullptr, "peak and clipped must not be NULL");
    earhip_ctx *ctx = lim->ctx;
    ctx->use();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    lim->levels.read(lim->C, peak, clipped);
    if (reset) lim->levels.zero(ctx->stream);
  });
}

int earhip_limiter_stats(earhip_limiter *lim, float *min_gain, uint64_t *limited_samples, int reset) {
  return guarded([&] {
    require(lim != nullptr, "limiter must not be NULL");
    require(min_gain != nullptr && limited_samples != nullptr, "min_gain and limited_samples must not be NULL");
    earhip_ctx *ctx = lim->ctx;
    ctx->use();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    unsigned worst[kLimSlots];
    unsigned long long count[kLimSlots];
    EARHIP_HIP(hipMemcpy(worst, lim->stat_min.p, sizeof(worst), hipMemcpyDeviceToHost));
    EARHIP_HIP(hipMemcpy(count, lim->stat_count.p, sizeof(count), hipMemcpyDeviceToHost));
    unsigned w = 0;
    uint64_t sum = 0;
    for (int k = 0; k < kLimSlots; k++) w = std::max(w, worst[k]), sum += count[k];
    const unsigned bits = kLimOneBits - w;
    std::memcpy(min_gain, &bits, sizeof(float));
    *limited_samples = sum;
    if (reset) lim->zero_stats();
  });
}

}  // extern "C"
