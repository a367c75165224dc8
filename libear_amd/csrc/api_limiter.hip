// api_limiter.hip — group N of include/earhip.h: a look-ahead true-peak limiter on planar float32 rows in device memory, one
// gain for all channels.  The kernels: limiter_kernels.h; the maths they share with the CPU tests: limiter.h, true_peak.h.
#include <cstring>
#include <memory>

#include "bus_stage.h"
#include "limiter_kernels.h"
#include "pcm_frames.h"

using namespace earhip;

struct earhip_limiter : BusStage {  // (n_in = n_out = the channels)
  static constexpr StageWords words = {
      "limiter must not be NULL",
      "device pointers must not be NULL", "device pointers must not be NULL",
      "stride too small", "stride too small",
      "in and out must not be NULL", "in and out must not be NULL",
      "a row pointer is NULL", "a row pointer is NULL"};
  earhip_limiter() { noun = "limiter", room_name = "max_samples"; }
  float c = 0.0f;
  int detect = 0;
  LimiterShape sh;
  unsigned long long clock = 0;  // samples since create / reset: the output clock (the dither's t)
  float h[4][12];                // the table where its shape is 4 x 12
  // everything a process call touches, made at create
  DevBuf<float> table, ones, r;           // [phases][taps]; [HR] of 1.0f; [max launch]
  PingPong<float> xhist, rhist;           // [2][C][HX]; [2][HR]: flipped together
  DevBuf<unsigned> stat_min;              // [kLimSlots]
  DevBuf<unsigned long long> stat_count;  // [kLimSlots]
  HostRows host;                          // the host form's rows and the PCM form's: [C][max_samples] each
  DevBuf<float> d_gain;                   // [max_samples]
  PcmLevels levels;                       // the PCM form's

  // a launch's sample indices are ints
  static constexpr size_t kMaxLaunch = (size_t)1 << 24;

  void zero_stats() {
    EARHIP_HIP(hipMemsetAsync(stat_min.p, 0, sizeof(unsigned) * stat_min.n, ctx->stream));
    EARHIP_HIP(hipMemsetAsync(stat_count.p, 0, sizeof(unsigned long long) * stat_count.n, ctx->stream));
  }
  void zero() override {
    xhist.zero(ctx->stream);
    rhist.rewind();
    for (float *half : {rhist.in(), rhist.out()})  // r = 1 before the clock starts
      EARHIP_HIP(hipMemcpyAsync(half, ones.p, sizeof(float) * (size_t)sh.r_hist(), hipMemcpyDeviceToDevice, ctx->stream));
    zero_stats();
    levels.zero(ctx->stream);
    clock = 0;
  }

  void launch(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride, float *gain) {
    LimArgs a;
    a.in = in, a.in_stride = in_stride, a.out = out, a.out_stride = out_stride, a.gain = gain;
    a.n = (unsigned)n, a.C = n_in, a.c = c;
    a.L = sh.L, a.M = sh.M, a.K = sh.K, a.D = sh.D, a.HX = sh.x_hist(), a.HR = sh.r_hist(), a.phases = sh.phases, a.taps = sh.taps;
    a.xhist_in = xhist.in(), a.xhist_out = xhist.out();
    a.rhist_in = rhist.in(), a.rhist_out = rhist.out();
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
    xhist.flip(), rhist.flip();
  }

  // gain: a row [nsamples] for the gain, or NULL
  void feed_gain(size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride, float *gain) {
    for_each_launch(nsamples, std::min(kMaxLaunch, r.n), [&](size_t at, size_t n, size_t) {
      launch(n, in + at, in_stride, out + at, out_stride, gain ? gain + at : nullptr);
      return n;
    });
  }
  void feed(size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride) override {
    feed_gain(nsamples, in, in_stride, out, out_stride, nullptr);
  }
};

template <>
BusStage *earhip::as_stage<earhip_limiter>(earhip_limiter *h) {
  return h;
}

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
    lim->n_in = lim->n_out = cfg->n_channels, lim->c = cfg->ceiling, lim->detect = cfg->detect;
    lim->sh = limiter_shape(cfg->lookahead, cfg->hold, cfg->detect, table.phases, table.taps);
    lim->room = cfg->max_samples;
    std::memcpy(lim->h, table.h, sizeof(lim->h));
    const size_t C = (size_t)cfg->n_channels, HR = (size_t)lim->sh.r_hist();
    lim->table.upload(table.v);
    lim->xhist.alloc(C * (size_t)lim->sh.x_hist());
    lim->rhist.alloc(HR);
    lim->ones.upload(std::vector<float>(HR, 1.0f));
    lim->r.alloc(std::min(cfg->max_samples, earhip_limiter::kMaxLaunch));
    lim->stat_min.alloc(kLimSlots);
    lim->stat_count.alloc(kLimSlots);
    lim->host.alloc(C * cfg->max_samples, C * cfg->max_samples);
    lim->d_gain.alloc(cfg->max_samples);
    lim->levels.reserve(cfg->n_channels, ctx->stream);
    stage_ready(lim, out);
  });
}

int earhip_limiter_destroy(earhip_limiter *lim) { return stage_destroy(lim); }
int earhip_limiter_reset(earhip_limiter *lim) { return stage_reset(lim); }

int earhip_limiter_latency(const earhip_limiter *lim, int *samples) {
  return guarded([&] {
    require(lim != nullptr && samples != nullptr, "limiter and samples must not be NULL");
    *samples = lim->sh.latency();
  });
}

int earhip_limiter_process_device(earhip_limiter *lim, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                                  size_t out_stride, float *gain_dev) {
  return guarded([&] {
    if (!stage_admits(lim, nsamples)) return;
    check_device_rows(earhip_limiter::words, nsamples, in_dev, in_stride, nsamples, out_dev, out_stride);
    lim->ctx->use();
    lim->feed_gain(nsamples, in_dev, in_stride, out_dev, out_stride, gain_dev);
  });
}

int earhip_limiter_process(earhip_limiter *lim, size_t nsamples, const float *const *in, float *const *out, float *gain) {
  return guarded([&] {
    if (!stage_admits(lim, nsamples)) return;
    const size_t n = nsamples;
    check_host_rows(earhip_limiter::words, n, in, lim->n_in, reads_every_row, n, out, lim->n_out);
    hipStream_t stream = lim->ctx->stream;
    lim->ctx->use();
    lim->host.to_device(in, lim->n_in, n, stream, reads_every_row);
    lim->feed_gain(n, lim->host.d_in.p, n, lim->host.d_out.p, n, gain ? lim->d_gain.p : nullptr);
    if (gain) EARHIP_HIP(hipMemcpyAsync(gain, lim->d_gain.p, sizeof(float) * n, hipMemcpyDeviceToHost, stream));
    lim->host.from_device(out, lim->n_out, n, stream);
  });
}

int earhip_limiter_process_pcm_device(earhip_limiter *lim, size_t nsamples, const float *in_dev, size_t in_stride, void *out_dev,
                                      size_t out_frame_bytes, size_t out_first_byte, const earhip_pcm_out *out) {
  return guarded([&] {
    require(lim != nullptr, "limiter must not be NULL");
    check_pcm_out_frame(lim->n_in, check_pcm_out(out), out_dev, out_frame_bytes, out_first_byte, "n_channels");
    lim->check_room(nsamples);
    if (nsamples == 0) return;
    require(in_dev != nullptr, "in_dev must not be NULL");
    require(in_stride >= nsamples, "stride too small");
    earhip_ctx *ctx = lim->ctx;
    ctx->use();
    const int64_t t0 = (int64_t)lim->clock;
    lim->feed(nsamples, in_dev, in_stride, lim->host.d_out.p, nsamples);
    launch_rows_to_pcm(*out, lim->host.d_out.p, nsamples, lim->n_in, nsamples, static_cast<unsigned char *>(out_dev), out_frame_bytes,
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
    lim->levels.read(lim->n_in, peak, clipped);
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
