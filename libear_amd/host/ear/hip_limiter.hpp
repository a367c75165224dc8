// ear/hip_limiter.hpp — a look-ahead true-peak limiter on the device, one gain for all channels: the C++ face of group N of the
// C ABI (include/earhip.h, where the operation is specified).  libear has no such object, so there is no libear header this
// one mirrors; it follows the conventions of the mirror classes (exceptions for status codes, a context argument that defaults
// to the process-wide one), as hip_loudness.hpp and hip_firmix.hpp do.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hip.hpp"

namespace ear {
  namespace hip {
    /// Every output sample stays under `ceiling` (times 1 + 2^-22), the output delayed by latency() samples.  Feed it rows
    /// yourself, or attach it to a renderer (ear::dsp::ObjectsRenderer::attach_limiter) and it limits every process call's
    /// output into a sink of yours; detach it before it dies.
    class Limiter {
     public:
      enum class Detect { SamplePeak = 0, TruePeak = 1 };
      /// n_channels in [1, 64], ceiling finite and > 0, lookahead in [8, 1024], hold in [0, 8192] samples, max_samples (the
      /// longest process call) >= 1; true peak with BS.1770-4's table at 44100 and 48000 Hz only: else ear::invalid_argument.
      Limiter(size_t n_channels, float ceiling, size_t lookahead = 64, size_t hold = 480, size_t max_samples = 48000,
              int sample_rate = 48000, Detect detect = Detect::TruePeak, Context &ctx = default_context())
          : n_channels_(n_channels) {
        create(ceiling, lookahead, hold, max_samples, sample_rate, detect, nullptr, ctx);
      }
      /// true peak on the caller's table [phases][taps] (phases in [1, 8], taps in [1, 64]), at any rate
      Limiter(size_t n_channels, float ceiling, size_t lookahead, size_t hold, size_t max_samples, int sample_rate, size_t phases,
              size_t taps, const std::vector<double> &table, Context &ctx = default_context())
          : n_channels_(n_channels) {
        if (table.size() != phases * taps || table.empty()) throw invalid_argument("the true-peak table must be phases x taps numbers");
        earhip_true_peak tp;
        tp.phases = (int)phases, tp.taps = (int)taps, tp.coeffs = table.data();
        create(ceiling, lookahead, hold, max_samples, sample_rate, Detect::TruePeak, &tp, ctx);
      }
      ~Limiter() { earhip_limiter_destroy(h_); }
      Limiter(const Limiter &) = delete;
      Limiter &operator=(const Limiter &) = delete;

      /// host rows in[n_channels], out[n_channels] of nsamples each (any nsamples <= max_samples); gain: [nsamples] or nullptr
      void process(size_t nsamples, const float *const *in, float *const *out, float *gain = nullptr) {
        check(earhip_limiter_process(h_, nsamples, in, out, gain));
      }
      void process(size_t nsamples, float **in, float **out, float *gain = nullptr) {
        check(earhip_limiter_process(h_, nsamples, in, out, gain));
      }
      /// planar rows in device memory; enqueues on the context's stream
      void process_device(size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev, size_t out_stride,
                          float *gain_dev = nullptr) {
        check(earhip_limiter_process_device(h_, nsamples, in_dev, in_stride, out_dev, out_stride, gain_dev));
      }
      /// the limited rows as interleaved PCM frames in device memory (the rules of ObjectsRenderer's PCM-out forms)
      void process_pcm_device(size_t nsamples, const float *in_dev, size_t in_stride, void *out_dev, size_t out_frame_bytes,
                              size_t out_first_byte, const earhip_pcm_out &out) {
        check(earhip_limiter_process_pcm_device(h_, nsamples, in_dev, in_stride, out_dev, out_frame_bytes, out_first_byte, &out));
      }
      /// D + L: how many samples the output lags the input
      size_t latency() const {
        int v = 0;
        check(earhip_limiter_latency(h_, &v));
        return (size_t)v;
      }
      struct Stats {
        float min_gain;            ///< the smallest gain so far (1: never limited)
        uint64_t limited_samples;  ///< samples with a gain below 1
      };
      Stats stats(bool reset = false) {
        Stats s{1.0f, 0};
        check(earhip_limiter_stats(h_, &s.min_gain, &s.limited_samples, reset ? 1 : 0));
        return s;
      }
      /// peak and clipped samples per channel of what went through process_pcm_device
      void output_levels(std::vector<float> &peak, std::vector<uint64_t> &clipped, bool reset = false) {
        peak.assign(n_channels_, 0.0f), clipped.assign(n_channels_, 0);
        check(earhip_limiter_output_levels(h_, peak.data(), clipped.data(), reset ? 1 : 0));
      }
      /// history, clock, stats and levels to zero
      void reset() { check(earhip_limiter_reset(h_)); }
      size_t num_channels() const { return n_channels_; }
      earhip_limiter *get() const { return h_; }

     private:
      void create(float ceiling, size_t lookahead, size_t hold, size_t max_samples, int sample_rate, Detect detect,
                  const earhip_true_peak *tp, Context &ctx) {
        if (n_channels_ > 64 || lookahead > 1024 || hold > 8192) throw invalid_argument("limiter: n_channels, lookahead or hold out of range");
        earhip_limiter_config cfg;
        cfg.n_channels = (int)n_channels_, cfg.sample_rate = sample_rate, cfg.ceiling = ceiling;
        cfg.lookahead = (int)lookahead, cfg.hold = (int)hold, cfg.detect = (int)detect;
        cfg.tp = tp;
        cfg.max_samples = max_samples;
        check(earhip_limiter_create(ctx.get(), &cfg, &h_));
      }
      size_t n_channels_;
      earhip_limiter *h_ = nullptr;
    };
  }  // namespace hip
}  // namespace ear
