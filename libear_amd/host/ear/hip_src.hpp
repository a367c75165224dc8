// ear/hip_src.hpp — a polyphase sample-rate converter on the device (44.1 or 96 kHz assets to a 48 kHz bed, a 48 kHz render
// delivered at 44.1 kHz): the C++ face of group P of the C ABI (include/earhip.h, where the operation is specified).  libear has
// no such object, so there is no libear header this one mirrors; it follows the conventions of the mirror classes (exceptions
// for status codes, a context argument that defaults to the process-wide one), as hip_iir.hpp and hip_limiter.hpp do.
#pragma once
#include <cstddef>
#include <vector>

#include "hip.hpp"

namespace ear {
  namespace hip {
    /// y = upfirdn(taps, x, up, down) per channel in float32: output j is one chain of taps_per_phase fused multiply-adds over
    /// inputs floor(j down / up) and before, so the same samples give the same bits however the stream is cut into calls.  Feed
    /// it rows: host rows, or rows in device memory — those a renderer's process_device just wrote, for one; on the same context
    /// the converter's kernels follow the renderer's on the stream.
    class SampleRateConverter {
     public:
      /// the prototype of a rate change by up / down: a Kaiser-windowed sinc of up * taps_per_phase taps with its cutoff at
      /// cutoff / max(up, down) of the prototype's Nyquist, unit DC gain, times up; a pure host function
      static std::vector<double> design(size_t up, size_t down, size_t taps_per_phase, double beta = 10.0, double cutoff = 1.0) {
        if (up < 1 || up > 1024 || down < 1 || down > 1024 || taps_per_phase < 1 || taps_per_phase > 256)
          throw invalid_argument("src: up, down or taps_per_phase out of range");
        std::vector<double> h(up * taps_per_phase);
        check(earhip_src_design((int)up, (int)down, (int)taps_per_phase, beta, cutoff, h.data()));
        return h;
      }
      /// channels in [1, 64], up and down in [1, 1024] without a common factor, taps_per_phase in [1, 256] with
      /// up * taps_per_phase <= 32768 = taps.size(), finite taps, max_samples (the longest process call, in inputs) >= 1: else
      /// ear::invalid_argument
      SampleRateConverter(size_t channels, size_t up, size_t down, size_t taps_per_phase, const std::vector<double> &taps,
                          size_t max_samples = 48000, Context &ctx = default_context())
          : channels_(channels) {
        if (channels > 64 || up > 1024 || down > 1024 || taps_per_phase > 256) throw invalid_argument("src: channels, up, down or taps_per_phase out of range");
        if (taps.size() != up * taps_per_phase) throw invalid_argument("src: taps must hold up * taps_per_phase values");
        earhip_src_config cfg;
        cfg.channels = (int)channels, cfg.up = (int)up, cfg.down = (int)down, cfg.taps_per_phase = (int)taps_per_phase;
        cfg.taps = taps.data(), cfg.max_samples = max_samples;
        check(earhip_src_create(ctx.get(), &cfg, &h_));
      }
      ~SampleRateConverter() { earhip_src_destroy(h_); }
      SampleRateConverter(const SampleRateConverter &) = delete;
      SampleRateConverter &operator=(const SampleRateConverter &) = delete;

      /// the outputs a call of nsamples inputs would produce now
      size_t next_out(size_t nsamples) const {
        size_t n = 0;
        check(earhip_src_next_out(h_, nsamples, &n));
        return n;
      }
      /// host rows in[channels] of nsamples, out[channels] with room for out_capacity; returns the outputs written per row
      size_t process(size_t nsamples, const float *const *in, float *const *out, size_t out_capacity) {
        size_t n = 0;
        check(earhip_src_process(h_, nsamples, in, out, out_capacity, &n));
        return n;
      }
      size_t process(size_t nsamples, float **in, float **out, size_t out_capacity) {
        size_t n = 0;
        check(earhip_src_process(h_, nsamples, in, out, out_capacity, &n));
        return n;
      }
      /// planar rows in device memory; enqueues on the context's stream; returns the outputs written per row
      size_t process_device(size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev, size_t out_stride, size_t out_capacity) {
        size_t n = 0;
        check(earhip_src_process_device(h_, nsamples, in_dev, in_stride, out_dev, out_stride, out_capacity, &n));
        return n;
      }
      earhip_src_properties info() const {
        earhip_src_properties v;
        check(earhip_src_info(h_, &v));
        return v;
      }
      /// the most outputs of one call: ceil(max_samples up / down)
      size_t max_out() const { return info().max_out; }
      /// histories to zero, clock to 0
      void reset() { check(earhip_src_reset(h_)); }
      size_t num_channels() const { return channels_; }
      earhip_src *get() const { return h_; }

     private:
      size_t channels_;
      earhip_src *h_ = nullptr;
    };
  }  // namespace hip
}  // namespace ear
