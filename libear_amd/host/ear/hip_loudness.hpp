// ear/hip_loudness.hpp — programme loudness (ITU-R BS.1770-4) measured on the device: the C++ face of group L of the C ABI
// (include/earhip.h, where the measurement is specified).  libear has no meter, so there is no libear header this one mirrors;
// it follows the conventions of the mirror classes (exceptions for status codes, a context argument that defaults to the
// process-wide one).
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "hip.hpp"

namespace ear {
  namespace hip {
    /// integrated, maximum momentary and maximum short-term loudness in LKFS; -infinity where there is nothing to measure
    struct Loudness {
      double integrated, max_momentary, max_short_term;
    };

    /// BS.1770-4's channel weights of a BS.2051 layout (LFE channels 0); throws ear::unknown_layout
    inline std::vector<double> loudness_layout_weights(const std::string &layout) {
      int n = 0;
      check(earhip_layout_num_channels(layout.c_str(), &n));
      std::vector<double> w((size_t)n);
      check(earhip_loudness_layout_weights(layout.c_str(), w.data()));
      return w;
    }

    /// The gating alone, on the calling thread: energy [n_steps][weights.size()] (the columns of several meters side by side —
    /// the ranks of a multi-GPU render each meter the channels they own).
    inline Loudness loudness_gate(const std::vector<double> &energy, const std::vector<double> &weights) {
      if (weights.empty() || energy.size() % weights.size() != 0) throw invalid_argument("energy is not [steps][channels]");
      Loudness l;
      check(earhip_loudness_gate(energy.size() / weights.size(), (int)weights.size(), energy.data(), weights.data(), &l.integrated,
                                 &l.max_momentary, &l.max_short_term));
      return l;
    }

    /// K-weighted 100 ms step energies kept on the device.  Feed it rows yourself, or attach it to a renderer
    /// (ear::dsp::ObjectsRenderer::attach_loudness) and it meters every process call's output; detach it before it dies.
    class LoudnessMeter {
     public:
      /// max_steps: capacity of the step store (100 ms each; the default holds an hour).  coeffs: 10 numbers, b0 b1 b2 a1 a2 of
      /// the two stages, for rates other than 48000; empty = BS.1770-4's at 48 kHz.
      explicit LoudnessMeter(size_t n_channels, int sample_rate = 48000, size_t max_steps = 36000,
                             const std::vector<double> &coeffs = std::vector<double>(), Context &ctx = default_context())
          : n_channels_(n_channels) {
        if (!coeffs.empty() && coeffs.size() != 10) throw invalid_argument("coeffs must be 2 x 5 numbers");
        check(earhip_loudness_create(ctx.get(), (int)n_channels, sample_rate, coeffs.empty() ? nullptr : coeffs.data(), max_steps, &h_));
      }
      ~LoudnessMeter() { earhip_loudness_destroy(h_); }
      LoudnessMeter(const LoudnessMeter &) = delete;
      LoudnessMeter &operator=(const LoudnessMeter &) = delete;

      /// host rows, any number of samples
      void process(const float *const *rows, size_t nsamples) { check(earhip_loudness_process(h_, nsamples, rows)); }
      /// planar rows in device memory; enqueues on the context's stream
      void process_device(const float *rows_dev, size_t nsamples, size_t stride) {
        check(earhip_loudness_process_device(h_, nsamples, rows_dev, stride));
      }
      size_t num_steps() const {
        size_t n = 0;
        check(earhip_loudness_num_steps(h_, &n));
        return n;
      }
      /// [n][n_channels] of the finished steps [first, first + n)
      std::vector<double> steps(size_t first, size_t n) const {
        std::vector<double> e(n * n_channels_);
        check(earhip_loudness_steps(h_, first, n, e.data()));
        return e;
      }
      std::vector<double> steps() const { return steps(0, num_steps()); }
      Loudness result(const std::vector<double> &weights) const {
        if (weights.size() != n_channels_) throw invalid_argument("one weight per channel");
        Loudness l;
        check(earhip_loudness_result(h_, weights.data(), &l.integrated, &l.max_momentary, &l.max_short_term));
        return l;
      }
      void reset() { check(earhip_loudness_reset(h_)); }
      size_t num_channels() const { return n_channels_; }
      earhip_loudness *get() const { return h_; }

     private:
      size_t n_channels_;
      earhip_loudness *h_ = nullptr;
    };
  }  // namespace hip
}  // namespace ear
