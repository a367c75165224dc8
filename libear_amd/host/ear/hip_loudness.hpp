// ear/hip_loudness.hpp — programme loudness (ITU-R BS.1770-4), true peak (its annex 2) and loudness range (EBU Tech 3342)
// measured on the device: the C++ face of group L of the C ABI
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

    /// loudness range in LU and the two percentiles it lies between in LKFS; 0 and -infinity where no window survives the gates
    struct LoudnessRange {
      double lra, low, high;
    };
    /// true and sample peak per channel, linear
    struct Peaks {
      std::vector<float> true_peak, sample_peak;
    };
    /// Whether and how a LoudnessMeter measures true peak: off (the default), BS.1770-4's 4 x 12 table (44100 and 48000 Hz), or
    /// a table of the caller's, [phases][taps].
    struct TruePeak {
      bool on = false;
      int phases = 0, taps = 0;
      std::vector<double> coeffs;
      TruePeak() = default;
      static TruePeak bs1770() {
        TruePeak t;
        t.on = true;
        return t;
      }
      static TruePeak table(int phases, int taps, const std::vector<double> &coeffs) {
        TruePeak t;
        t.on = true, t.phases = phases, t.taps = taps, t.coeffs = coeffs;
        return t;
      }
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

    /// EBU Tech 3342 over step energies [n_steps][weights.size()], on the calling thread (columns joined as for loudness_gate)
    inline LoudnessRange loudness_range(const std::vector<double> &energy, const std::vector<double> &weights) {
      if (weights.empty() || energy.size() % weights.size() != 0) throw invalid_argument("energy is not [steps][channels]");
      LoudnessRange r;
      check(earhip_loudness_range(energy.size() / weights.size(), (int)weights.size(), energy.data(), weights.data(), &r.lra, &r.low,
                                  &r.high));
      return r;
    }

    /// K-weighted 100 ms step energies kept on the device.  Feed it rows yourself, or attach it to a renderer
    /// (ear::dsp::ObjectsRenderer::attach_loudness) and it meters every process call's output; detach it before it dies.
    class LoudnessMeter {
     public:
      /// max_steps: capacity of the step store (100 ms each; the default holds an hour).  coeffs: 10 numbers, b0 b1 b2 a1 a2 of
      /// the two stages, for rates other than 48000; empty = BS.1770-4's at 48 kHz.
      /// true_peak: off unless asked for (TruePeak::bs1770() or TruePeak::table(...)).
      explicit LoudnessMeter(size_t n_channels, int sample_rate = 48000, size_t max_steps = 36000,
                             const std::vector<double> &coeffs = std::vector<double>(), Context &ctx = default_context(),
                             const TruePeak &true_peak = TruePeak())
          : n_channels_(n_channels) {
        if (!coeffs.empty() && coeffs.size() != 10) throw invalid_argument("coeffs must be 2 x 5 numbers");
        const double *k = coeffs.empty() ? nullptr : coeffs.data();
        if (!true_peak.on) {
          check(earhip_loudness_create(ctx.get(), (int)n_channels, sample_rate, k, max_steps, &h_));
          return;
        }
        if (!true_peak.coeffs.empty() &&
            (true_peak.phases < 1 || true_peak.taps < 1 ||
             true_peak.coeffs.size() != (size_t)true_peak.phases * (size_t)true_peak.taps))
          throw invalid_argument("the true-peak table must be phases x taps numbers");
        earhip_true_peak tp;
        tp.phases = true_peak.phases, tp.taps = true_peak.taps;
        tp.coeffs = true_peak.coeffs.empty() ? nullptr : true_peak.coeffs.data();
        check(earhip_loudness_create_tp(ctx.get(), (int)n_channels, sample_rate, k, max_steps, &tp, &h_));
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
      /// so far, the unfinished step included (throws on a meter made without true peak, as step_peaks does)
      Peaks peaks() const {
        Peaks p;
        p.true_peak.resize(n_channels_), p.sample_peak.resize(n_channels_);
        check(earhip_loudness_peaks(h_, p.true_peak.data(), p.sample_peak.data()));
        return p;
      }
      /// [n][n_channels] each, of the finished steps [first, first + n)
      Peaks step_peaks(size_t first, size_t n) const {
        Peaks p;
        p.true_peak.resize(n * n_channels_), p.sample_peak.resize(n * n_channels_);
        check(earhip_loudness_step_peaks(h_, first, n, p.true_peak.data(), p.sample_peak.data()));
        return p;
      }
      Peaks step_peaks() const { return step_peaks(0, num_steps()); }
      LoudnessRange range(const std::vector<double> &weights) const {
        if (weights.size() != n_channels_) throw invalid_argument("one weight per channel");
        LoudnessRange r;
        check(earhip_loudness_result_range(h_, weights.data(), &r.lra, &r.low, &r.high));
        return r;
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
