// ear/hip_iir.hpp — a matrix of biquad cascades on the device (crossovers, bass management, EQ): the C++ face of group O of the
// C ABI (include/earhip.h, where the operation is specified).  libear has no such object, so there is no libear header this
// one mirrors; it follows the conventions of the mirror classes (exceptions for status codes, a context argument that defaults
// to the process-wide one), as hip_limiter.hpp and hip_firmix.hpp do.
#pragma once
#include <array>
#include <cstddef>
#include <vector>

#include "hip.hpp"

namespace ear {
  namespace hip {
    /// out_k = the sum over the routes into k, in list order, of gain * (input `in` through the route's sections), float64
    /// inside, rounded to float32 once.  Feed it rows: host rows, or rows in device memory — those a renderer's
    /// process_device just wrote, for one; on the same context the bank's kernels follow the renderer's on the stream.
    class IirBank {
     public:
      using Section = std::array<double, 5>;  ///< b0 b1 b2 a1 a2 (a0 = 1)
      enum class Kind { Lowpass = 0, Highpass = 1, Peaking = 2, LowShelf = 3, HighShelf = 4 };
      struct Route {
        size_t in, out;
        double gain;
        std::vector<Section> sections;  ///< at most 8; none: a pure gain route
      };
      /// one section of the RBJ cookbook; a pure host function.  f0 outside (0, sample_rate / 2) or q <= 0: ear::invalid_argument
      static Section design(Kind kind, double sample_rate, double f0, double q = 0.70710678118654752, double gain_db = 0.0) {
        Section s;
        check(earhip_iir_design((int)kind, sample_rate, f0, q, gain_db, s.data()));
        return s;
      }
      /// a Linkwitz-Riley 4th-order low-pass or high-pass: two Butterworth sections
      static std::vector<Section> linkwitz_riley4(Kind kind, double sample_rate, double f0) {
        return std::vector<Section>(2, design(kind, sample_rate, f0));
      }
      /// n_in, n_out in [1, 64], 1 to 512 routes, every section stable, max_samples (the longest process call) >= 1: else
      /// ear::invalid_argument
      IirBank(size_t n_in, size_t n_out, const std::vector<Route> &routes, size_t max_samples = 48000, Context &ctx = default_context())
          : n_in_(n_in), n_out_(n_out) {
        if (n_in > 64 || n_out > 64 || routes.size() > 512) throw invalid_argument("iir: n_in, n_out or the number of routes out of range");
        std::vector<earhip_iir_route> list(routes.size());
        for (size_t r = 0; r < routes.size(); r++) {
          if (routes[r].in >= n_in || routes[r].out >= n_out || routes[r].sections.size() > 8)
            throw invalid_argument("iir: a route's in, out or number of sections out of range");
          list[r].in = (int)routes[r].in, list[r].out = (int)routes[r].out, list[r].gain = routes[r].gain;
          list[r].n_sections = (int)routes[r].sections.size();
          for (size_t s = 0; s < 8; s++)
            for (size_t i = 0; i < 5; i++) list[r].coeffs[s][i] = s < routes[r].sections.size() ? routes[r].sections[s][i] : 0.0;
        }
        earhip_iir_config cfg;
        cfg.n_in = (int)n_in, cfg.n_out = (int)n_out, cfg.n_routes = (int)list.size(), cfg.routes = list.data();
        cfg.max_samples = max_samples;
        check(earhip_iir_create(ctx.get(), &cfg, &h_));
      }
      ~IirBank() { earhip_iir_destroy(h_); }
      IirBank(const IirBank &) = delete;
      IirBank &operator=(const IirBank &) = delete;

      /// host rows in[n_in], out[n_out] of nsamples each (any nsamples <= max_samples)
      void process(size_t nsamples, const float *const *in, float *const *out) { check(earhip_iir_process(h_, nsamples, in, out)); }
      void process(size_t nsamples, float **in, float **out) { check(earhip_iir_process(h_, nsamples, in, out)); }
      /// planar rows in device memory; enqueues on the context's stream
      void process_device(size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev, size_t out_stride) {
        check(earhip_iir_process_device(h_, nsamples, in_dev, in_stride, out_dev, out_stride));
      }
      /// the chunk length of the decomposition along time
      size_t chunk_length() const {
        int v[6];
        check(earhip_iir_info(h_, v));
        return (size_t)v[0];
      }
      /// states and clock to zero
      void reset() { check(earhip_iir_reset(h_)); }
      size_t num_inputs() const { return n_in_; }
      size_t num_outputs() const { return n_out_; }
      earhip_iir *get() const { return h_; }

     private:
      size_t n_in_, n_out_;
      earhip_iir *h_ = nullptr;
    };
  }  // namespace hip
}  // namespace ear
