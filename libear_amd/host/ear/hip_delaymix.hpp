// ear/hip_delaymix.hpp — a matrix of delayed short FIRs on the device (time alignment of loudspeakers, a subwoofer against its
// mains, a lip-sync offset on the bus): the C++ face of group S of the C ABI (include/earhip.h, where the operation is
// specified).  libear's DelayBuffer delays every channel by one amount and has no such object, so there is no libear header this
// one mirrors; it follows the conventions of the mirror classes (exceptions for status codes, a context argument that defaults
// to the process-wide one), as hip_iir.hpp and hip_src.hpp do.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "hip.hpp"

namespace ear {
  namespace hip {
    /// out_k[n] = the chain of fused multiply-adds, over the routes into k in list order and each route's taps in order, of
    /// taps[j] * in[n - delay - j], in float32: the same samples give the same bits however the stream is cut into calls.  Feed
    /// it rows: host rows, or rows in device memory — those a renderer's process_device just wrote, for one; on the same
    /// context the matrix's kernels follow the renderer's on the stream.
    class DelayMatrix {
     public:
      struct Route {
        size_t in, out;
        size_t delay;             ///< whole samples, at most 65536
        std::vector<float> taps;  ///< 1 to 32; one tap: a gain
      };
      /// a delay of `delay` samples as (whole delay, taps): n_taps = 1 rounds to the nearest sample, an even n_taps in [2, 32]
      /// is a Kaiser-windowed sinc centred on the fraction with unit DC gain (delay >= n_taps / 2 - 1); a pure host function
      static std::pair<size_t, std::vector<float>> fractional(double delay, size_t n_taps = 16, double beta = 8.0) {
        if (n_taps < 1 || n_taps > 32) throw invalid_argument("delaymix: n_taps out of range");
        int whole = 0;
        std::vector<double> h(n_taps);
        check(earhip_delaymix_fractional(delay, (int)n_taps, beta, &whole, h.data()));
        return std::make_pair((size_t)whole, std::vector<float>(h.begin(), h.end()));
      }
      /// loudspeakers at distances_m brought to the farthest one's arrival time and level: (delay in samples, gain) each; a
      /// pure host function
      static std::vector<std::pair<double, double>> align(const std::vector<double> &distances_m, double sample_rate,
                                                          double speed_of_sound = 343.0) {
        std::vector<double> delay(distances_m.size() + 1), gain(distances_m.size() + 1);
        check(earhip_delaymix_align((int)distances_m.size(), distances_m.data(), sample_rate, speed_of_sound, delay.data(), gain.data()));
        std::vector<std::pair<double, double>> out;
        for (size_t c = 0; c < distances_m.size(); c++) out.push_back(std::make_pair(delay[c], gain[c]));
        return out;
      }
      /// the diagonal route list of align(): channel c to channel c, its delay as fractional(delay, n_taps, beta), the taps
      /// times its gain
      static std::vector<Route> alignment(const std::vector<double> &distances_m, double sample_rate, size_t n_taps = 16,
                                          double beta = 8.0, double speed_of_sound = 343.0) {
        const std::vector<std::pair<double, double>> dg = align(distances_m, sample_rate, speed_of_sound);
        std::vector<Route> routes;
        for (size_t c = 0; c < dg.size(); c++) {
          // (a delay too short for the taps' centre is pushed back by it on every channel alike)
          std::pair<size_t, std::vector<float>> f = fractional(dg[c].first + (n_taps > 1 ? (double)(n_taps / 2 - 1) : 0.0), n_taps, beta);
          for (float &v : f.second) v = (float)((double)v * dg[c].second);
          routes.push_back(Route{c, c, f.first, f.second});
        }
        return routes;
      }
      /// n_in, n_out in [1, 64], 1 to 512 routes with 1 to 32 finite taps and a delay of at most 65536, max_samples (the longest
      /// process call) >= 1: else ear::invalid_argument
      DelayMatrix(size_t n_in, size_t n_out, const std::vector<Route> &routes, size_t max_samples = 48000, Context &ctx = default_context())
          : n_in_(n_in), n_out_(n_out) {
        if (n_in > 64 || n_out > 64 || routes.size() > 512) throw invalid_argument("delaymix: n_in, n_out or the number of routes out of range");
        std::vector<earhip_delaymix_route> list(routes.size());
        for (size_t r = 0; r < routes.size(); r++) {
          if (routes[r].in >= n_in || routes[r].out >= n_out || routes[r].delay > 65536 || routes[r].taps.size() > 32)
            throw invalid_argument("delaymix: a route's in, out, delay or number of taps out of range");
          list[r].in = (int)routes[r].in, list[r].out = (int)routes[r].out, list[r].delay = (int)routes[r].delay;
          list[r].n_taps = (int)routes[r].taps.size();
          for (size_t j = 0; j < 32; j++) list[r].taps[j] = j < routes[r].taps.size() ? routes[r].taps[j] : 0.0f;
        }
        earhip_delaymix_config cfg;
        cfg.n_in = (int)n_in, cfg.n_out = (int)n_out, cfg.n_routes = (int)list.size(), cfg.routes = list.data();
        cfg.max_samples = max_samples;
        check(earhip_delaymix_create(ctx.get(), &cfg, &h_));
      }
      ~DelayMatrix() { earhip_delaymix_destroy(h_); }
      DelayMatrix(const DelayMatrix &) = delete;
      DelayMatrix &operator=(const DelayMatrix &) = delete;

      /// host rows in[n_in], out[n_out] of nsamples each (any nsamples <= max_samples)
      void process(size_t nsamples, const float *const *in, float *const *out) { check(earhip_delaymix_process(h_, nsamples, in, out)); }
      void process(size_t nsamples, float **in, float **out) { check(earhip_delaymix_process(h_, nsamples, in, out)); }
      /// planar rows in device memory; enqueues on the context's stream
      void process_device(size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev, size_t out_stride) {
        check(earhip_delaymix_process_device(h_, nsamples, in_dev, in_stride, out_dev, out_stride));
      }
      earhip_delaymix_properties info() const {
        earhip_delaymix_properties v;
        check(earhip_delaymix_info(h_, &v));
        return v;
      }
      /// histories and clock to zero
      void reset() { check(earhip_delaymix_reset(h_)); }
      size_t num_inputs() const { return n_in_; }
      size_t num_outputs() const { return n_out_; }
      earhip_delaymix *get() const { return h_; }

     private:
      size_t n_in_, n_out_;
      earhip_delaymix *h_ = nullptr;
    };
  }  // namespace hip
}  // namespace ear
