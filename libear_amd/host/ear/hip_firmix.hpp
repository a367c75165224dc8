// ear/hip_firmix.hpp — a matrix of FIR filters from n_in rows to n_out rows on the device (binaural monitoring of a
// loudspeaker bus, per-loudspeaker EQ, a filtered fold-down): the C++ face of group M of the C ABI (include/earhip.h, where the
// operation is specified).  libear has no such object — a libear user writes one BlockConvolver per pair — so there is no
// libear header this one mirrors; it follows the conventions of the mirror classes (exceptions for status codes, a context
// argument that defaults to the process-wide one).
#pragma once
#include <cstddef>
#include <vector>

#include "hip.hpp"

namespace ear {
  namespace hip {
    /// y[k][n] = sum over c, j of taps[k][c][j] x[c][n - j], partitioned at block_size.  Pairs whose taps are all zero cost
    /// nothing and their input channels are never read.  Feed it rows yourself, or attach it to a renderer
    /// (ear::dsp::ObjectsRenderer::attach_fir_matrix) and it filters every process call's output into a sink of yours; detach
    /// it before it dies.
    class FirMatrix {
     public:
      /// taps: [n_out][n_in][n_taps], every one finite.  n_in in [1, 64], n_out in [1, 64], block_size a power of two in
      /// [64, 4096], n_taps in [1, 64 * block_size], max_blocks (the longest process call) >= 1: else ear::invalid_argument.
      FirMatrix(size_t n_in, size_t n_out, size_t block_size, size_t n_taps, const std::vector<float> &taps, size_t max_blocks = 1,
                Context &ctx = default_context())
          : n_in_(n_in), n_out_(n_out), block_size_(block_size), n_taps_(n_taps) {
        if (taps.size() != n_in * n_out * n_taps) throw invalid_argument("taps must be n_out x n_in x n_taps numbers");
        earhip_firmix_config cfg;
        cfg.n_in = (int)n_in, cfg.n_out = (int)n_out, cfg.block_size = (int)block_size, cfg.n_taps = (int)n_taps;
        cfg.taps = taps.data();
        cfg.max_blocks = (int)max_blocks;
        check(earhip_firmix_create(ctx.get(), &cfg, &h_));
      }
      /// The same with room for n_sets filter sets of this shape (n_sets in [1, 4096]): `taps` is set 0 and current, the
      /// others are unloaded until load_set.  Every input channel is read (include/earhip.h, FILTER SETS).
      FirMatrix(size_t n_in, size_t n_out, size_t block_size, size_t n_taps, const std::vector<float> &taps, size_t max_blocks,
                size_t n_sets, Context &ctx = default_context())
          : n_in_(n_in), n_out_(n_out), block_size_(block_size), n_taps_(n_taps) {
        if (taps.size() != n_in * n_out * n_taps) throw invalid_argument("taps must be n_out x n_in x n_taps numbers");
        if (n_sets > 4096) throw invalid_argument("n_sets must be in [1, 4096]");
        earhip_firmix_config cfg;
        cfg.n_in = (int)n_in, cfg.n_out = (int)n_out, cfg.block_size = (int)block_size, cfg.n_taps = (int)n_taps;
        cfg.taps = taps.data();
        cfg.max_blocks = (int)max_blocks;
        check(earhip_firmix_create_sets(ctx.get(), &cfg, (int)n_sets, &h_));
      }
      ~FirMatrix() { earhip_firmix_destroy(h_); }
      FirMatrix(const FirMatrix &) = delete;
      FirMatrix &operator=(const FirMatrix &) = delete;

      /// host rows in[n_in], out[n_out] of nblocks * block_size samples each
      void process(size_t nblocks, const float *const *in, float *const *out) { check(earhip_firmix_process(h_, nblocks, in, out)); }
      /// planar rows in device memory; enqueues on the context's stream
      void process_device(size_t nblocks, const float *in_dev, size_t in_stride, float *out_dev, size_t out_stride) {
        check(earhip_firmix_process_device(h_, nblocks, in_dev, in_stride, out_dev, out_stride));
      }
      /// state and clock to zero; a fade ends at once, its target current
      void reset() { check(earhip_firmix_reset(h_)); }

      /// Filter sets (a matrix made with n_sets).  taps [n_out][n_in][n_taps] on the host become set `set`, which must be
      /// neither current nor being faded from; not a call for the audio thread.
      void load_set(size_t set, const std::vector<float> &taps) {
        if (taps.size() != n_in_ * n_out_ * n_taps_) throw invalid_argument("taps must be n_out x n_in x n_taps numbers");
        check(earhip_firmix_load_set(h_, (int)set, taps.data()));
      }
      /// the same from device memory: no pair is dropped, nothing is allocated or synchronised
      void load_set_device(size_t set, const float *taps_dev) { check(earhip_firmix_load_set_device(h_, (int)set, taps_dev)); }
      /// From the next block fed, go from the current set to `set` over fade_blocks blocks (0: a hard switch), the fade on
      /// the OUTPUT side: y = (1 - a) y_from + a y_to, a = (q B + n) / (F B) — unlike libear's
      /// BlockConvolver::crossfade_filter, which fades the input.  Host bookkeeping only.
      void select(size_t set, size_t fade_blocks = 0) { check(earhip_firmix_select(h_, (int)set, (int)fade_blocks)); }
      struct State {
        int current, from, done, total;  ///< from = -1: no fade pending or running
      };
      State state() const {
        int v[4];
        check(earhip_firmix_state(h_, v));
        return State{v[0], v[1], v[2], v[3]};
      }
      bool set_loaded(size_t set) const { return set_info(set, 0) != 0; }
      size_t set_nonzero_pairs(size_t set) const { return (size_t)set_info(set, 1); }
      size_t num_inputs() const { return n_in_; }
      size_t num_outputs() const { return n_out_; }
      size_t block_size() const { return block_size_; }
      size_t partitions() const { return (size_t)info(3); }
      /// pairs (output, input) with a tap that is not zero (of the current set)
      size_t nonzero_pairs() const { return (size_t)info(4); }
      earhip_firmix *get() const { return h_; }

     private:
      int info(int i) const {
        int v[5];
        check(earhip_firmix_info(h_, v));
        return v[i];
      }
      int set_info(size_t set, int i) const {
        int v[2];
        check(earhip_firmix_set_info(h_, (int)set, v));
        return v[i];
      }
      size_t n_in_, n_out_, block_size_, n_taps_;
      earhip_firmix *h_ = nullptr;
    };
  }  // namespace hip
}  // namespace ear
