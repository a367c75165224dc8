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
          : n_in_(n_in), n_out_(n_out), block_size_(block_size) {
        if (taps.size() != n_in * n_out * n_taps) throw invalid_argument("taps must be n_out x n_in x n_taps numbers");
        earhip_firmix_config cfg;
        cfg.n_in = (int)n_in, cfg.n_out = (int)n_out, cfg.block_size = (int)block_size, cfg.n_taps = (int)n_taps;
        cfg.taps = taps.data();
        cfg.max_blocks = (int)max_blocks;
        check(earhip_firmix_create(ctx.get(), &cfg, &h_));
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
      /// state and clock to zero
      void reset() { check(earhip_firmix_reset(h_)); }
      size_t num_inputs() const { return n_in_; }
      size_t num_outputs() const { return n_out_; }
      size_t block_size() const { return block_size_; }
      size_t partitions() const { return (size_t)info(3); }
      /// pairs (output, input) with a tap that is not zero
      size_t nonzero_pairs() const { return (size_t)info(4); }
      earhip_firmix *get() const { return h_; }

     private:
      int info(int i) const {
        int v[5];
        check(earhip_firmix_info(h_, v));
        return v[i];
      }
      size_t n_in_, n_out_, block_size_;
      earhip_firmix *h_ = nullptr;
    };
  }  // namespace hip
}  // namespace ear
