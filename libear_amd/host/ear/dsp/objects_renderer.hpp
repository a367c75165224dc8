// ear/dsp/objects_renderer.hpp — the composed Objects render block libear
// documents but does not ship (docs/dsp.rst:40-71): interpolated direct/diffuse
// gains -> buses -> decorrelators + compensation delay -> mix.  This is the
// batched GPU boundary: it has the shape of VariableBlockSizeAdapter's
// ProcessFunc (one block in, one block out) and a multi-block stream variant.
#pragma once
#include <cstdint>
#include <vector>
#include "../hip.hpp"
#include "../hip_firmix.hpp"
#include "../hip_limiter.hpp"
#include "../hip_loudness.hpp"
#include "../hip_timeline.hpp"

namespace ear {
  namespace dsp {
    class ObjectsRenderer {
     public:
      /// decorrelators: designDecorrelators(channel names); empty = direct bus only
      ObjectsRenderer(size_t n_objects, size_t n_out, size_t block_size,
                      const std::vector<std::vector<float>> &decorrelators, int delay,
                      size_t max_blocks = 1, hip::Context &ctx = hip::default_context())
          : n_objects_(n_objects), n_out_(n_out), block_size_(block_size), two_buses_(!decorrelators.empty()) {
        earhip_render_config cfg;
        cfg.n_objects = (int)n_objects;
        cfg.n_out = (int)n_out;
        cfg.block_size = (int)block_size;
        cfg.n_buses = decorrelators.empty() ? 1 : 2;
        std::vector<float> flat;
        cfg.n_taps = 0;
        if (!decorrelators.empty()) {
          if (decorrelators.size() != n_out) throw invalid_argument("one decorrelator per output");
          cfg.n_taps = (int)decorrelators[0].size();
          for (auto &d : decorrelators) {
            if ((int)d.size() != cfg.n_taps) throw invalid_argument("decorrelators differ in length");
            flat.insert(flat.end(), d.begin(), d.end());
          }
        }
        cfg.decorrelators = flat.empty() ? nullptr : flat.data();
        cfg.delay = delay;
        cfg.max_blocks = (int)max_blocks;
        hip::check(earhip_render_create(ctx.get(), &cfg, &h_));
      }
      ~ObjectsRenderer() { earhip_render_destroy(h_); }
      ObjectsRenderer(const ObjectsRenderer &) = delete;
      ObjectsRenderer &operator=(const ObjectsRenderer &) = delete;

      /// Gain curve of one object: same meaning as GainInterpolator::interp_points
      /// of its direct and diffuse LinearInterpVector interpolators.
      void set_object_points(size_t object, const std::vector<int64_t> &times,
                             const std::vector<std::vector<float>> &direct,
                             const std::vector<std::vector<float>> &diffuse) {
        if (direct.size() != times.size()) throw invalid_argument("one direct gain vector per time");
        if (two_buses_ ? diffuse.size() != times.size() : !diffuse.empty())
          throw invalid_argument(two_buses_ ? "one diffuse gain vector per time"
                                            : "diffuse gains given to a renderer without a diffuse bus");
        std::vector<float> d, f;
        for (auto &p : direct) {
          if (p.size() != n_out_) throw invalid_argument("gain vector length != number of outputs");
          d.insert(d.end(), p.begin(), p.end());
        }
        for (auto &p : diffuse) {
          if (p.size() != n_out_) throw invalid_argument("gain vector length != number of outputs");
          f.insert(f.end(), p.begin(), p.end());
        }
        hip::check(earhip_render_set_object_points(h_, (int)object, (int)times.size(), times.data(),
                                                   d.data(), f.empty() ? nullptr : f.data()));
      }
      /// Gain curve of one object from its blocks' timing and one gain vector per block (include/earhip.h group W, where the
      /// rule is specified; ear/hip_timeline.hpp), for the time window [t0, t1): silence outside the blocks, no ramp into the
      /// first, a ramp from the previous block's gains over the whole block or over interpolationLength after a jump.
      void set_object_blocks(size_t object, hip::TimelineMode mode, int64_t start, const std::vector<hip::BlockTiming> &blocks,
                             const std::vector<std::vector<float>> &direct, const std::vector<std::vector<float>> &diffuse,
                             int64_t t0 = hip::kTimelineBegin, int64_t t1 = hip::kTimelineEnd) {
        if (direct.size() != blocks.size()) throw invalid_argument("one direct gain vector per block");
        if (two_buses_ ? diffuse.size() != blocks.size() : !diffuse.empty())
          throw invalid_argument(two_buses_ ? "one diffuse gain vector per block"
                                            : "diffuse gains given to a renderer without a diffuse bus");
        std::vector<float> d, f;
        for (auto &p : direct) {
          if (p.size() != n_out_) throw invalid_argument("gain vector length != number of outputs");
          d.insert(d.end(), p.begin(), p.end());
        }
        for (auto &p : diffuse) {
          if (p.size() != n_out_) throw invalid_argument("gain vector length != number of outputs");
          f.insert(f.end(), p.begin(), p.end());
        }
        const std::vector<earhip_block_timing> c = hip::detail::to_c(blocks);
        hip::check(earhip_render_set_object_blocks(h_, (int)object, (int)mode, start, (int)c.size(), c.data(), t0, t1, d.data(),
                                                   f.empty() ? nullptr : f.data()));
      }
      /// The curves of many objects in one call.  direct and diffuse: [blocks of all tracks, in order][n_out], the rows a gain
      /// calculator's batch form returns for the concatenated blocks; only rows of blocks the window selects
      /// (hip::timelineWindow) are read.  Every track is checked before any curve changes.  diffuse: ignored without a
      /// diffuse bus.
      void set_objects_blocks(const std::vector<hip::TimelineTrack> &tracks, const std::vector<float> &direct,
                              const std::vector<float> &diffuse, int64_t t0 = hip::kTimelineBegin,
                              int64_t t1 = hip::kTimelineEnd) {
        std::vector<int> objects, modes;
        std::vector<int64_t> starts, offsets(1, 0);
        std::vector<earhip_block_timing> blocks;
        for (auto &t : tracks) {
          const std::vector<earhip_block_timing> c = hip::detail::to_c(t.blocks);
          blocks.insert(blocks.end(), c.begin(), c.end());
          objects.push_back((int)t.object), modes.push_back((int)t.mode), starts.push_back(t.start);
          offsets.push_back((int64_t)blocks.size());
        }
        if (direct.size() != blocks.size() * n_out_) throw invalid_argument("one direct gain vector per block");
        if (two_buses_ && diffuse.size() != direct.size()) throw invalid_argument("one diffuse gain vector per block");
        hip::check(earhip_render_set_objects_blocks(h_, (int)tracks.size(), objects.data(), modes.data(), starts.data(),
                                                    offsets.data(), blocks.data(), t0, t1, direct.data(),
                                                    two_buses_ ? diffuse.data() : nullptr));
      }
      /// upload pending curve changes now (otherwise done by the next process call)
      void commit() { hip::check(earhip_render_commit(h_)); }
      /// one block: in[n_objects][block_size] -> out[n_out][block_size] (ProcessFunc shape)
      void process(const float *const *in, float *const *out) {
        hip::check(earhip_render_process(h_, 1, in, out));
      }
      /// nblocks consecutive blocks per call
      void process(size_t nblocks, const float *const *in, float *const *out) {
        hip::check(earhip_render_process(h_, nblocks, in, out));
      }
      /// device-resident planar buffers, asynchronous on the context's stream
      void process_device(size_t nblocks, const float *in_dev, size_t in_stride, float *out_dev,
                          size_t out_stride) {
        hip::check(earhip_render_process_device(h_, nblocks, in_dev, in_stride, out_dev, out_stride));
      }
      /// Interleaved PCM frames (include/earhip.h: earhip_render_process_frames): nblocks * block_size frames of
      /// frame_channels samples; this renderer's inputs are channels [first_channel, first_channel + n_objects).  The
      /// samples are converted to float on the device: int16_t s16, int32_t s32, float f32, and uint8_t s24 (3 bytes a
      /// sample).  out: n_out planar rows, as process().
      void process_frames(size_t nblocks, const int16_t *frames, int frame_channels, int first_channel, float *const *out) {
        frames_(nblocks, frames, EARHIP_PCM_S16, frame_channels, first_channel, out, 0);
      }
      void process_frames(size_t nblocks, const uint8_t *frames, int frame_channels, int first_channel, float *const *out) {
        frames_(nblocks, frames, EARHIP_PCM_S24, frame_channels, first_channel, out, 0);
      }
      void process_frames(size_t nblocks, const int32_t *frames, int frame_channels, int first_channel, float *const *out) {
        frames_(nblocks, frames, EARHIP_PCM_S32, frame_channels, first_channel, out, 0);
      }
      void process_frames(size_t nblocks, const float *frames, int frame_channels, int first_channel, float *const *out) {
        frames_(nblocks, frames, EARHIP_PCM_F32, frame_channels, first_channel, out, 0);
      }
      /// the same with interleaved outputs: out_interleaved [frames][n_out]
      void process_frames(size_t nblocks, const int16_t *frames, int frame_channels, int first_channel, float *out_interleaved) {
        frames_(nblocks, frames, EARHIP_PCM_S16, frame_channels, first_channel, &out_interleaved, 1);
      }
      void process_frames(size_t nblocks, const uint8_t *frames, int frame_channels, int first_channel, float *out_interleaved) {
        frames_(nblocks, frames, EARHIP_PCM_S24, frame_channels, first_channel, &out_interleaved, 1);
      }
      void process_frames(size_t nblocks, const int32_t *frames, int frame_channels, int first_channel, float *out_interleaved) {
        frames_(nblocks, frames, EARHIP_PCM_S32, frame_channels, first_channel, &out_interleaved, 1);
      }
      void process_frames(size_t nblocks, const float *frames, int frame_channels, int first_channel, float *out_interleaved) {
        frames_(nblocks, frames, EARHIP_PCM_F32, frame_channels, first_channel, &out_interleaved, 1);
      }
      /// device-resident frames (or device-reachable host memory) -> device outputs, asynchronous on the context's stream:
      /// out_interleaved false: out_dev [n_out][out_stride]; true: out_dev [frames][out_stride] (out_stride >= n_out)
      void process_frames_device(size_t nblocks, const int16_t *frames_dev, int frame_channels, int first_channel, float *out_dev,
                                 size_t out_stride, bool out_interleaved = false) {
        frames_device_(nblocks, frames_dev, EARHIP_PCM_S16, frame_channels, first_channel, out_dev, out_stride, out_interleaved);
      }
      void process_frames_device(size_t nblocks, const uint8_t *frames_dev, int frame_channels, int first_channel, float *out_dev,
                                 size_t out_stride, bool out_interleaved = false) {
        frames_device_(nblocks, frames_dev, EARHIP_PCM_S24, frame_channels, first_channel, out_dev, out_stride, out_interleaved);
      }
      void process_frames_device(size_t nblocks, const int32_t *frames_dev, int frame_channels, int first_channel, float *out_dev,
                                 size_t out_stride, bool out_interleaved = false) {
        frames_device_(nblocks, frames_dev, EARHIP_PCM_S32, frame_channels, first_channel, out_dev, out_stride, out_interleaved);
      }
      void process_frames_device(size_t nblocks, const float *frames_dev, int frame_channels, int first_channel, float *out_dev,
                                 size_t out_stride, bool out_interleaved = false) {
        frames_device_(nblocks, frames_dev, EARHIP_PCM_F32, frame_channels, first_channel, out_dev, out_stride, out_interleaved);
      }
      /// Interleaved PCM frames in AND out (include/earhip.h: earhip_render_process_frames_pcm): file to file in one call.  The
      /// output format is the type of the output pointer — int16_t s16, uint8_t s24 (3 bytes a sample, packed), int32_t s32,
      /// float f32 —, out_frames holds nblocks * block_size frames of n_out samples.  The conversion (scale, round half to even,
      /// saturate; optional TPDF dither for s16, a function of (seed, sample clock, channel)) runs on the device.
      struct PcmOutOptions {
        bool dither;    ///< s16 only
        uint32_t seed;  ///< of the dither hash
        PcmOutOptions(bool dither_ = false, uint32_t seed_ = 0) : dither(dither_), seed(seed_) {}
      };
      template <typename In>
      void process_frames(size_t nblocks, const In *frames, int frame_channels, int first_channel, int16_t *out_frames,
                          const PcmOutOptions &opt = PcmOutOptions()) {
        frames_pcm_(nblocks, frames, pcm_format_of(frames), frame_channels, first_channel, out_frames, EARHIP_PCM_S16, opt);
      }
      template <typename In>
      void process_frames(size_t nblocks, const In *frames, int frame_channels, int first_channel, uint8_t *out_frames,
                          const PcmOutOptions &opt = PcmOutOptions()) {
        frames_pcm_(nblocks, frames, pcm_format_of(frames), frame_channels, first_channel, out_frames, EARHIP_PCM_S24, opt);
      }
      template <typename In>
      void process_frames(size_t nblocks, const In *frames, int frame_channels, int first_channel, int32_t *out_frames,
                          const PcmOutOptions &opt = PcmOutOptions()) {
        frames_pcm_(nblocks, frames, pcm_format_of(frames), frame_channels, first_channel, out_frames, EARHIP_PCM_S32, opt);
      }
      /// device memory to device memory, asynchronous on the context's stream: the renderer's samples are bytes
      /// [out_first_byte, + n_out * sample size) of each output frame of out_frame_bytes; every other byte is left alone
      template <typename In, typename Out>
      void process_frames_pcm_device(size_t nblocks, const In *frames_dev, int frame_channels, int first_channel, Out *out_dev,
                                     size_t out_frame_bytes, size_t out_first_byte = 0, const PcmOutOptions &opt = PcmOutOptions()) {
        earhip_pcm_out o;
        o.format = pcm_format_of(static_cast<const Out *>(out_dev));
        o.dither = opt.dither ? 1 : 0;
        o.seed = opt.seed;
        hip::check(earhip_render_process_frames_pcm_device(h_, nblocks, frames_dev, pcm_format_of(frames_dev), frame_channels,
                                                           first_channel, out_dev, out_frame_bytes, out_first_byte, &o));
      }
      /// per output channel since the last reset of these numbers: the largest |x| that went through a PCM-out call and the
      /// number of clipped samples (synchronises the stream); reset_after: zero them afterwards.  reset() zeroes them too.
      void output_levels(std::vector<float> &peak, std::vector<uint64_t> &clipped, bool reset_after = false) {
        peak.assign(n_out_, 0.0f);
        clipped.assign(n_out_, 0);
        hip::check(earhip_render_output_levels(h_, peak.data(), clipped.data(), reset_after ? 1 : 0));
      }
      /// From now on every process call of every form feeds its float32 output samples to `meter` on the device (before any PCM
      /// conversion); detach_loudness() ends it.  The meter must have n_out channels and this renderer's context, and outlive
      /// the attachment.  reset() leaves the meter alone.
      void attach_loudness(hip::LoudnessMeter &meter) { hip::check(earhip_render_attach_loudness(h_, meter.get())); }
      void detach_loudness() { hip::check(earhip_render_attach_loudness(h_, nullptr)); }
      /// From now on every process call of every form also feeds its float32 output rows to `matrix` on the device; the matrix's
      /// rows go to sink[k * sink_stride + position], position = the samples fed since the attach (fir_matrix_position()).  The
      /// sink is the caller's: device memory, or hip::Context::alloc_host memory read after synchronize().  The matrix must have
      /// n_out inputs, this renderer's block size and context, and outlive the attachment.  A call that would pass
      /// sink_capacity or the matrix's max_blocks throws ear::invalid_argument before anything is rendered.  reset() leaves the
      /// matrix alone.
      void attach_fir_matrix(hip::FirMatrix &matrix, float *sink, size_t sink_stride, size_t sink_capacity) {
        hip::check(earhip_render_attach_firmix(h_, matrix.get(), sink, sink_stride, sink_capacity));
      }
      void detach_fir_matrix() { hip::check(earhip_render_attach_firmix(h_, nullptr, nullptr, 0, 0)); }
      size_t fir_matrix_position() const {
        size_t n = 0;
        hip::check(earhip_render_firmix_position(h_, &n));
        return n;
      }
      /// From now on every process call of every form also feeds its float32 output rows to `limiter` on the device, behind an
      /// attached meter and FIR matrix, which keep seeing the unlimited bus; the limited rows go to
      /// sink[c * sink_stride + position], position = the samples fed since the attach (limiter_position()).  The limiter must
      /// have n_out channels and this renderer's context, and outlive the attachment.  A call that would pass sink_capacity or
      /// the limiter's max_samples throws ear::invalid_argument before anything is rendered.  reset() leaves the limiter alone.
      void attach_limiter(hip::Limiter &limiter, float *sink, size_t sink_stride, size_t sink_capacity) {
        hip::check(earhip_render_attach_limiter(h_, limiter.get(), sink, sink_stride, sink_capacity));
      }
      void detach_limiter() { hip::check(earhip_render_attach_limiter(h_, nullptr, nullptr, 0, 0)); }
      size_t limiter_position() const {
        size_t n = 0;
        hip::check(earhip_render_limiter_position(h_, &n));
        return n;
      }
      void reset(int64_t sample_time = 0) { hip::check(earhip_render_reset(h_, sample_time)); }
      size_t block_size() const { return block_size_; }
      size_t n_out() const { return n_out_; }

     private:
      static earhip_pcm_format pcm_format_of(const int16_t *) { return EARHIP_PCM_S16; }
      static earhip_pcm_format pcm_format_of(const uint8_t *) { return EARHIP_PCM_S24; }
      static earhip_pcm_format pcm_format_of(const int32_t *) { return EARHIP_PCM_S32; }
      static earhip_pcm_format pcm_format_of(const float *) { return EARHIP_PCM_F32; }
      void frames_pcm_(size_t nblocks, const void *frames, earhip_pcm_format fmt, int frame_channels, int first_channel,
                       void *out_frames, earhip_pcm_format out_fmt, const PcmOutOptions &opt) {
        earhip_pcm_out o;
        o.format = out_fmt;
        o.dither = opt.dither ? 1 : 0;
        o.seed = opt.seed;
        hip::check(earhip_render_process_frames_pcm(h_, nblocks, frames, fmt, frame_channels, first_channel, out_frames, &o));
      }
      void frames_(size_t nblocks, const void *frames, earhip_pcm_format fmt, int frame_channels, int first_channel, float *const *out,
                   int interleaved) {
        hip::check(earhip_render_process_frames(h_, nblocks, frames, fmt, frame_channels, first_channel, out, interleaved));
      }
      void frames_device_(size_t nblocks, const void *frames, earhip_pcm_format fmt, int frame_channels, int first_channel,
                          float *out_dev, size_t out_stride, bool interleaved) {
        hip::check(earhip_render_process_frames_device(h_, nblocks, frames, fmt, frame_channels, first_channel, out_dev, out_stride,
                                                       interleaved ? 1 : 0));
      }
      size_t n_objects_, n_out_, block_size_;
      bool two_buses_;
      earhip_render *h_ = nullptr;
    };
  }  // namespace dsp
}  // namespace ear
