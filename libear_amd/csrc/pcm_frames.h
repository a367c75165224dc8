// pcm_frames.h — group F's conversions (include/earhip.h: interleaved PCM frames in and out) as the renderer (api_render.hip) and
// the limiter's PCM form (api_limiter.hip) use them.  The kernels are compiled in api_frames.hip alone; none is defined here.
#pragma once

#include "common.h"

namespace earhip {

int pcm_sample_bytes(int fmt);  // of an earhip_pcm_format; 0: not a format

// frames -> planar rows out [M][row_stride] (samples [0, len)), on stream s
void launch_pcm_to_rows(int fmt, const void *frames, size_t frame_bytes, size_t first_byte, int M, size_t len, float *out,
                        size_t row_stride, hipStream_t s);
// planar rows [N][in_stride] -> frames [len][out_stride], on stream s
void launch_rows_to_frames(const float *in, size_t in_stride, int N, size_t len, float *out, size_t out_stride, hipStream_t s);
// planar rows [N][in_stride] (samples [0, len), the first at sample clock t0) -> PCM frames: bytes [first_byte, + N * sample size) of
// each frame of frame_bytes at `out`; levels into peak / clipped (PcmLevels); on stream s
void launch_rows_to_pcm(const earhip_pcm_out &o, const float *in, size_t in_stride, int N, size_t len, unsigned char *out,
                        size_t frame_bytes, size_t first_byte, unsigned *peak, unsigned long long *clipped, int64_t t0, hipStream_t s);

// what every PCM-out form refuses about its earhip_pcm_out (returns the output sample size), and what the device forms refuse
// about where the C samples of So bytes go in the caller's frames (`channels`: the caller's name for C, "n_out" or "n_channels")
size_t check_pcm_out(const earhip_pcm_out *out);
void check_pcm_out_frame(int C, size_t So, const void *out_dev, size_t out_frame_bytes, size_t out_first_byte, const char *channels);

// The levels k_rows_to_pcm keeps: several copies [slots][C] of the peak's bits and of the clip count, folded on the host
// (pcm_levels_fold, pcm_convert.h).
struct PcmLevels {
  DevBuf<unsigned> peak;
  DevBuf<unsigned long long> clip;
  void reserve(int C, hipStream_t s);  // made and zeroed at the first call (behind a synchronisation of s), kept after that
  void zero(hipStream_t s);            // (levels that were never made are zero already)
  void read(int C, float *peak_out, uint64_t *clipped_out) const;  // (the caller has synchronised the stream that wrote them)
};

}  // namespace earhip
