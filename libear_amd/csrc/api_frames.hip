// api_frames.hip — group F's conversions (pcm_frames.h): interleaved PCM frames <-> planar float rows on the device, for the
// renderer's frames forms (api_render.hip) and the limiter's PCM form.  The one unit that compiles pcm_kernels.h and pcm_out_kernels.h.
#include <cstring>
#include <vector>

#include "pcm_frames.h"
#include "pcm_kernels.h"
#include "pcm_out_kernels.h"

namespace earhip {

int pcm_sample_bytes(int fmt) {
  switch (fmt) {
    case EARHIP_PCM_S16: return 2;
    case EARHIP_PCM_S24: return 3;
    case EARHIP_PCM_S32: case EARHIP_PCM_F32: return 4;
    default: return 0;
  }
}

void launch_pcm_to_rows(int fmt, const void *frames, size_t frame_bytes, size_t first_byte, int M, size_t len, float *out,
                        size_t row_stride, hipStream_t s) {
  const dim3 grid((unsigned)((len + kPcmFrames - 1) / kPcmFrames), (unsigned)((M + kPcmChans - 1) / kPcmChans));
  const unsigned char *f = static_cast<const unsigned char *>(frames);
  switch (fmt) {
    case EARHIP_PCM_S16: hipLaunchKernelGGL((k_pcm_to_rows<2, false>), grid, dim3(kPcmThreads), 0, s, f, frame_bytes, first_byte, M, len, out, row_stride); break;
    case EARHIP_PCM_S24: hipLaunchKernelGGL((k_pcm_to_rows<3, false>), grid, dim3(kPcmThreads), 0, s, f, frame_bytes, first_byte, M, len, out, row_stride); break;
    case EARHIP_PCM_S32: hipLaunchKernelGGL((k_pcm_to_rows<4, false>), grid, dim3(kPcmThreads), 0, s, f, frame_bytes, first_byte, M, len, out, row_stride); break;
    default: hipLaunchKernelGGL((k_pcm_to_rows<4, true>), grid, dim3(kPcmThreads), 0, s, f, frame_bytes, first_byte, M, len, out, row_stride); break;
  }
  EARHIP_HIP(hipGetLastError());
}

void launch_rows_to_frames(const float *in, size_t in_stride, int N, size_t len, float *out, size_t out_stride, hipStream_t s) {
  const dim3 grid((unsigned)((len + kIlvFrames - 1) / kIlvFrames), (unsigned)((N + kIlvChans - 1) / kIlvChans));
  hipLaunchKernelGGL(k_rows_to_frames, grid, dim3(256), 0, s, in, in_stride, N, len, out, out_stride);
  EARHIP_HIP(hipGetLastError());
}

void launch_rows_to_pcm(const earhip_pcm_out &o, const float *in, size_t in_stride, int N, size_t len, unsigned char *out,
                        size_t frame_bytes, size_t first_byte, unsigned *peak, unsigned long long *clipped, int64_t t0, hipStream_t s) {
  const dim3 grid((unsigned)((len + kOutFrames - 1) / kOutFrames), (unsigned)((N + kOutChans - 1) / kOutChans));
  PcmOutArgs a;
  a.in = in; a.in_stride = in_stride; a.N = N; a.len = len; a.out = out; a.frame_bytes = frame_bytes; a.first_byte = first_byte;
  a.peak = peak; a.clipped = clipped; a.seed = o.seed; a.t0 = (long long)t0;
  switch (o.format) {
    case EARHIP_PCM_S16:
      if (o.dither) hipLaunchKernelGGL((k_rows_to_pcm<kPcmS16, true>), grid, dim3(kOutThreads), 0, s, a);
      else hipLaunchKernelGGL((k_rows_to_pcm<kPcmS16, false>), grid, dim3(kOutThreads), 0, s, a);
      break;
    case EARHIP_PCM_S24: hipLaunchKernelGGL((k_rows_to_pcm<kPcmS24, false>), grid, dim3(kOutThreads), 0, s, a); break;
    case EARHIP_PCM_S32: hipLaunchKernelGGL((k_rows_to_pcm<kPcmS32, false>), grid, dim3(kOutThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((k_rows_to_pcm<kPcmF32, false>), grid, dim3(kOutThreads), 0, s, a); break;
  }
  EARHIP_HIP(hipGetLastError());
}

size_t check_pcm_out(const earhip_pcm_out *out) {
  require(out != nullptr, "out (earhip_pcm_out) must not be NULL");
  const int So = pcm_sample_bytes(out->format);
  require(So != 0, "unknown PCM output format");
  require(out->dither == 0 || out->dither == 1, "dither must be 0 or 1");
  require(out->dither == 0 || out->format == EARHIP_PCM_S16, "dither is defined for EARHIP_PCM_S16 only");
  return (size_t)So;
}

void check_pcm_out_frame(int C, size_t So, const void *out_dev, size_t out_frame_bytes, size_t out_first_byte, const char *channels) {
  const std::string samples = std::string(channels) + " samples";
  require(out_dev != nullptr, "out_dev must not be NULL");
  require(So == 3 || reinterpret_cast<uintptr_t>(out_dev) % So == 0, "out_dev not aligned to the sample size");
  if (out_frame_bytes < (size_t)C * So) fail_invalid("out_frame_bytes smaller than " + samples);
  if (out_first_byte > out_frame_bytes - (size_t)C * So) fail_invalid("out_first_byte + " + samples + " exceed out_frame_bytes");
  require(So == 3 || (out_frame_bytes % So == 0 && out_first_byte % So == 0), "out_frame_bytes / out_first_byte not multiples of the sample size");
}

void PcmLevels::reserve(int C, hipStream_t s) {
  if (peak.p) return;
  EARHIP_HIP(hipStreamSynchronize(s));
  peak.alloc_zero((size_t)kLevelSlots * (size_t)C, s);
  clip.alloc_zero((size_t)kLevelSlots * (size_t)C, s);
}

void PcmLevels::zero(hipStream_t s) {
  if (!peak.p) return;
  EARHIP_HIP(hipMemsetAsync(peak.p, 0, sizeof(unsigned) * peak.n, s));
  EARHIP_HIP(hipMemsetAsync(clip.p, 0, sizeof(unsigned long long) * clip.n, s));
}

void PcmLevels::read(int C, float *peak_out, uint64_t *clipped_out) const {
  const size_t cnt = (size_t)kLevelSlots * (size_t)C;
  std::vector<unsigned> pk(cnt, 0u);
  std::vector<unsigned long long> cl(cnt, 0ull);
  if (peak.p) {  // (else: no PCM-out call yet)
    EARHIP_HIP(hipMemcpy(pk.data(), peak.p, sizeof(unsigned) * cnt, hipMemcpyDeviceToHost));
    EARHIP_HIP(hipMemcpy(cl.data(), clip.p, sizeof(unsigned long long) * cnt, hipMemcpyDeviceToHost));
  }
  pcm_levels_fold(kLevelSlots, C, pk.data(), cl.data(), peak_out, clipped_out);
}

}  // namespace earhip
