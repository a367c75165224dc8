// pcm_out_kernels.h — the device side of earhip_render_process_frames_pcm (include/earhip.h, group F): the render's planar float
// rows out as interleaved PCM frames, with the per-channel peak and clip count taken on the way.  The mirror image of
// k_pcm_to_rows (pcm_kernels.h).
//
// k_rows_to_pcm: a workgroup takes a tile of kOutFrames frames x kOutChans channels.
//   1. Each wave takes one channel at a time and reads 64 consecutive samples of its row (full 256-byte lines), converts its
//      sample (pcm_convert.h: the rules of the header), and places it in LDS AS THE BYTES OF THE OUTPUT FRAME: frame f is an LDS
//      row of kStride dwords whose byte k stands for the byte k of the aligned dwords that cover the frame's run in global
//      memory (so a dword of the run that lies inside one frame is an aligned LDS dword).  kStride is odd: the 64 lanes of a
//      wave write one channel of 64 consecutive frames, different banks.
//   2. |x| and the clip flag are reduced across the wave (__shfl_xor / __ballot) and lane 0 issues ONE atomicMax on the bits
//      of |x| (non-negative floats order as unsigned integers) and ONE 64-bit atomicAdd per (wave, channel), each skipped
//      when the wave has nothing to add, to one of kLevelSlots copies of the levels (below).
//   3. The tile's bytes are written out in whole dwords, consecutive threads on consecutive dwords: per frame run, or —
//      when the frames are exactly the renderer's samples (out_frame_bytes == N * S, all channels in one tile) — over the
//      tile as ONE contiguous range.  A dword of which only some bytes belong to the range (the first and last of a run at
//      an odd offset: s24, odd N, wide frames) is written as byte stores of those bytes alone: no byte outside the runs is
//      written or read, so another renderer may write its channels of the same frames at the same time.
// The dither hash is integer VALU work per sample and exists only in the kDither instantiation.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pcm_convert.h"

namespace earhip {

constexpr int kOutFrames = 64, kOutChans = 32, kOutThreads = 256;
// The levels live in kLevelSlots copies [kLevelSlots][N]; a workgroup adds to the copy of its tile index, and the host takes the
// maximum / the sum over the copies (earhip_render_output_levels).  With one copy, every wave of a launch met the others on
// N addresses: 2048 workgroups x 24 channels of a 256-block call took 377 us in the atomics against 9 us for the data.
constexpr int kLevelSlots = 64;

template <int S>
struct PcmOutTile {
  // dwords that cover one frame's run of kOutChans samples at any offset the API admits: s16 / s32 / f32 runs start on a
  // multiple of their sample size (earhip.h refuses other out_dev / out_first_byte / out_frame_bytes), s24 runs at any byte:
  // a run of R = kOutChans * S bytes (a multiple of 4) at offset o in [0, 4) within its first dword covers R / 4 + 1 dwords
  static_assert((kOutChans * S) % 4 == 0, "a full run is whole dwords long");
  static constexpr int kLoad = kOutChans * S / 4 + 1;
  static constexpr int kStride = kLoad | 1;            // odd
};

struct PcmOutArgs {
  const float *in;         // [N][in_stride], samples [0, len)
  size_t in_stride;
  int N;
  size_t len;
  unsigned char *out;      // the first byte of frame 0 of this launch
  size_t frame_bytes;      // distance between output frames
  size_t first_byte;       // the renderer's samples: bytes [first_byte, first_byte + N * S) of each frame
  unsigned *peak;          // [kLevelSlots][N] bits of the largest |x|
  unsigned long long *clipped;  // [kLevelSlots][N]
  unsigned seed;
  long long t0;            // sample clock of frame 0
};

// FMT: kPcmS16 / S24 / S32 / F32 (S = 2, 3, 4, 4 bytes per sample)
template <int FMT, bool kDither>
__global__ __launch_bounds__(kOutThreads) void k_rows_to_pcm(PcmOutArgs a) {
  constexpr int S = FMT == kPcmS16 ? 2 : FMT == kPcmS24 ? 3 : 4;
  using T = PcmOutTile<S>;
  __shared__ unsigned tile[kOutFrames * T::kStride];
  unsigned char *tile_b = reinterpret_cast<unsigned char *>(tile);
  const size_t f0 = (size_t)blockIdx.x * kOutFrames;
  const int n0 = blockIdx.y * kOutChans;
  const int nc = min(kOutChans, a.N - n0);
  const int fc = (int)min((size_t)kOutFrames, a.len - f0);
  const unsigned rb = (unsigned)nc * S;  // bytes of one frame's run
  const uintptr_t run0 = reinterpret_cast<uintptr_t>(a.out) + f0 * a.frame_bytes + a.first_byte + (size_t)n0 * S;

  // 1. + 2.: convert into the LDS image of the frames, levels by the way
  {
    const int f = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool live = f < fc;
    const int o = (int)((run0 + (size_t)f * a.frame_bytes) & 3);
    for (int n = w; n < nc; n += kOutThreads / 64) {
      float x = 0.f;
      if (live) x = a.in[(size_t)(n0 + n) * a.in_stride + f0 + f];
      const unsigned xb = __float_as_uint(x);
      unsigned mag = xb & 0x7FFFFFFFu;
      if (mag > 0x7F800000u) mag = 0;  // (NaN: not a level)
      bool clip = false;
      unsigned q;
      if constexpr (FMT == kPcmF32) {
        q = xb;
      } else {
        float d = 0.f;
        if (kDither) d = pcm_dither_value(pcm_dither_hash(a.seed, (uint64_t)(a.t0 + (long long)(f0 + f)), (uint32_t)(n0 + n)));
        q = (unsigned)pcm_from_float<FMT, kDither>(x, d, &clip);
      }
      if (live) {
        const int byte = f * (T::kStride * 4) + o + n * S;
        if (S == 4) {
          tile[byte >> 2] = q;
        } else if (S == 2) {
          *reinterpret_cast<unsigned short *>(tile_b + byte) = (unsigned short)q;  // (o is even for s16: aligned)
        } else {
          tile_b[byte] = (unsigned char)q;
          tile_b[byte + 1] = (unsigned char)(q >> 8);
          tile_b[byte + 2] = (unsigned char)(q >> 16);
        }
      }
      for (int sh = 32; sh >= 1; sh >>= 1) mag = max(mag, (unsigned)__shfl_xor((int)mag, sh, 64));
      const unsigned long long cl = FMT == kPcmF32 ? 0ull : __ballot(clip && live);
      if (f == 0) {
        const size_t slot = (size_t)(blockIdx.x % kLevelSlots) * a.N + n0 + n;
        if (mag > a.peak[slot]) atomicMax(&a.peak[slot], mag);
        if (cl) atomicAdd(&a.clipped[slot], (unsigned long long)__popcll(cl));
      }
    }
  }
  __syncthreads();

  // 3.: write out.  A range of bytes [g0, g0 + total) of global memory; byte q of it belongs to frame fr = q / rb of the tile.
  const bool whole = a.frame_bytes == (size_t)rb && nc == a.N;
  const unsigned nranges = whole ? 1u : (unsigned)fc;
  const unsigned total = whole ? (unsigned)fc * rb : rb;
  const unsigned per = whole ? (total + 3) / 4 + 1 : (unsigned)T::kLoad;  // dwords that cover a range at any offset
  for (unsigned i = threadIdx.x; i < nranges * per; i += kOutThreads) {
    const unsigned rg = whole ? 0u : i / per, j = i - rg * per;
    const uintptr_t g0 = run0 + (size_t)rg * a.frame_bytes;
    const uintptr_t ad = (g0 & ~(uintptr_t)3) + 4 * (uintptr_t)j;  // this thread's aligned dword
    if (ad >= g0 + total) continue;
    const long long q0 = (long long)ad - (long long)g0;  // its first byte within the range (negative: before it)
    // LDS byte of range byte q
    auto lds_byte = [&](unsigned q) -> unsigned {
      const unsigned fr = whole ? q / rb : rg;
      const unsigned r = whole ? q - fr * rb : q;
      const unsigned o = (unsigned)((run0 + (size_t)fr * a.frame_bytes) & 3);
      return fr * (unsigned)(T::kStride * 4) + o + r;
    };
    const bool full = q0 >= 0 && (unsigned long long)q0 + 4 <= total;
    if (full) {
      const unsigned lb0 = lds_byte((unsigned)q0), lb3 = lds_byte((unsigned)q0 + 3);
      unsigned v;
      if (lb3 == lb0 + 3) {
        v = tile[lb0 >> 2];  // (inside one frame: aligned in LDS as in global memory)
      } else {
        v = (unsigned)tile_b[lb0] | ((unsigned)tile_b[lds_byte((unsigned)q0 + 1)] << 8) |
            ((unsigned)tile_b[lds_byte((unsigned)q0 + 2)] << 16) | ((unsigned)tile_b[lb3] << 24);
      }
      *reinterpret_cast<unsigned *>(ad) = v;
    } else {
      for (int k = 0; k < 4; k++) {
        const long long q = q0 + k;
        if (q >= 0 && q < (long long)total) *reinterpret_cast<unsigned char *>(ad + k) = tile_b[lds_byte((unsigned)q)];
      }
    }
  }
}

}  // namespace earhip
