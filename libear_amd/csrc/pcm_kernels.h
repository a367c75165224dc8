// pcm_kernels.h — the device side of earhip_render_process_frames (include/earhip.h, group F): interleaved PCM frames in, the
// renderer's planar float rows out, and the render's planar outputs back out as interleaved float frames.
//
// k_pcm_to_rows: deinterleave, convert and select channels in one pass.  A workgroup takes a tile of kPcmFrames frames x
// kPcmChans selected channels.  Each frame's part of the tile is one run of bytes (kPcmChans * S of them, at any byte offset for
// s24): the workgroup loads the dwords that cover these runs, consecutive threads on consecutive dwords of a frame (coalesced
// whatever the frame stride is), into LDS rows of kStride dwords — odd, so that the 32 lanes of an LDS read group, which read
// one channel of 32 consecutive frames, hit 32 different banks (ds_read_b32 banks: dword address mod 32).  Then each wave
// takes one channel at a time and writes 64 consecutive samples of its row: full 256-byte lines.  Only dwords holding at least
// one byte of a run are read: a dword never crosses a page, so no load leaves the pages of the caller's frames.
// The conversions are the ones include/earhip.h defines (exact: a power-of-two scale of an int that converts exactly, or with
// round-to-nearest-even for s32; f32 moves the bits as they are).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace earhip {

constexpr int kPcmFrames = 64, kPcmChans = 64, kPcmThreads = 256;

template <int S>
struct PcmTile {
  static constexpr int kLoad = kPcmChans * S / 4 + 1;  // dwords that cover one frame's run at any offset
  static constexpr int kStride = (kLoad + 1) | 1;      // + the dword after it (a sample read as two dwords), odd
};

// frames: the first byte of frame 0 of this launch; frame f, selected channel m = bytes [f * frame_bytes + first_byte + m * S, + S)
// out: [M][row_stride], samples [0, len) of each row.  fmt: 1 s16, 2 s24, 3 s32, 4 f32 (S = 2, 3, 4, 4).
template <int S, bool kF32>
__global__ __launch_bounds__(kPcmThreads) void k_pcm_to_rows(const unsigned char *frames, size_t frame_bytes, size_t first_byte, int M,
                                                              size_t len, float *out, size_t row_stride) {
  using T = PcmTile<S>;
  __shared__ unsigned tile[kPcmFrames * T::kStride];
  const size_t f0 = (size_t)blockIdx.x * kPcmFrames;
  const int m0 = blockIdx.y * kPcmChans;
  const int mc = min(kPcmChans, M - m0);
  const int fc = (int)min((size_t)kPcmFrames, len - f0);
  const uintptr_t run0 = reinterpret_cast<uintptr_t>(frames) + f0 * frame_bytes + first_byte + (size_t)m0 * S;
  const size_t run_bytes = (size_t)mc * S;
  for (int i = threadIdx.x; i < kPcmFrames * T::kLoad; i += kPcmThreads) {
    const int f = i / T::kLoad, j = i - f * T::kLoad;
    if (f >= fc) break;
    const uintptr_t b = run0 + (size_t)f * frame_bytes;
    const uintptr_t a = (b & ~(uintptr_t)3) + 4 * (uintptr_t)j;
    if (a < b + run_bytes) tile[f * T::kStride + j] = *reinterpret_cast<const unsigned *>(a);
  }
  __syncthreads();
  const int f = threadIdx.x & (kPcmFrames - 1);
  if (f >= fc) return;
  const int o = (int)((run0 + (size_t)f * frame_bytes) & 3);  // (0 for s32 / f32: aligned; even for s16)
  const unsigned *row = tile + f * T::kStride;
  float *dst = out + (size_t)m0 * row_stride + f0 + f;
  for (int m = threadIdx.x / kPcmFrames; m < mc; m += kPcmThreads / kPcmFrames) {
    const int byte = o + m * S, idx = byte >> 2, sh = (byte & 3) * 8;
    if (S == 2) {
      const int x = (int)(short)(unsigned short)(row[idx] >> sh);
      dst[(size_t)m * row_stride] = (float)x * 0x1p-15f;
    } else if (S == 3) {
      const unsigned long long w = (unsigned long long)row[idx] | ((unsigned long long)row[idx + 1] << 32);
      const int x = (int)((unsigned)(w >> sh) << 8) >> 8;
      dst[(size_t)m * row_stride] = (float)x * 0x1p-23f;
    } else if (kF32) {
      reinterpret_cast<unsigned *>(dst)[(size_t)m * row_stride] = row[idx];  // (the bits: NaN payloads, denormals)
    } else {
      dst[(size_t)m * row_stride] = (float)(int)row[idx] * 0x1p-31f;  // (v_cvt_f32_i32: round to nearest even)
    }
  }
}

// k_rows_to_frames: planar rows [N][in_stride] (samples [0, len)) -> frames [len][out_stride] (channels [0, N) of each), through an
// LDS tile of kIlvChans channels x kIlvFrames frames: coalesced row reads, and runs of up to kIlvChans consecutive floats per frame
// written (the whole tile one contiguous range when out_stride == N <= kIlvChans).  Rows of kIlvFrames + 1 floats: the lanes of a
// read group take consecutive channels of one frame, 32 different banks.  Moves bits, no arithmetic.
constexpr int kIlvFrames = 64, kIlvChans = 32;
__global__ __launch_bounds__(256) void k_rows_to_frames(const float *in, size_t in_stride, int N, size_t len, float *out, size_t out_stride) {
  __shared__ float t[kIlvChans][kIlvFrames + 1];
  const size_t f0 = (size_t)blockIdx.x * kIlvFrames;
  const int n0 = blockIdx.y * kIlvChans;
  const int nc = min(kIlvChans, N - n0);
  const int fc = (int)min((size_t)kIlvFrames, len - f0);
  for (int i = threadIdx.x; i < nc * kIlvFrames; i += 256) {
    const int n = i / kIlvFrames, f = i - n * kIlvFrames;
    if (f < fc) t[n][f] = in[(size_t)(n0 + n) * in_stride + f0 + f];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < fc * nc; i += 256) {
    const int f = i / nc, n = i - f * nc;
    out[(f0 + f) * out_stride + n0 + n] = t[n][f];
  }
}

}  // namespace earhip
