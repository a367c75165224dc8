// hoa_kernels.h — the device form of the Ambisonic encoder (earhip group Q, api_hoa.hip): a wave per 64 positions.
// Each lane owns a position: it reads its azimuth, elevation and gain (coalesced 8-byte loads), runs hoa::encode_position once
// — the channel table is a kernel argument, so the loop over channels is uniform and its reads are scalar — and leaves its
// row in the wave's LDS tile.  The tile's 64 rows are one contiguous run of 64 * n_coef floats of the output, which the wave
// then stores with the flat index as the address (256 bytes per store instruction, whatever n_coef is).  A lane writing its
// own row to memory would put the lanes of a store n_coef * 4 bytes apart.
// The other layout, one thread per output element, needs no LDS but repeats the position's sin / sqrt / fmod and the
// recurrence per element and diverges on (n, m): tools/experiments/hoa_encode_layouts.hip measures the two (NOTES.md).
#pragma once

#include "hoa_encode.h"

namespace earhip {
namespace hoa {

constexpr int kTileWaves = 2;  // waves (tiles of 64 positions) per workgroup
// a tile row's stride in floats: odd, so that the 32 lanes of a half-wave writing one column fall on 32 banks
__host__ __device__ inline int tile_stride(int n_coef) { return n_coef | 1; }
inline size_t tile_lds_bytes(int n_coef) { return sizeof(float) * kTileWaves * 64 * (size_t)tile_stride(n_coef); }

__global__ void __launch_bounds__(64 * kTileWaves)
    k_hoa_encode(Table t, size_t n, const double *__restrict__ az, const double *__restrict__ el,
                 const double *__restrict__ gain, float *__restrict__ out, int *__restrict__ status) {
  extern __shared__ float hoa_tiles[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int stride = tile_stride(t.n_coef);
  float *tile = hoa_tiles + (size_t)wave * 64 * stride;
  const size_t first = ((size_t)blockIdx.x * kTileWaves + wave) * 64;  // the tile's first position
  const size_t i = first + lane;
  const bool live = i < n;
  const double a = live ? az[i] : 0.0, e = live ? el[i] : 0.0, g = live ? (gain ? gain[i] : 1.0) : 0.0;
  const bool ok = encode_valid(a, e, g);
  float *row = tile + lane * stride;
  encode_position(t, a, e, g, [&](int c, double v) { row[c] = ok ? (float)v : __int_as_float(0x7fc00000); });
  if (live && status) status[i] = ok ? 0 : 1;
  __syncthreads();
  if (first >= n) return;
  const size_t rows = n - first < 64 ? n - first : 64;
  const unsigned count = (unsigned)rows * (unsigned)t.n_coef;
  float *dst = out + first * (size_t)t.n_coef;
  for (unsigned f = lane; f < count; f += 64) {
    const unsigned r = f / (unsigned)t.n_coef, c = f - r * (unsigned)t.n_coef;
    dst[f] = tile[r * stride + c];
  }
}

}  // namespace hoa
}  // namespace earhip
