// allo_kernels.h — the device form of the allocentric panner (earhip group T, api_allo.hip): a wave per 64 positions, the
// layout of k_hoa_encode (hoa_kernels.h).  Each lane owns a position: it reads its x, y, z, gain, diffuse and mask
// (coalesced loads), runs allo::pan_position once — the snapped loudspeaker table is a kernel argument, so the loops over
// channels are uniform and their reads are scalar — and keeps the at most 8 (channel, weight) pairs in registers, never a
// row of 32 gains.  It zeroes its row of the wave's LDS tile and writes those weights; the tile's 64 rows are one contiguous
// run of 64 * n_channels floats of the output, which the wave stores with the flat index as the address (256 bytes per store
// instruction, whatever n_channels is).  The same tile then serves diffuse_out.  A lane writing its own row to memory would
// put the lanes of a store n_channels * 4 bytes apart.
#pragma once

#include <hip/hip_runtime.h>

#include "allo.h"

namespace earhip {
namespace allo {

constexpr int kTileWaves = 2;  // waves (tiles of 64 positions) per workgroup
// a tile row's stride in floats: odd, so that the 32 lanes of a half-wave writing one column fall on 32 banks
__host__ __device__ inline int tile_stride(int n_channels) { return n_channels | 1; }
inline size_t tile_lds_bytes(int n_channels) { return sizeof(float) * kTileWaves * 64 * (size_t)tile_stride(n_channels); }

// the rows [0, rows) of a wave's tile to dst, a contiguous run of rows * n_channels floats
__device__ inline void store_tile(const float *tile, int stride, unsigned n_channels, unsigned rows, int lane, float *dst) {
  const unsigned count = rows * n_channels;
  for (unsigned f = lane; f < count; f += 64) {
    const unsigned r = f / n_channels, c = f - r * n_channels;
    dst[f] = tile[r * stride + c];
  }
}

__global__ void __launch_bounds__(64 * kTileWaves)
    k_allo_calculate(Table t, size_t n, const double *__restrict__ x, const double *__restrict__ y,
                     const double *__restrict__ z, const double *__restrict__ gain, const double *__restrict__ diffuse,
                     const uint32_t *__restrict__ excluded, float *__restrict__ direct, float *__restrict__ diffuse_out,
                     int *__restrict__ status) {
  extern __shared__ float allo_tiles[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int stride = tile_stride(t.n);
  float *tile = allo_tiles + (size_t)wave * 64 * stride;
  const size_t first = ((size_t)blockIdx.x * kTileWaves + wave) * 64;  // the tile's first position
  const size_t i = first + lane;
  const bool live = i < n;
  const double px = live ? x[i] : 0.0, py = live ? y[i] : 0.0, pz = live ? z[i] : 0.0;
  const double g = live && gain ? gain[i] : 1.0, d = live && diffuse ? diffuse[i] : 0.0;
  const uint32_t mask = live && excluded ? excluded[i] : 0u;
  const bool ok = position_valid(px, py, pz, g, d);
  Gains hit;
  pan_position(t, ok ? px : 0.0, ok ? py : 0.0, ok ? pz : 0.0, mask, hit);
  if (live && status) status[i] = ok ? 0 : 1;
  const unsigned rows = first >= n ? 0u : (n - first < 64 ? (unsigned)(n - first) : 64u);  // of this tile, wave-uniform
  float *row = tile + lane * stride;
  const float nan = __int_as_float(0x7fc00000);

  if (ok) {
    write_row(t, hit, g, direct_factor(d), row);
  } else {
    for (int c = 0; c < t.n; c++) row[c] = nan;
  }
  __syncthreads();
  store_tile(tile, stride, (unsigned)t.n, rows, lane, direct + first * (size_t)t.n);
  if (diffuse_out == nullptr) return;  // (uniform: the same for every thread of the launch)
  __syncthreads();
  if (ok) {
    write_row(t, hit, g, diffuse_factor(d), row);
  } else {
    for (int c = 0; c < t.n; c++) row[c] = nan;
  }
  __syncthreads();
  store_tile(tile, stride, (unsigned)t.n, rows, lane, diffuse_out + first * (size_t)t.n);
}

}  // namespace allo
}  // namespace earhip
