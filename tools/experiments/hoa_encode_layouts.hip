// hoa_encode_layouts.hip — the two layouts of the Ambisonic encoder's kernel (earhip group Q) side by side on resident arrays:
// the library's wave-per-64-positions kernel (libear_amd/csrc/hoa_kernels.h) and one thread per output element (flat index =
// store address, no LDS, hoa::encode_one per element).  Checks that the two give the same bits, then times them in
// alternating windows with device events; one line per (order, layout).
//
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I libear_amd/csrc tools/experiments/hoa_encode_layouts.hip -o hoa_encode_layouts
// usage: hoa_encode_layouts [positions (262144)] [launches per window (20)]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "hoa_kernels.h"

using namespace earhip::hoa;

#define HIP_OK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      std::printf("HIP error %s in %s\n", hipGetErrorString(e_), #expr);              \
      std::exit(2);                                                                   \
    }                                                                                 \
  } while (0)

__global__ void __launch_bounds__(256)
    k_hoa_encode_flat(Table t, size_t n, const double *__restrict__ az, const double *__restrict__ el,
                      const double *__restrict__ gain, float *__restrict__ out, int *__restrict__ status) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n * (size_t)t.n_coef) return;
  const size_t i = f / (unsigned)t.n_coef;
  const int c = (int)(f - i * (unsigned)t.n_coef);
  const double a = az[i], e = el[i], g = gain ? gain[i] : 1.0;
  const bool ok = encode_valid(a, e, g);
  out[f] = ok ? (float)encode_one(t.ch[c], a, e, g) : __int_as_float(0x7fc00000);
  if (status && c == 0) status[i] = ok ? 0 : 1;
}

static Table acn_table(int order) {
  int orders[kMaxCoef], degrees[kMaxCoef], k = 0;
  for (int n = 0; n <= order; n++)
    for (int m = -n; m <= n; m++, k++) orders[k] = n, degrees[k] = m;
  Table t;
  fill_table(t, k, orders, degrees, kSN3D);
  return t;
}

int main(int argc, char **argv) {
  const size_t n = argc > 1 ? (size_t)std::atoll(argv[1]) : (size_t)1 << 18;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 20;
  std::mt19937_64 rng(3);
  std::uniform_real_distribution<double> uaz(-180.0, 180.0), uel(-90.0, 90.0), ug(0.1, 1.0);
  std::vector<double> az(n), el(n), gain(n);
  for (size_t i = 0; i < n; i++) az[i] = uaz(rng), el[i] = uel(rng), gain[i] = ug(rng);
  double *d_az, *d_el, *d_gain;
  float *d_out[2];
  HIP_OK(hipMalloc((void **)&d_az, n * 8));
  HIP_OK(hipMalloc((void **)&d_el, n * 8));
  HIP_OK(hipMalloc((void **)&d_gain, n * 8));
  for (int k = 0; k < 2; k++) HIP_OK(hipMalloc((void **)&d_out[k], n * kMaxCoef * 4));
  HIP_OK(hipMemcpy(d_az, az.data(), n * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_el, el.data(), n * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_gain, gain.data(), n * 8, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  for (int order : {3, 7}) {
    const Table t = acn_table(order);
    const size_t total = n * (size_t)t.n_coef, per_wg = (size_t)64 * kTileWaves;
    auto tile = [&] {
      hipLaunchKernelGGL(k_hoa_encode, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(64 * kTileWaves),
                         tile_lds_bytes(t.n_coef), 0, t, n, d_az, d_el, d_gain, d_out[0], (int *)nullptr);
    };
    auto flat = [&] {
      hipLaunchKernelGGL(k_hoa_encode_flat, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, t, n, d_az, d_el, d_gain,
                         d_out[1], (int *)nullptr);
    };
    for (int k = 0; k < 3; k++) tile(), flat();
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> a(total), b(total);
    HIP_OK(hipMemcpy(a.data(), d_out[0], total * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(b.data(), d_out[1], total * 4, hipMemcpyDeviceToHost));
    std::printf("order %d: the two layouts give %s bits\n", order, std::memcmp(a.data(), b.data(), total * 4) ? "DIFFERENT" : "the same");
    std::vector<float> ms_tile, ms_flat;
    for (int w = 0; w < 5; w++)
      for (int which = 0; which < 2; which++) {
        HIP_OK(hipEventRecord(e0, 0));
        for (int k = 0; k < reps; k++) which ? flat() : tile();
        HIP_OK(hipEventRecord(e1, 0));
        HIP_OK(hipEventSynchronize(e1));
        float ms = 0.0f;
        HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        (which ? ms_flat : ms_tile).push_back(ms / reps);
      }
    std::sort(ms_tile.begin(), ms_tile.end());
    std::sort(ms_flat.begin(), ms_flat.end());
    std::printf("order %d (%d channels), %zu positions: wave per 64 positions %.4f ms [%.4f, %.4f] = %.1f Mvectors/s; one thread "
                "per element %.4f ms [%.4f, %.4f] = %.1f Mvectors/s\n", order, t.n_coef, n, ms_tile[2], ms_tile[0], ms_tile[4],
                n / ms_tile[2] / 1e3, ms_flat[2], ms_flat[0], ms_flat[4], n / ms_flat[2] / 1e3);
  }
  return 0;
}
