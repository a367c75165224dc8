// api_hoa.hip — the Ambisonic encoder for Objects and the rotation of the HOA bus (earhip group Q; libear has no
// counterpart, the conventions are those of its hoa::sph_harm).  The arithmetic is hoa_encode.h, shared by the host form
// (computed on the calling thread, like the host forms of group K) and the device form (hoa_kernels.h: a wave per 64
// positions, enqueued on the context's stream).  The rotation matrix is host arithmetic over the decoder's t-design.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "hoa_encode.h"
#include "hoa_kernels.h"
#include "tdesign_5200.h"

using namespace earhip;
using namespace earhip::hoa;

namespace {

HoaNorm parse_norm(const char *normalization) {
  require(normalization != nullptr, "normalization must not be NULL");
  if (std::strcmp(normalization, "N3D") == 0) return kN3D;
  if (std::strcmp(normalization, "SN3D") == 0) return kSN3D;
  if (std::strcmp(normalization, "FuMa") == 0) return kFuMa;
  throw Error{EARHIP_ADM_ERROR, std::string("ADM error: unknown normalization type: '") + normalization + "'"};
}

// the call's channel table: checked, normalised, and sorted for the position core.  No allocation.
Table make_table(int n_coef, const int *orders, const int *degrees, const char *normalization) {
  require(orders != nullptr && degrees != nullptr, "orders and degrees must not be NULL");
  require(n_coef >= 1 && n_coef <= kMaxCoef, "n_coef must lie in [1, 64]");
  for (int c = 0; c < n_coef; c++) {
    require(orders[c] >= 0, "orders must not be negative");
    require(orders[c] <= kMaxOrder, "order too high (at most 7)");
    require(std::abs(degrees[c]) <= orders[c], "magnitude of degree must not be greater than order");
  }
  const HoaNorm norm = parse_norm(normalization);
  Table t;
  fill_table(t, n_coef, orders, degrees, norm);
  return t;
}

const size_t kMaxElements = (size_t)1 << 31;

}  // namespace

int earhip_hoa_acn(int max_order, int *orders, int *degrees) {
  return guarded([&] {
    require(orders != nullptr && degrees != nullptr, "orders and degrees must not be NULL");
    require(max_order >= 0 && max_order <= kMaxOrder, "max_order must lie in [0, 7]");
    int k = 0;
    for (int n = 0; n <= max_order; n++)
      for (int m = -n; m <= n; m++, k++) orders[k] = n, degrees[k] = m;  // k = n^2 + n + m
  });
}

int earhip_hoa_encode(int n_coef, const int *orders, const int *degrees, const char *normalization, size_t n,
                      const double *azimuth, const double *elevation, const double *gain, float *out) {
  return guarded([&] {
    const Table t = make_table(n_coef, orders, degrees, normalization);
    require(n == 0 || (azimuth && elevation && out), "azimuth, elevation and out must not be NULL");
    for (size_t i = 0; i < n; i++) {
      const double g = gain ? gain[i] : 1.0;
      if (!encode_valid(azimuth[i], elevation[i], g)) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "element %zu: azimuth %g, elevation %g, gain %g: every one must be finite and the "
                      "elevation within +-90 degrees", i, azimuth[i], elevation[i], g);
        fail_invalid(msg);
      }
      float *row = out + i * (size_t)n_coef;
      encode_position(t, azimuth[i], elevation[i], g, [&](int c, double v) { row[c] = (float)v; });
    }
  });
}

int earhip_hoa_encode_device(earhip_ctx *ctx, int n_coef, const int *orders, const int *degrees, const char *normalization,
                             size_t n, const double *azimuth_dev, const double *elevation_dev, const double *gain_dev,
                             float *out_dev, int *status_dev) {
  return guarded([&] {
    require(ctx != nullptr, "context must not be NULL");
    const Table t = make_table(n_coef, orders, degrees, normalization);
    require(n < kMaxElements, "too many elements (at most 2^31 - 1 per call)");
    if (n == 0) return;
    require(azimuth_dev && elevation_dev && out_dev, "azimuth, elevation and out must not be NULL");
    ctx->use();
    const size_t per_wg = (size_t)64 * kTileWaves;
    hipLaunchKernelGGL(k_hoa_encode, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(64 * kTileWaves),
                       tile_lds_bytes(n_coef), ctx->stream, t, n, azimuth_dev, elevation_dev, gain_dev, out_dev, status_dev);
    EARHIP_HIP(hipGetLastError());
  });
}

int earhip_hoa_rotation_matrix(int n_coef, const int *orders, const int *degrees, const char *normalization, const double *q,
                               float *out) {
  return guarded([&] {
    const Table t = make_table(n_coef, orders, degrees, normalization);
    require(q != nullptr && out != nullptr, "q and out must not be NULL");
    for (int i = 0; i < 9; i++) require(std::isfinite(q[i]), "q must be finite");
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double dot = 0.0;
        for (int k = 0; k < 3; k++) dot += q[3 * i + k] * q[3 * j + k];
        require(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-9, "q must be orthonormal (q q^T = I to 1e-9)");
      }
    const double det = q[0] * (q[4] * q[8] - q[5] * q[7]) - q[1] * (q[3] * q[8] - q[5] * q[6]) +
                       q[2] * (q[3] * q[7] - q[4] * q[6]);
    require(std::fabs(det - 1.0) <= 1e-9, "q must be a proper rotation (determinant +1 to 1e-9)");
    // the same channels in N3D; R = (1/P) sum_p y(q x_p) y(x_p)^T over the design's directions (ADM axes: the decoder's
    // mapping of the design's angles, api_panner.hip)
    Table t3;
    fill_table(t3, n_coef, orders, degrees, kN3D);
    const size_t C = (size_t)n_coef;
    std::vector<double> R(C * C, 0.0);
    double y[kMaxCoef], yq[kMaxCoef];
    auto harmonics = [&](const double v[3], double *dst) {
      const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      const double x = std::max(-1.0, std::min(1.0, v[2] / len));
      encode_position_rad(t3, -std::atan2(v[0], v[1]), x, 1.0, [&](int c, double val) { dst[c] = val; });
    };
    for (int p = 0; p < kTDesignPoints; p++) {
      const double phi = kTDesign[p][0], theta = kTDesign[p][1];
      const double u[3] = {std::sin(theta) * std::cos(phi), std::sin(theta) * std::sin(phi), std::cos(theta)};
      double v[3];
      for (int i = 0; i < 3; i++) v[i] = q[3 * i] * u[0] + q[3 * i + 1] * u[1] + q[3 * i + 2] * u[2];
      harmonics(u, y);
      harmonics(v, yq);
      for (size_t i = 0; i < C; i++)
        for (size_t j = 0; j < C; j++) R[i * C + j] += yq[i] * y[j];
    }
    for (size_t i = 0; i < C; i++)
      for (size_t j = 0; j < C; j++) {
        const double v = R[i * C + j] / (double)kTDesignPoints * (t.ch[i].k / t3.ch[i].k) * (t3.ch[j].k / t.ch[j].k);
        out[i * C + j] = t.ch[i].n == t.ch[j].n ? (float)v : 0.0f;
      }
  });
}
