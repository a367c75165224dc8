// api_hoa.hip — the Ambisonic encoder for Objects and the rotation of the HOA bus (earhip group Q; libear has no
// counterpart, the conventions are those of its hoa::sph_harm).  The arithmetic is hoa_encode.h, shared by the host form
// (computed on the calling thread, like the host forms of group K) and the device form (hoa_kernels.h: a wave per 64
// positions, enqueued on the context's stream).  The rotation matrix is host arithmetic over the decoder's t-design.  And
// the HOA decode matrix of group I (libear's GainCalculatorHOA): host linear algebra over the same design, whose
// directions the point source panner of api_panner.hip pans on the device.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "hoa_encode.h"
#include "hoa_kernels.h"
#include "panner.h"
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

// the design's directions as unit vectors (src/hoa/hoa.cpp:4-14), [kTDesignPoints][3]
std::vector<double> earhip::tdesign_directions(size_t extra_rows) {
  const size_t P = (size_t)kTDesignPoints;
  std::vector<double> xyz(3 * (P + extra_rows));
  for (size_t i = 0; i < P; i++) {
    const double phi = kTDesign[i][0], theta = kTDesign[i][1];
    xyz[3 * i] = std::sin(theta) * std::cos(phi);
    xyz[3 * i + 1] = std::sin(theta) * std::sin(phi);
    xyz[3 * i + 2] = std::cos(theta);
  }
  return xyz;
}

// GainCalculatorHOAImpl (src/hoa/gain_calculator_hoa.cpp:8-72): AllRAD — the point source panner sampled
// at the 5200 directions of a spherical t-design (device, one thread per direction), times the N3D
// spherical harmonics at those directions (host, double: a cold 24 x 5200 x n_coef product), power
// normalised and converted to the requested normalisation.
int earhip_hoa_decode_matrix(earhip_ctx *ctx, const char *layout, int n_coef, const int *orders, const int *degrees,
                             const char *normalization, float *out) {
  return earhip_hoa_decode_matrix_positions(ctx, layout, 0, nullptr, nullptr, n_coef, orders, degrees, normalization, out);
}

int earhip_hoa_decode_matrix_positions(earhip_ctx *ctx, const char *layout, int n_channels, const double *azimuth,
                                       const double *elevation, int n_coef, const int *orders, const int *degrees,
                                       const char *normalization, float *out) {
  return guarded([&] {
    require(ctx != nullptr && out != nullptr, "NULL argument");
    require(n_coef >= 1 && orders != nullptr && degrees != nullptr, "orders and degrees must be the same size");
    require(n_coef <= 4096, "too many coefficients");
    for (int i = 0; i < n_coef; i++) {
      require(orders[i] >= 0, "orders must not be negative");
      require(std::abs(degrees[i]) <= orders[i], "magnitude of degree must not be greater than order");
      require(orders[i] <= 64, "order too high");
    }
    const HoaNorm norm = parse_norm(normalization);
    earhip_panner *pn = nullptr;
    const int st = panner_create(ctx, layout, n_channels, azimuth, elevation, &pn, false);
    if (st != EARHIP_OK) throw Error{st, earhip_last_error()};
    std::unique_ptr<earhip_panner, int (*)(earhip_panner *)> guard(pn, earhip_panner_destroy);
    const PanParams &pp = panner_params(pn);
    const size_t P = (size_t)kTDesignPoints, C = (size_t)n_coef;
    const size_t S = pp.stereo ? 2 : (size_t)pp.table.n_real;
    // G_virt [P][S] on the device
    const std::vector<double> xyz = tdesign_directions();
    unsigned missed = 0;
    const std::vector<double> G = panner_pan_points(pn, P, xyz.data(), &missed);
    if (missed) fail_internal("point source panner: a design direction was not handled by any region");
    // Y_virt [C][P], N3D (hoa.hpp:115-133)
    std::vector<double> Y(C * P);
    for (size_t i = 0; i < P; i++) {
      const double az = -std::atan2(xyz[3 * i], xyz[3 * i + 1]);
      const double el = std::atan2(xyz[3 * i + 2], std::hypot(xyz[3 * i], xyz[3 * i + 1]));
      for (size_t c = 0; c < C; c++) {
        const int n = orders[c], m = degrees[c], am = std::abs(m);
        const double trig = m > 0 ? std::sqrt(2.0) * std::cos(m * az) : m < 0 ? -std::sqrt(2.0) * std::sin(m * az) : 1.0;
        Y[c * P + i] = hoa_norm(kN3D, n, am) * legendre_nm(n, am, std::sin(el)) * trig;
      }
    }
    // D = G_virt (Y_virt^T / P), then |D Y_virt|_F = sqrt(P), then N3D -> norm (gain_calculator_hoa.cpp:56-63)
    std::vector<double> D(S * C, 0.0);
    for (size_t sp = 0; sp < S; sp++)
      for (size_t c = 0; c < C; c++) {
        double acc = 0.0;
        for (size_t i = 0; i < P; i++) acc += G[i * S + sp] * (Y[c * P + i] / (double)P);
        D[sp * C + c] = acc;
      }
    double fro = 0.0;
    for (size_t sp = 0; sp < S; sp++)
      for (size_t i = 0; i < P; i++) {
        double v = 0.0;
        for (size_t c = 0; c < C; c++) v += D[sp * C + c] * Y[c * P + i];
        fro += v * v;
      }
    const double k = std::sqrt((double)P) / std::sqrt(fro);
    for (size_t i = 0; i < (size_t)pp.n_full * C; i++) out[i] = 0.0f;
    for (size_t sp = 0; sp < S; sp++) {
      const int row = pp.stereo ? pp.stereo_index[sp] : pp.full_index[sp];
      for (size_t c = 0; c < C; c++) {
        const int am = std::abs(degrees[c]);
        const double conv = hoa_norm(kN3D, orders[c], am) / hoa_norm(norm, orders[c], am);
        out[(size_t)row * C + c] = (float)(D[sp * C + c] * k * conv);
      }
    }
  });
}

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
    // mapping of the design's angles, tdesign_directions)
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
