// api_screen.hip — screenRef scaling and screenEdgeLock of Objects positions (earhip group R; ITU-R BS.2127-0 sections 7.3.3
// and 7.3.4, which libear refuses).  The per-element arithmetic is screen.h, shared by the host form (computed on the calling
// thread, like the host forms of group K) and the device form (one thread per element, enqueued on the context's stream).
// A screen's edges, and from them the six segments of a call, are host arithmetic.  Group V is the same stage for Cartesian
// positions: screen_cart.h wraps the per-element arithmetic in group K's point conversions, one kernel and one host loop here.
#include <cmath>
#include <cstdio>
#include <string>

#include "common.h"
#include "screen.h"
#include "screen_cart.h"

using namespace earhip;
using namespace earhip::screen;

namespace {

const earhip_screen kDefaultScreen = {0, 1.78, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 58.0, 0.0};

constexpr double kPi = 3.141592653589793238462643383279502884;

struct Vec {
  double x, y, z;
};

Vec cart(double az, double el, double d) {
  const double a = -az * (kPi / 180.0), e = el * (kPi / 180.0);
  return Vec{std::sin(a) * std::cos(e) * d, std::cos(a) * std::cos(e) * d, std::sin(e) * d};
}
double azim(const Vec &v) { return -std::atan2(v.x, v.y) * (180.0 / kPi); }
double elev(const Vec &v) { return std::atan2(v.z, std::hypot(v.x, v.y)) * (180.0 / kPi); }

void need(bool ok, const char *which, const char *field, const char *rule) {
  if (!ok) fail_invalid(std::string(which) + " screen: " + field + " " + rule);
}

// earhip_screen_edges with the screen's role in the message
void screen_edges(const earhip_screen &s, const char *which, double e[4]) {
  need(std::isfinite(s.aspect_ratio), which, "aspect_ratio", "must be finite");
  need(s.aspect_ratio > 0.0, which, "aspect_ratio", "must be positive");
  Vec c, xv, zv;
  if (s.cartesian == 0) {
    need(std::isfinite(s.azimuth), which, "azimuth", "must be finite");
    need(std::isfinite(s.elevation), which, "elevation", "must be finite");
    need(std::isfinite(s.distance), which, "distance", "must be finite");
    need(std::isfinite(s.width_azimuth), which, "width_azimuth", "must be finite");
    need(s.width_azimuth > 0.0 && s.width_azimuth < 180.0, which, "width_azimuth", "must lie within (0, 180) degrees");
    need(s.distance > 0.0, which, "distance", "must be positive");
    need(std::fabs(s.elevation) <= 90.0, which, "elevation", "must lie within +-90 degrees");
    c = cart(s.azimuth, s.elevation, s.distance);
    const double W = s.distance * std::tan(s.width_azimuth / 2.0 * (kPi / 180.0)), H = W / s.aspect_ratio;
    const Vec ux = cart(s.azimuth - 90.0, 0.0, 1.0), uz = cart(s.azimuth, s.elevation + 90.0, 1.0);
    xv = Vec{W * ux.x, W * ux.y, W * ux.z};
    zv = Vec{H * uz.x, H * uz.y, H * uz.z};
  } else {
    need(std::isfinite(s.x), which, "x", "must be finite");
    need(std::isfinite(s.y), which, "y", "must be finite");
    need(std::isfinite(s.z), which, "z", "must be finite");
    need(std::isfinite(s.width_x), which, "width_x", "must be finite");
    need(s.width_x > 0.0, which, "width_x", "must be positive");
    c = Vec{s.x, s.y, s.z};
    const double W = s.width_x / 2.0, H = W / s.aspect_ratio;
    xv = Vec{W, 0.0, 0.0};
    zv = Vec{0.0, 0.0, H};
  }
  e[0] = azim(Vec{c.x - xv.x, c.y - xv.y, c.z - xv.z});
  e[1] = azim(Vec{c.x + xv.x, c.y + xv.y, c.z + xv.z});
  e[2] = elev(Vec{c.x - zv.x, c.y - zv.y, c.z - zv.z});
  e[3] = elev(Vec{c.x + zv.x, c.y + zv.y, c.z + zv.z});
  // (false for a NaN edge)
  if (!(-180.0 < e[1] && e[1] < e[0] && e[0] < 180.0 && -90.0 < e[2] && e[2] < e[3] && e[3] < 90.0)) {
    char msg[256];
    std::snprintf(msg, sizeof msg, "%s screen: edges left %g, right %g, bottom %g, top %g are not ordered -180 < right < left "
                  "< 180 and -90 < bottom < top < 90 (a screen across the rear seam or over a pole)", which, e[0], e[1], e[2],
                  e[3]);
    fail_invalid(msg);
  }
}

// SoA arrays of one call.  An output may alias its own input: an element's inputs are read before its outputs are written.
struct ScreenArgs {
  size_t n;
  const double *az, *el;
  const unsigned char *ref, *lock_h, *lock_v;  // NULL: all 1, all 0, all 0
  double *az_out, *el_out;
};

__host__ __device__ inline int apply_element(const Map &m, const ScreenArgs &a, size_t i, double &az, double &el) {
  return apply_one(m, a.az[i], a.el[i], a.ref ? a.ref[i] : 1u, a.lock_h ? a.lock_h[i] : 0u, a.lock_v ? a.lock_v[i] : 0u, az,
                   el);
}

__global__ void __launch_bounds__(256) k_screen_apply(Map m, ScreenArgs a, int *status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  double az, el;
  const int st = apply_element(m, a, i, az, el);
  if (st != 0) az = el = __longlong_as_double(0x7ff8000000000000LL);  // the host form refuses it
  a.az_out[i] = az;
  a.el_out[i] = el;
  if (status) status[i] = st;
}

const size_t kMaxElements = (size_t)1 << 31;

// the host arithmetic both groups share, after a call's own checks of n and its arrays: the call's map
Map make_map_of(const earhip_screen *reference, const earhip_screen *reproduction) {
  double e_ref[4], e_rep[4];
  screen_edges(reference ? *reference : kDefaultScreen, "reference", e_ref);
  if (!reproduction) return identity_map();
  screen_edges(*reproduction, "reproduction", e_rep);
  return make_map(e_ref, e_rep);
}

// the checks and the host arithmetic both forms share: the call's map and arrays
Map make_call(const earhip_screen *reference, const earhip_screen *reproduction, size_t n, const double *az, const double *el,
              const unsigned char *ref, const unsigned char *lock_h, const unsigned char *lock_v, double *az_out,
              double *el_out, ScreenArgs &a) {
  require(n < kMaxElements, "too many elements (at most 2^31 - 1 per call)");
  require(n == 0 || (az && el && az_out && el_out), "azimuth, elevation, azimuth_out and elevation_out must not be NULL");
  a = ScreenArgs{n, az, el, ref, lock_h, lock_v, az_out, el_out};
  return make_map_of(reference, reproduction);
}

// Group V.  SoA arrays of one call; an output may alias its own input, as in ScreenArgs.
struct ScreenCartArgs {
  size_t n;
  const double *in[3];                         // x, y, z
  const unsigned char *ref, *lock_h, *lock_v;  // NULL: all 1, all 0, all 0
  double *out[3];
};

__host__ __device__ inline int apply_cart_element(const Map &m, const ScreenCartArgs &a, size_t i, double out[3]) {
  return apply_cart_one(m, a.in[0][i], a.in[1][i], a.in[2][i], a.ref ? a.ref[i] : 1u, a.lock_h ? a.lock_h[i] : 0u,
                        a.lock_v ? a.lock_v[i] : 0u, out);
}

__global__ void __launch_bounds__(256) k_screen_apply_cartesian(Map m, ScreenCartArgs a, int *status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  double out[3];
  const int st = apply_cart_element(m, a, i, out);
  if (st != EARHIP_OK) out[0] = out[1] = out[2] = __longlong_as_double(0x7ff8000000000000LL);  // the host form refuses it
  for (int k = 0; k < 3; k++) a.out[k][i] = out[k];
  if (status) status[i] = st;
}

Map make_cart_call(const earhip_screen *reference, const earhip_screen *reproduction, size_t n, const double *x, const double *y,
                   const double *z, const unsigned char *ref, const unsigned char *lock_h, const unsigned char *lock_v,
                   double *x_out, double *y_out, double *z_out, ScreenCartArgs &a) {
  require(n < kMaxElements, "too many elements (at most 2^31 - 1 per call)");
  require(n == 0 || (x && y && z && x_out && y_out && z_out), "x, y, z, x_out, y_out and z_out must not be NULL");
  a = ScreenCartArgs{n, {x, y, z}, ref, lock_h, lock_v, {x_out, y_out, z_out}};
  return make_map_of(reference, reproduction);
}

}  // namespace

int earhip_screen_default(earhip_screen *out) {
  return guarded([&] {
    require(out != nullptr, "out must not be NULL");
    *out = kDefaultScreen;
  });
}

int earhip_screen_edges(const earhip_screen *s, double edges[4]) {
  return guarded([&] {
    require(s != nullptr && edges != nullptr, "the screen and edges must not be NULL");
    double e[4];
    screen_edges(*s, "the", e);
    for (int k = 0; k < 4; k++) edges[k] = e[k];
  });
}

int earhip_screen_apply(const earhip_screen *reference, const earhip_screen *reproduction, size_t n, const double *azimuth,
                        const double *elevation, const unsigned char *screen_ref, const unsigned char *lock_horizontal,
                        const unsigned char *lock_vertical, double *azimuth_out, double *elevation_out) {
  return guarded([&] {
    ScreenArgs a;
    const Map m = make_call(reference, reproduction, n, azimuth, elevation, screen_ref, lock_horizontal, lock_vertical,
                            azimuth_out, elevation_out, a);
    for (size_t i = 0; i < n; i++) {
      double az, el;
      if (apply_element(m, a, i, az, el) != 0) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "element %zu: azimuth %g, elevation %g, lock codes %u, %u: the angles must be finite, "
                      "the azimuth within +-2^40 and the elevation within +-90 degrees, a lock code at most 2", i, a.az[i],
                      a.el[i], a.lock_h ? a.lock_h[i] : 0u, a.lock_v ? a.lock_v[i] : 0u);
        fail_invalid(msg);
      }
      a.az_out[i] = az;
      a.el_out[i] = el;
    }
  });
}

int earhip_screen_apply_device(earhip_ctx *ctx, const earhip_screen *reference, const earhip_screen *reproduction, size_t n,
                               const double *azimuth, const double *elevation, const unsigned char *screen_ref,
                               const unsigned char *lock_horizontal, const unsigned char *lock_vertical, double *azimuth_out,
                               double *elevation_out, int *status) {
  return guarded([&] {
    require(ctx != nullptr, "context must not be NULL");
    ScreenArgs a;
    const Map m = make_call(reference, reproduction, n, azimuth, elevation, screen_ref, lock_horizontal, lock_vertical,
                            azimuth_out, elevation_out, a);
    if (n == 0) return;
    ctx->use();
    hipLaunchKernelGGL(k_screen_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, m, a, status);
    EARHIP_HIP(hipGetLastError());
  });
}

int earhip_screen_apply_cartesian(const earhip_screen *reference, const earhip_screen *reproduction, size_t n, const double *x,
                                  const double *y, const double *z, const unsigned char *screen_ref,
                                  const unsigned char *lock_horizontal, const unsigned char *lock_vertical, double *x_out,
                                  double *y_out, double *z_out) {
  return guarded([&] {
    ScreenCartArgs a;
    const Map m = make_cart_call(reference, reproduction, n, x, y, z, screen_ref, lock_horizontal, lock_vertical, x_out, y_out,
                                 z_out, a);
    for (size_t i = 0; i < n; i++) {
      double out[3];
      const int st = apply_cart_element(m, a, i, out);
      if (st != EARHIP_OK) {
        char msg[256];
        if (st == EARHIP_INVALID_ARGUMENT)
          std::snprintf(msg, sizeof msg, "element %zu: position %g, %g, %g, lock codes %u, %u: the coordinates must be finite, "
                        "a lock code at most 2", i, x[i], y[i], z[i],
                        a.lock_h ? a.lock_h[i] : 0u, a.lock_v ? a.lock_v[i] : 0u);
        else
          std::snprintf(msg, sizeof msg, "internal error: element %zu: could not find sector or p out of range (position %g, "
                        "%g, %g)", i, x[i], y[i], z[i]);
        throw Error{st, msg};
      }
      for (int k = 0; k < 3; k++) a.out[k][i] = out[k];
    }
  });
}

int earhip_screen_apply_cartesian_device(earhip_ctx *ctx, const earhip_screen *reference, const earhip_screen *reproduction,
                                         size_t n, const double *x, const double *y, const double *z,
                                         const unsigned char *screen_ref, const unsigned char *lock_horizontal,
                                         const unsigned char *lock_vertical, double *x_out, double *y_out, double *z_out,
                                         int *status) {
  return guarded([&] {
    require(ctx != nullptr, "context must not be NULL");
    ScreenCartArgs a;
    const Map m = make_cart_call(reference, reproduction, n, x, y, z, screen_ref, lock_horizontal, lock_vertical, x_out, y_out,
                                 z_out, a);
    if (n == 0) return;
    ctx->use();
    hipLaunchKernelGGL(k_screen_apply_cartesian, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, m, a, status);
    EARHIP_HIP(hipGetLastError());
  });
}
