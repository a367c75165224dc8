// api_conversion.hip — conversion of Objects positions and extents between polar and Cartesian (earhip group K;
// libear include/ear/conversion.hpp, src/conversion.cpp).  The arithmetic is conversion.h, shared by the host
// forms (libear's free functions take no device, so they are computed on the calling thread) and the device
// forms (one thread per element, enqueued on the context's stream).
#include <cstdio>
#include <string>

#include "common.h"
#include "conversion.h"

using namespace earhip;

namespace {

// SoA arrays of one call.  An output may alias the input of the same component: an element's inputs are all read
// before any of its outputs is written.
struct ConvArgs {
  size_t n;
  const double *in[3];      // x, y, z or azimuth, elevation, distance
  const double *ext_in[3];  // width, height, depth; each may be NULL (0)
  double *out[3];
  double *ext_out[3];  // all NULL: the point form
  bool extent;         // ext_out given
};

// one element; to_polar: Cartesian -> polar
__host__ __device__ inline int convert_one(const ConvArgs &a, bool to_polar, size_t i, double pos[3], double ext[3]) {
  const double p0 = a.in[0][i], p1 = a.in[1][i], p2 = a.in[2][i];
  double e[3];
  for (int k = 0; k < 3; k++) e[k] = a.ext_in[k] ? a.ext_in[k][i] : 0.0;
  int st;
  if (to_polar) {
    st = conv::point_cart_to_polar(p0, p1, p2, pos);
    if (st == EARHIP_OK && a.extent) conv::extent_cart_to_polar(pos[0], pos[1], e, ext);
  } else {
    st = conv::point_polar_to_cart(p0, p1, p2, pos);
    if (st == EARHIP_OK && a.extent) conv::extent_polar_to_cart(p0, p1, e, ext);
  }
  return st;
}

__global__ void __launch_bounds__(256) k_convert(ConvArgs a, int to_polar, int *status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  double pos[3], ext[3];
  const int st = convert_one(a, to_polar != 0, i, pos, ext);
  if (st != EARHIP_OK) {
    // libear returns nothing for such an element: its outputs are NaN, its status says why
    for (int k = 0; k < 3; k++) pos[k] = ext[k] = __longlong_as_double(0x7ff8000000000000LL);
  }
  for (int k = 0; k < 3; k++) a.out[k][i] = pos[k];
  if (a.extent)
    for (int k = 0; k < 3; k++) a.ext_out[k][i] = ext[k];
  if (status) status[i] = st;
}

const size_t kMaxElements = (size_t)1 << 31;

ConvArgs make_args(size_t n, const double *a, const double *b, const double *c, const double *w, const double *h,
                   const double *d, double *oa, double *ob, double *oc, double *ow, double *oh, double *od) {
  require(a && b && c && oa && ob && oc, "the position arrays must not be NULL");
  require(n < kMaxElements, "too many elements (at most 2^31 - 1 per call)");
  const bool extent = ow || oh || od;
  require(!extent || (ow && oh && od), "width_out, height_out and depth_out are all given or all NULL");
  return ConvArgs{n, {a, b, c}, {w, h, d}, {oa, ob, oc}, {ow, oh, od}, extent};
}

int host_convert(bool to_polar, const ConvArgs &a) {
  return guarded([&] {
    for (size_t i = 0; i < a.n; i++) {
      double pos[3], ext[3];
      const int st = convert_one(a, to_polar, i, pos, ext);
      if (st != EARHIP_OK) {
        char msg[256];
        if (st == EARHIP_INVALID_ARGUMENT)
          std::snprintf(msg, sizeof msg, "element %zu: azimuth %g is infinite or beyond +-2^40 degrees", i, a.in[0][i]);
        else
          std::snprintf(msg, sizeof msg, "internal error: element %zu: could not find sector or p out of range "
                        "(position %g, %g, %g)", i, a.in[0][i], a.in[1][i], a.in[2][i]);
        throw Error{st, msg};
      }
      for (int k = 0; k < 3; k++) a.out[k][i] = pos[k];
      if (a.extent)
        for (int k = 0; k < 3; k++) a.ext_out[k][i] = ext[k];
    }
  });
}

int device_convert(earhip_ctx *ctx, bool to_polar, const ConvArgs &a, int *status) {
  return guarded([&] {
    require(ctx != nullptr, "context must not be NULL");
    if (a.n == 0) return;
    ctx->use();
    const unsigned blocks = (unsigned)((a.n + 255) / 256);
    hipLaunchKernelGGL(k_convert, dim3(blocks), dim3(256), 0, ctx->stream, a, to_polar ? 1 : 0, status);
    EARHIP_HIP(hipGetLastError());
  });
}

}  // namespace

int earhip_conversion_to_polar(size_t n, const double *x, const double *y, const double *z, const double *width,
                               const double *height, const double *depth, double *azimuth, double *elevation,
                               double *distance, double *width_out, double *height_out, double *depth_out) {
  ConvArgs a;
  const int st = guarded([&] {
    a = make_args(n, x, y, z, width, height, depth, azimuth, elevation, distance, width_out, height_out, depth_out);
  });
  return st != EARHIP_OK ? st : host_convert(true, a);
}

int earhip_conversion_to_cartesian(size_t n, const double *azimuth, const double *elevation, const double *distance,
                                   const double *width, const double *height, const double *depth, double *x,
                                   double *y, double *z, double *width_out, double *height_out, double *depth_out) {
  ConvArgs a;
  const int st = guarded([&] {
    a = make_args(n, azimuth, elevation, distance, width, height, depth, x, y, z, width_out, height_out, depth_out);
  });
  return st != EARHIP_OK ? st : host_convert(false, a);
}

int earhip_conversion_to_polar_device(earhip_ctx *ctx, size_t n, const double *x, const double *y, const double *z,
                                      const double *width, const double *height, const double *depth,
                                      double *azimuth, double *elevation, double *distance, double *width_out,
                                      double *height_out, double *depth_out, int *status) {
  ConvArgs a;
  const int st = guarded([&] {
    a = make_args(n, x, y, z, width, height, depth, azimuth, elevation, distance, width_out, height_out, depth_out);
  });
  return st != EARHIP_OK ? st : device_convert(ctx, true, a, status);
}

int earhip_conversion_to_cartesian_device(earhip_ctx *ctx, size_t n, const double *azimuth, const double *elevation,
                                          const double *distance, const double *width, const double *height,
                                          const double *depth, double *x, double *y, double *z, double *width_out,
                                          double *height_out, double *depth_out, int *status) {
  ConvArgs a;
  const int st = guarded([&] {
    a = make_args(n, azimuth, elevation, distance, width, height, depth, x, y, z, width_out, height_out, depth_out);
  });
  return st != EARHIP_OK ? st : device_convert(ctx, false, a, status);
}
