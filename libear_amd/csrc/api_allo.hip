// api_allo.hip — the allocentric (Cartesian) point-source panner for Objects (earhip group T; libear has only a stub,
// AllocentricPanner::handle returns boost::none).  The handle is host data: the layout's loudspeakers on the cube, snapped
// per axis (allo_table.h or the caller's positions).  The arithmetic is allo.h, shared by the host form (computed on the
// calling thread, like the host forms of groups K and Q) and the device form (allo_kernels.h: a wave per 64 positions,
// enqueued on the context's stream).  Group U, on the same handle: channelLock, Cartesian objectDivergence and extent
// (allo_objects.h, the core of both forms; allo_objects_kernels.h, lanes over (object, loudspeaker)).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "allo.h"
#include "allo_kernels.h"
#include "allo_objects.h"
#include "allo_objects_kernels.h"
#include "allo_table.h"
#include "layout_registry.h"

using namespace earhip;
using namespace earhip::allo;

struct earhip_allo {
  Table t;
};

namespace {

const size_t kMaxElements = (size_t)1 << 31;

bool is_bs2051(const char *name) {
  for (int i = 0; i < kNumLayouts; i++)
    if (std::strcmp(kLayouts[i].name, name) == 0) return true;
  return false;
}

// One axis: the loudspeakers' coordinates sorted ascending and walked; a value within kSnap of the first value of the
// current group takes that first value.
void snap_axis(double *coord, int n, uint32_t real) {
  std::vector<int> order;
  for (int c = 0; c < n; c++)
    if ((real >> c) & 1u) order.push_back(c);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return coord[a] < coord[b]; });
  double first = 0.0;
  for (size_t k = 0; k < order.size(); k++) {
    double &v = coord[order[k]];
    if (k > 0 && v - first <= kSnap) v = first;
    else first = v;
  }
}

// the handle of a layout whose loudspeakers stand at (x, y, z), one per channel of the full layout (LFE entries ignored)
std::unique_ptr<earhip_allo> make_handle(const LayoutEntry &L, const double *x, const double *y, const double *z) {
  require(L.n >= 1 && L.n <= kMaxChannels, "a layout has 1 to 32 channels");
  std::unique_ptr<earhip_allo> a(new earhip_allo);
  Table &t = a->t;
  std::memset(&t, 0, sizeof t);
  t.n = L.n;
  for (int c = 0; c < L.n; c++) {
    if (L.channels[c].is_lfe) continue;
    if (!(std::isfinite(x[c]) && std::isfinite(y[c]) && std::isfinite(z[c])))
      fail_invalid("channel " + std::to_string(c) + " (" + L.channels[c].name + "): the position must be finite");
    t.real |= 1u << c;
    t.x[c] = x[c], t.y[c] = y[c], t.z[c] = z[c];
  }
  require(t.real != 0, "a layout has at least one channel that is not an LFE");
  snap_axis(t.x, t.n, t.real);
  snap_axis(t.y, t.n, t.real);
  snap_axis(t.z, t.n, t.real);
  for (int c = 0; c < t.n; c++)
    for (int o = 0; o < c; o++)
      if (((t.real >> c) & 1u) && ((t.real >> o) & 1u) && t.x[c] == t.x[o] && t.y[c] == t.y[o] && t.z[c] == t.z[o])
        fail_invalid(std::string("channels ") + L.channels[o].name + " and " + L.channels[c].name + " stand at the same position");
  return a;
}

void check_arrays(const earhip_allo *a, size_t n, const void *x, const void *y, const void *z, const void *diffuse,
                  const void *direct, const void *diffuse_out) {
  require(a != nullptr, "the handle must not be NULL");
  require(n < kMaxElements, "too many elements (at most 2^31 - 1 per call)");
  require(diffuse_out != nullptr || diffuse == nullptr, "diffuse_out may be NULL only when diffuse is NULL");
  require(n == 0 || (x && y && z && direct), "x, y, z and direct must not be NULL");
}

}  // namespace

extern "C" {

int earhip_allo_create(const char *layout, earhip_allo **out) {
  return guarded([&] {
    require(out != nullptr, "NULL argument");
    const LayoutEntry &L = find_layout(layout);
    if (!is_bs2051(layout))
      throw Error{EARHIP_NOT_IMPLEMENTED, std::string("no allocentric loudspeaker table for layout ") + layout +
                                              ": give the positions (earhip_allo_create_positions)"};
    double x[kMaxChannels] = {0}, y[kMaxChannels] = {0}, z[kMaxChannels] = {0};
    for (int c = 0; c < L.n; c++) {
      if (L.channels[c].is_lfe) continue;
      const AlloPosition *p = allo_position(L.name, L.channels[c].name);
      if (!p) fail_internal(std::string("no allocentric position for channel ") + L.channels[c].name);
      x[c] = p->x, y[c] = p->y, z[c] = p->z;
    }
    *out = make_handle(L, x, y, z).release();
  });
}

int earhip_allo_create_positions(const char *layout, int n_channels, const double *x, const double *y, const double *z,
                                 earhip_allo **out) {
  return guarded([&] {
    require(out != nullptr && x != nullptr && y != nullptr && z != nullptr, "NULL argument");
    const LayoutEntry &L = find_layout(layout);
    require(n_channels == L.n, "one position per channel of the layout (LFE channels included)");
    *out = make_handle(L, x, y, z).release();
  });
}

int earhip_allo_destroy(earhip_allo *a) {
  return guarded([&] { delete a; });
}

int earhip_allo_num_channels(const earhip_allo *a, int *n_channels) {
  return guarded([&] {
    require(a != nullptr && n_channels != nullptr, "NULL argument");
    *n_channels = a->t.n;
  });
}

int earhip_allo_positions(const earhip_allo *a, double *xyz) {
  return guarded([&] {
    require(a != nullptr && xyz != nullptr, "NULL argument");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int c = 0; c < a->t.n; c++) {
      const bool real = (a->t.real >> c) & 1u;
      xyz[3 * c] = real ? a->t.x[c] : nan, xyz[3 * c + 1] = real ? a->t.y[c] : nan, xyz[3 * c + 2] = real ? a->t.z[c] : nan;
    }
  });
}

int earhip_allo_excluded_channels(const earhip_allo *a, int n_zones, const earhip_exclusion_zone *zones, uint32_t *mask) {
  return guarded([&] {
    require(a != nullptr && mask != nullptr && n_zones >= 0 && (zones != nullptr || n_zones == 0), "NULL argument");
    const double tol = 1e-6;
    const Table &t = a->t;
    uint32_t m = 0;
    for (int k = 0; k < n_zones; k++) {
      const earhip_exclusion_zone &zn = zones[k];
      if (!zn.cartesian)
        fail_invalid("zone " + std::to_string(k) + " is polar: the allocentric panner takes Cartesian zones "
                     "(earhip_objects_excluded_channels takes polar ones)");
      for (int c = 0; c < t.n; c++)
        if (((t.real >> c) & 1u) && zn.min_x - tol < t.x[c] && t.x[c] < zn.max_x + tol && zn.min_y - tol < t.y[c] &&
            t.y[c] < zn.max_y + tol && zn.min_z - tol < t.z[c] && t.z[c] < zn.max_z + tol)
          m |= 1u << c;
    }
    *mask = m;
  });
}

int earhip_allo_calculate(const earhip_allo *a, size_t n, const double *x, const double *y, const double *z,
                          const double *gain, const double *diffuse, const uint32_t *excluded, float *direct,
                          float *diffuse_out) {
  return guarded([&] {
    check_arrays(a, n, x, y, z, diffuse, direct, diffuse_out);
    const Table &t = a->t;
    const uint32_t beyond = t.n >= 32 ? 0u : ~0u << t.n;
    for (size_t i = 0; i < n; i++) {
      const double g = gain ? gain[i] : 1.0, d = diffuse ? diffuse[i] : 0.0;
      const uint32_t mask = excluded ? excluded[i] : 0u;
      if (!position_valid(x[i], y[i], z[i], g, d) || (mask & beyond)) {
        char msg[320];
        std::snprintf(msg, sizeof msg, "element %zu: x %g, y %g, z %g, gain %g, diffuse %g, excluded 0x%x: the position and the "
                      "gain must be finite, the diffuse within [0, 1] and the mask within the layout's %d channels",
                      i, x[i], y[i], z[i], g, d, (unsigned)mask, t.n);
        fail_invalid(msg);
      }
      Gains hit;
      pan_position(t, x[i], y[i], z[i], mask, hit);
      write_row(t, hit, g, direct_factor(d), direct + i * (size_t)t.n);
      if (diffuse_out) write_row(t, hit, g, diffuse_factor(d), diffuse_out + i * (size_t)t.n);
    }
  });
}

int earhip_allo_calculate_device(earhip_ctx *ctx, const earhip_allo *a, size_t n, const double *x_dev, const double *y_dev,
                                 const double *z_dev, const double *gain_dev, const double *diffuse_dev,
                                 const uint32_t *excluded_dev, float *direct_dev, float *diffuse_out_dev, int *status_dev) {
  return guarded([&] {
    require(ctx != nullptr, "context must not be NULL");
    check_arrays(a, n, x_dev, y_dev, z_dev, diffuse_dev, direct_dev, diffuse_out_dev);
    if (n == 0) return;
    ctx->use();
    const size_t per_wg = (size_t)64 * kTileWaves;
    hipLaunchKernelGGL(k_allo_calculate, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(64 * kTileWaves),
                       tile_lds_bytes(a->t.n), ctx->stream, a->t, n, x_dev, y_dev, z_dev, gain_dev, diffuse_dev, excluded_dev,
                       direct_dev, diffuse_out_dev, status_dev);
    EARHIP_HIP(hipGetLastError());
  });
}

int earhip_allo_lock_priority(const earhip_allo *a, int *order) {
  return guarded([&] {
    require(a != nullptr && order != nullptr, "NULL argument");
    const Extras e = make_extras(a->t);
    for (int k = 0; k < e.n_order; k++) order[k] = e.order[k];
  });
}

int earhip_allo_calculate_objects(const earhip_allo *a, size_t n, const double *x, const double *y, const double *z,
                                  const double *width, const double *height, const double *depth, const double *gain,
                                  const double *diffuse, const unsigned char *channel_lock, const double *lock_max_distance,
                                  const double *divergence, const double *position_range, const uint32_t *excluded,
                                  float *direct, float *diffuse_out) {
  return guarded([&] {
    check_arrays(a, n, x, y, z, diffuse, direct, diffuse_out);
    const Table &t = a->t;
    const Extras e = make_extras(t);
    const uint32_t beyond = t.n >= 32 ? 0u : ~0u << t.n;
    for (size_t i = 0; i < n; i++) {
      const double sw = width ? width[i] : 0.0, sh = height ? height[i] : 0.0, sd = depth ? depth[i] : 0.0;
      const double g = gain ? gain[i] : 1.0, d = diffuse ? diffuse[i] : 0.0;
      const bool lock = channel_lock ? channel_lock[i] != 0 : false;
      const double maxd = lock_max_distance ? lock_max_distance[i] : HUGE_VAL;
      const double v = divergence ? divergence[i] : 0.0, r = position_range ? position_range[i] : 0.0;
      const uint32_t mask = excluded ? excluded[i] : 0u;
      if (!position_valid(x[i], y[i], z[i], g, d) || !objects_valid(sw, sh, sd, maxd, v, r) || (mask & beyond)) {
        char msg[640];
        std::snprintf(msg, sizeof msg, "element %zu: x %g, y %g, z %g, width %g, height %g, depth %g, gain %g, diffuse %g, "
                      "maxDistance %g, divergence %g, positionRange %g, excluded 0x%x: the position and the gain must be finite, "
                      "the sizes and the positionRange finite and not negative, the maxDistance not negative, the diffuse and "
                      "the divergence within [0, 1] and the mask within the layout's %d channels",
                      i, x[i], y[i], z[i], sw, sh, sd, g, d, maxd, v, r, (unsigned)mask, t.n);
        fail_invalid(msg);
      }
      Object o;
      prepare_object(t, e, x[i], y[i], z[i], sw, sh, sd, lock, maxd, v, r, mask, o);
      double w[kMaxChannels][3], G[kMaxChannels][3], sum[3] = {0.0, 0.0, 0.0}, norm[3];
      for (int c = 0; c < t.n; c++) {
        channel_terms(t, e, o, c, w[c], G[c]);
        for (int k = 0; k < 3; k++) sum[k] += G[c][k] * G[c][k];
      }
      for (int k = 0; k < 3; k++) norm[k] = sqrt(sum[k]);
      for (int c = 0; c < t.n; c++) {
        const double gc = combine(o, w[c], G[c], norm);
        direct[i * (size_t)t.n + c] = row_value(gc, g, direct_factor(d));
        if (diffuse_out) diffuse_out[i * (size_t)t.n + c] = row_value(gc, g, diffuse_factor(d));
      }
    }
  });
}

int earhip_allo_calculate_objects_device(earhip_ctx *ctx, const earhip_allo *a, size_t n, const double *x_dev,
                                         const double *y_dev, const double *z_dev, const double *width_dev,
                                         const double *height_dev, const double *depth_dev, const double *gain_dev,
                                         const double *diffuse_dev, const unsigned char *channel_lock_dev,
                                         const double *lock_max_distance_dev, const double *divergence_dev,
                                         const double *position_range_dev, const uint32_t *excluded_dev, float *direct_dev,
                                         float *diffuse_out_dev, int *status_dev) {
  return guarded([&] {
    require(ctx != nullptr, "context must not be NULL");
    check_arrays(a, n, x_dev, y_dev, z_dev, diffuse_dev, direct_dev, diffuse_out_dev);
    if (n == 0) return;
    ctx->use();
    const size_t per_wg = (size_t)objects_per_workgroup(a->t.n);
    hipLaunchKernelGGL(k_allo_objects, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(kObjectsThreads), 0, ctx->stream, a->t,
                       make_extras(a->t), objects_log2_width(a->t.n), n, x_dev, y_dev, z_dev, width_dev, height_dev, depth_dev,
                       gain_dev, diffuse_dev, channel_lock_dev, lock_max_distance_dev, divergence_dev, position_range_dev,
                       excluded_dev, direct_dev, diffuse_out_dev, status_dev);
    EARHIP_HIP(hipGetLastError());
  });
}

}  // extern "C"
