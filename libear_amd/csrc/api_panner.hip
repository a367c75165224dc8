// api_panner.hip — (I) the gain-vector producer for Objects content of include/earhip.h: the handle and the entry points.
// The point source panner and the host set-up of a layout are panner.h (plain C++, also compiled on the CPU), the kernels
// panner_kernels.h (a thread per position), extent_kernels.h (a wave per position that is spread, over the plain core of
// extent.h) and objects_kernels.h
// (channelLock, objectDivergence, zoneExclusion).  The HOA decode matrix, which pans the directions of a t-design through
// panner_pan_points, is api_hoa.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "objects_kernels.h"

using namespace earhip;

struct earhip_panner {
  earhip_ctx *ctx;
  PanParams P;
  DevBuf<PanRegion> regions;
  DevBuf<unsigned> missed;
  // the extent panner's point grid: positions [3][n_padded], gains [n_pv][n_padded], per-chunk direction,
  // radius and gain sum (float)
  ExtentTable E;
  DevBuf<float> ext_pos, ext_gains, ext_chunks;
  // what the thread-per-position kernel leaves for the wave-per-position one (grown at first use; a call is
  // cut into launches of at most kExtentBatch positions, so at most that many records)
  DevBuf<ExtentJob> jobs;
  DevBuf<unsigned> job_count;  // [2]: records in jobs, records in ojobs
  // channel lock, divergence and zone exclusion (objects_kernels.h): the layout's tables, and what the front pass leaves
  // for the wave-per-object kernel
  LockTable lock_table;
  ZoneTable zone_table;
  DevBuf<ObjectsJob> ojobs;
  // staging of the host-pointer entry point (grown at first use)
  DevBuf<double> d_in;
  DevBuf<float> d_out;
  PinBuf<double> p_in;
  PinBuf<float> p_out;
  PinBuf<unsigned> p_missed;
  int n_triplets = 0, n_quads = 0, n_ngons = 0, largest_ngon = 0;  // the regions by kind (earhip_panner_self_check)
};

static_assert(kMaxLayoutSpeakers == kObjMaxOut && kMaxLayoutChannels == kMaxPanOut, "layout_registry.h states the kernels' limits");

// guarded(), for bodies that run the host set-up of panner.h: what that refuses becomes the status and the text
template <typename F>
static int guarded_layout(F &&f) {
  return guarded([&] {
    try {
      f();
    } catch (const LayoutFailure &e) {
      throw Error{e.status, e.msg};
    }
  });
}

// Host directions xyz [npos][3] up, one launch over them (launch(d_xyz, d_out): a kernel on the context's stream that
// writes n_out records), the records back; waits.  missed != NULL: the panner's counter is cleared first and read after.
template <typename Out, typename Launch>
static std::vector<Out> over_directions(earhip_panner *p, size_t npos, const double *xyz, size_t n_out, unsigned *missed,
                                        Launch &&launch) {
  hipStream_t s = p->ctx->stream;
  DevBuf<double> d_xyz;
  DevBuf<Out> d_out;
  d_xyz.alloc(3 * npos);
  d_out.alloc(n_out);
  EARHIP_HIP(hipMemcpyAsync(d_xyz.p, xyz, sizeof(double) * 3 * npos, hipMemcpyHostToDevice, s));
  if (missed) EARHIP_HIP(hipMemsetAsync(p->missed.p, 0, sizeof(unsigned), s));
  launch(d_xyz.p, d_out.p);
  EARHIP_HIP(hipGetLastError());
  std::vector<Out> out(n_out);
  EARHIP_HIP(hipMemcpyAsync(out.data(), d_out.p, sizeof(Out) * n_out, hipMemcpyDeviceToHost, s));
  if (missed) EARHIP_HIP(hipMemcpyAsync(missed, p->missed.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  EARHIP_HIP(hipStreamSynchronize(s));
  return out;
}

const PanParams &earhip::panner_params(const earhip_panner *p) { return p->P; }

std::vector<double> earhip::panner_pan_points(earhip_panner *p, size_t npos, const double *xyz, unsigned *missed) {
  const size_t S = p->P.stereo ? 2 : (size_t)p->P.table.n_real;
  return over_directions<double>(p, npos, xyz, npos * S, missed, [&](const double *d_xyz, double *d_pv) {
    hipLaunchKernelGGL(k_pan_points, dim3((unsigned)((npos + 127) / 128)), dim3(128), 0, p->ctx->stream, p->P, npos, d_xyz, d_pv,
                       p->missed.p);
  });
}

// PolarExtent's constructor (src/object_based/polar_extent.cpp:16-50, :96-176): the 37 rows of points (extent_grid,
// extent.h) and the point source panner's gains at each of them (device, one thread per point, double), kept as float
static void build_extent_table(earhip_panner &pn) {
  const ExtentGrid grid = extent_grid();
  const size_t np = grid.points.size(), padded = grid.n_padded, n_chunks = grid.n_chunks;
  require(n_chunks <= (size_t)kExtentMaxChunks, "extent grid too large");
  std::vector<double> xyz(3 * np);
  for (size_t q = 0; q < np; q++) xyz[3 * q] = grid.points[q].x, xyz[3 * q + 1] = grid.points[q].y, xyz[3 * q + 2] = grid.points[q].z;
  const size_t S = pn.P.stereo ? 2 : (size_t)pn.P.table.n_real;
  unsigned missed = 0;
  const std::vector<double> G = panner_pan_points(&pn, np, xyz.data(), &missed);
  if (missed) fail_internal("point source panner: a point of the extent grid was not handled by any region");
  std::vector<float> pos(3 * padded), gains(S * padded, 0.0f);
  for (size_t q = 0; q < padded; q++) {
    const size_t src = std::min(q, np - 1);  // (padding repeats the last point; its gains stay zero)
    for (int k = 0; k < 3; k++) pos[k * padded + q] = (float)xyz[3 * src + k];
  }
  for (size_t q = 0; q < np; q++)
    for (size_t c = 0; c < S; c++) gains[c * padded + q] = (float)G[q * S + c];
  // per chunk: mean direction and angular radius around it (the grid's), float sum of the gain vectors
  const size_t MC = (size_t)kExtentMaxChunks;
  std::vector<float> chunks(3 * MC + MC + MC * kMaxPanOut, 0.0f);
  float *dir = chunks.data(), *rad = dir + 3 * MC, *sum = rad + MC;
  for (size_t c = 0; c < n_chunks; c++) {
    const size_t lo = 64 * c, hi = std::min(lo + 64, np);
    for (size_t k = 0; k < 3; k++) dir[k * MC + c] = grid.chunk_dir[k * n_chunks + c];
    rad[c] = grid.chunk_rad[c];
    for (size_t q = lo; q < hi; q++)
      for (size_t k = 0; k < S; k++) sum[c * kMaxPanOut + k] += gains[k * padded + q];
  }
  pn.ext_pos.alloc(3 * padded);
  pn.ext_gains.alloc(S * padded);
  pn.ext_chunks.alloc(chunks.size());
  EARHIP_HIP(hipMemcpy(pn.ext_pos.p, pos.data(), sizeof(float) * pos.size(), hipMemcpyHostToDevice));
  EARHIP_HIP(hipMemcpy(pn.ext_gains.p, gains.data(), sizeof(float) * gains.size(), hipMemcpyHostToDevice));
  EARHIP_HIP(hipMemcpy(pn.ext_chunks.p, chunks.data(), sizeof(float) * chunks.size(), hipMemcpyHostToDevice));
  pn.E.n_points = (int)np;
  pn.E.n_padded = (int)padded;
  pn.E.n_chunks = (int)n_chunks;
  pn.E.n_pv = (int)S;
  pn.E.xs = pn.ext_pos.p;
  pn.E.ys = pn.ext_pos.p + padded;
  pn.E.zs = pn.ext_pos.p + 2 * padded;
  pn.E.gains = pn.ext_gains.p;
  pn.E.chunk_dir = pn.ext_chunks.p;
  pn.E.chunk_rad = pn.ext_chunks.p + 3 * MC;
  pn.E.chunk_sum = pn.ext_chunks.p + 4 * MC;
}

// with_extent = false: the point source panner alone (the HOA design only pans points: no extent grid to pan,
// upload and wait for on every decode matrix)
int earhip::panner_create(earhip_ctx *ctx, const char *layout, int n_channels, const double *azimuth,
                          const double *elevation, earhip_panner **out, bool with_extent) {
  return guarded_layout([&] {
    require(ctx != nullptr && out != nullptr, "NULL argument");
    const LayoutEntry &L = find_layout(layout);
    require((azimuth == nullptr) == (elevation == nullptr), "azimuth and elevation come together");
    if (azimuth) {
      require(n_channels == L.n, "one position per channel of the layout (LFE channels included)");
      for (int c = 0; c < L.n; c++)
        require(std::isfinite(azimuth[c]) && std::isfinite(elevation[c]), "loudspeaker positions must be finite");
    }
    ctx->use();
    std::unique_ptr<earhip_panner> p(new earhip_panner);
    p->ctx = ctx;
    const std::vector<PanRegion> regions = pan_params(L, azimuth, elevation, p->P);
    const int n_pv = p->P.stereo ? 2 : p->P.table.n_real;
    {  // the outputs as lock candidates (real positions) and their zone groups (nominal positions)
      const std::vector<ObjSpeaker> sp = objects_speakers(L);
      require((int)sp.size() == n_pv, "internal: panner outputs and loudspeakers differ");
      const std::vector<int> rank = objects_lock_rank(sp);
      std::memset(&p->lock_table, 0, sizeof(p->lock_table));
      p->lock_table.n = p->zone_table.n = n_pv;
      for (int k = 0; k < n_pv; k++) {
        const Vec3 v = azimuth ? polar_to_cart(azimuth[sp[k].full], elevation[sp[k].full], 1.0) : sp[k].nominal;
        p->lock_table.rank[k] = rank[k];
        p->lock_table.pos[k][0] = v.x, p->lock_table.pos[k][1] = v.y, p->lock_table.pos[k][2] = v.z;
      }
      objects_zone_groups(sp, p->zone_table.groups);
    }
    for (const PanRegion &R : regions) {
      p->n_triplets += R.kind == 0, p->n_quads += R.kind == 1, p->n_ngons += R.kind == 2;
      if (R.kind == 2) p->largest_ngon = std::max(p->largest_ngon, R.n);
    }
    p->regions.alloc(regions.size());
    EARHIP_HIP(hipMemcpy(p->regions.p, regions.data(), sizeof(PanRegion) * regions.size(), hipMemcpyHostToDevice));
    p->P.table.regions = p->regions.p;
    p->missed.alloc_zero(1, ctx->stream);
    p->p_missed.reserve(1);
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    if (with_extent) build_extent_table(*p);
    *out = p.release();
  });
}

constexpr size_t kExtentBatch = (size_t)1 << 18;  // positions per batch of launches (bounds the job buffer: 115 MB)

// Device pointers; any of the optional arrays may be NULL.  Without lock, divergence and masks: k_pan_objects, then the
// wave-per-position kernel over the jobs it left (nothing is spread at a distance of 1 without an extent,
// extentMod(0, 1) = 0: one launch, no jobs).  With any of them: the front pass, then the two wave-per-object kernels.
static void launch_objects(earhip_panner *p, size_t npos, const double *az, const double *el, const double *dist,
                           const double *width, const double *height, const double *depth, const double *gain,
                           const double *diffuse, const unsigned char *lock, const double *lock_max, const double *divergence,
                           const double *az_range, const uint32_t *excluded, float *direct, float *diffuse_out) {
  hipStream_t s = p->ctx->stream;
  const bool may_spread = dist || width || height || depth, meta = lock || divergence || excluded;
  if (!meta && !may_spread) {
    hipLaunchKernelGGL(k_pan_objects, dim3((unsigned)((npos + 127) / 128)), dim3(128), 0, s, p->P, npos, az, el, dist, width,
                       height, depth, gain, diffuse, direct, diffuse_out, p->missed.p, (ExtentJob *)nullptr,
                       (unsigned *)nullptr);
    EARHIP_HIP(hipGetLastError());
    return;
  }
  p->jobs.reserve(std::min(npos, kExtentBatch));
  if (meta) p->ojobs.reserve(std::min(npos, kExtentBatch));
  p->job_count.reserve(2);
  auto at = [](const double *q, size_t o) { return q ? q + o : q; };
  for (size_t o = 0; o < npos; o += kExtentBatch) {
    const size_t n = std::min(kExtentBatch, npos - o);
    const size_t N = (size_t)p->P.n_full;
    const dim3 front((unsigned)((n + 127) / 128)), waves((unsigned)((n + kExtentWaves - 1) / kExtentWaves)), wg(64 * kExtentWaves);
    EARHIP_HIP(hipMemsetAsync(p->job_count.p, 0, (meta ? 2 : 1) * sizeof(unsigned), s));
    if (meta)
      hipLaunchKernelGGL(k_pan_objects_front, front, dim3(128), 0, s, p->P, p->lock_table, n, az + o, el + o, at(dist, o),
                         at(width, o), at(height, o), at(depth, o), at(gain, o), at(diffuse, o), lock ? lock + o : lock,
                         at(lock_max, o), at(divergence, o), at(az_range, o), excluded ? excluded + o : excluded, may_spread,
                         direct + o * N, diffuse_out + o * N, p->missed.p, p->jobs.p, p->job_count.p, p->ojobs.p);
    else
      hipLaunchKernelGGL(k_pan_objects, front, dim3(128), 0, s, p->P, n, az + o, el + o, at(dist, o), at(width, o),
                         at(height, o), at(depth, o), at(gain, o), at(diffuse, o), direct + o * N, diffuse_out + o * N,
                         p->missed.p, p->jobs.p, p->job_count.p);
    EARHIP_HIP(hipGetLastError());
    // (launched for the worst case — every position a job of that kind; surplus waves leave at once)
    if (may_spread) {
      hipLaunchKernelGGL(k_pan_objects_extent, waves, wg, 0, s, p->P, p->E, p->jobs.p, p->job_count.p, at(gain, o),
                         at(diffuse, o), direct + o * N, diffuse_out + o * N);
      EARHIP_HIP(hipGetLastError());
    }
    if (meta) {
      hipLaunchKernelGGL(k_pan_objects_meta, waves, wg, 0, s, p->P, p->E, p->zone_table, p->ojobs.p, p->job_count.p + 1,
                         at(width, o), at(height, o), at(depth, o), at(gain, o), at(diffuse, o), may_spread, direct + o * N,
                         diffuse_out + o * N, p->missed.p);
      EARHIP_HIP(hipGetLastError());
    }
  }
}

extern "C" {

int earhip_panner_create(earhip_ctx *ctx, const char *layout, earhip_panner **out) {
  return panner_create(ctx, layout, 0, nullptr, nullptr, out, true);
}

int earhip_panner_create_positions(earhip_ctx *ctx, const char *layout, int n_channels, const double *azimuth,
                                   const double *elevation, earhip_panner **out) {
  return panner_create(ctx, layout, n_channels, azimuth, elevation, out, true);
}

int earhip_panner_destroy(earhip_panner *p) {
  return guarded([&] {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    delete p;
  });
}

int earhip_panner_num_channels(const earhip_panner *p, int *n_channels) {
  return guarded([&] {
    require(p != nullptr && n_channels != nullptr, "NULL argument");
    *n_channels = p->P.n_full;
  });
}

// Does every direction land in a region, with unit power, and does a loudspeaker's own direction give that loudspeaker
// alone?  One launch over the t-design and the loudspeakers' real directions (the lock table's: the panner's outputs at
// the positions it was created with); a set-up-time call, it synchronises.
int earhip_panner_self_check(earhip_panner *p, earhip_panner_report *report) {
  return guarded([&] {
    require(p != nullptr && report != nullptr, "NULL argument");
    p->ctx->use();
    const int n_out = p->lock_table.n;
    std::vector<double> xyz = tdesign_directions((size_t)n_out);
    const int n_dirs = (int)(xyz.size() / 3), n_design = n_dirs - n_out;
    for (int k = 0; k < n_out; k++)
      for (int q = 0; q < 3; q++) xyz[3 * (size_t)(n_design + k) + q] = p->lock_table.pos[k][q];
    const int n_wg = (n_dirs + kSelfCheckThreads - 1) / kSelfCheckThreads;
    const std::vector<SelfCheckPartial> partial = over_directions<SelfCheckPartial>(
        p, (size_t)n_dirs, xyz.data(), (size_t)n_wg, nullptr, [&](const double *d_xyz, SelfCheckPartial *d_partial) {
          hipLaunchKernelGGL(k_pan_self_check, dim3((unsigned)n_wg), dim3(kSelfCheckThreads), 0, p->ctx->stream, p->P, n_dirs,
                             n_design, d_xyz, d_partial);
        });
    std::memset(report, 0, sizeof(*report));
    report->n_directions = n_dirs;
    report->min_own_gain = 2.0;
    for (const SelfCheckPartial &w : partial) {
      report->missed += w.missed;
      report->max_power_error = std::max(report->max_power_error, w.max_power_error);
      report->min_own_gain = std::min(report->min_own_gain, w.min_own_gain);
    }
    report->n_regions = p->P.table.n_regions;
    report->n_triplets = p->n_triplets;
    report->n_quads = p->n_quads;
    report->n_ngons = p->n_ngons;
    report->largest_ngon = p->largest_ngon;
  });
}

int earhip_panner_missed(earhip_panner *p, unsigned *count) {
  return guarded([&] {
    require(p != nullptr && count != nullptr, "NULL argument");
    earhip_ctx *ctx = p->ctx;
    ctx->use();
    EARHIP_HIP(hipMemcpyAsync(p->p_missed.p, p->missed.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    *count = *p->p_missed.p;
  });
}

int earhip_panner_calculate_objects_device(earhip_panner *p, size_t npos, const double *azimuth, const double *elevation,
                                           const double *distance, const double *width, const double *height,
                                           const double *depth, const double *gain, const double *diffuse,
                                           const unsigned char *channel_lock, const double *lock_max_distance,
                                           const double *divergence, const double *azimuth_range, const uint32_t *excluded,
                                           float *direct, float *diffuse_out) {
  return guarded([&] {
    require(p != nullptr, "panner must not be NULL");
    require(azimuth && elevation && direct && diffuse_out, "azimuth, elevation and the outputs must not be NULL");
    require(npos < ((size_t)1 << 28), "too many positions");
    p->ctx->use();
    // the counter of positions no region takes means "this call" (earhip_panner_missed reads it) — an empty call too
    EARHIP_HIP(hipMemsetAsync(p->missed.p, 0, sizeof(unsigned), p->ctx->stream));
    if (npos == 0) return;
    launch_objects(p, npos, azimuth, elevation, distance, width, height, depth, gain, diffuse, channel_lock, lock_max_distance,
                   divergence, azimuth_range, excluded, direct, diffuse_out);
  });
}

int earhip_panner_calculate_extent_device(earhip_panner *p, size_t npos, const double *azimuth, const double *elevation,
                                          const double *distance, const double *width, const double *height,
                                          const double *depth, const double *gain, const double *diffuse, float *direct,
                                          float *diffuse_out) {
  return earhip_panner_calculate_objects_device(p, npos, azimuth, elevation, distance, width, height, depth, gain, diffuse, nullptr,
                                                nullptr, nullptr, nullptr, nullptr, direct, diffuse_out);
}

int earhip_panner_calculate_device(earhip_panner *p, size_t npos, const double *azimuth, const double *elevation,
                                   const double *distance, const double *gain, const double *diffuse, float *direct,
                                   float *diffuse_out) {
  return earhip_panner_calculate_extent_device(p, npos, azimuth, elevation, distance, nullptr, nullptr, nullptr, gain, diffuse,
                                               direct, diffuse_out);
}

int earhip_panner_calculate_objects(earhip_panner *p, size_t npos, const double *azimuth, const double *elevation,
                                    const double *distance, const double *width, const double *height, const double *depth,
                                    const double *gain, const double *diffuse, const unsigned char *channel_lock,
                                    const double *lock_max_distance, const double *divergence, const double *azimuth_range,
                                    const uint32_t *excluded, float *direct, float *diffuse_out) {
  return guarded([&] {
    require(npos < ((size_t)1 << 28), "too many positions");
    // (the values first: they are refused whatever the panner is)
    for (size_t i = 0; (divergence || lock_max_distance || azimuth_range) && i < npos; i++) {
      const std::string at = "[" + std::to_string(i) + "]";
      if (divergence && !(divergence[i] >= 0.0 && divergence[i] <= 1.0)) fail_invalid("divergence" + at + " must be in [0, 1]");
      if (lock_max_distance && !(lock_max_distance[i] >= 0.0))
        fail_invalid("lock_max_distance" + at + " must not be negative or NaN");
      if (azimuth_range && !std::isfinite(azimuth_range[i])) fail_invalid("azimuth_range" + at + " must be finite");
    }
    require(p != nullptr, "panner must not be NULL");
    require(azimuth && elevation && direct && diffuse_out, "azimuth, elevation and the outputs must not be NULL");
    const size_t N = (size_t)p->P.n_full;
    for (size_t i = 0; excluded && i < npos; i++)
      if (N < 32 && (excluded[i] >> N) != 0)
        fail_invalid("excluded[" + std::to_string(i) + "] has a bit set beyond the layout's " + std::to_string(N) + " channels");
    if (npos == 0) return;
    earhip_ctx *ctx = p->ctx;
    ctx->use();
    // staging: 8 arrays of doubles; with any of the five Objects arrays 11, then the lock flags and the masks in whole doubles
    const bool objects = channel_lock || lock_max_distance || divergence || azimuth_range || excluded;
    const size_t kIn = objects ? 11 : 8;
    const size_t lock_at = kIn * npos, mask_at = lock_at + (npos + 7) / 8, total = objects ? mask_at + (npos + 1) / 2 : lock_at;
    p->p_in.reserve(total);
    p->d_in.reserve(total);
    p->p_out.reserve(2 * npos * N);
    p->d_out.reserve(2 * npos * N);
    const double *src[11] = {azimuth, elevation, distance, width, height, depth, gain, diffuse, lock_max_distance, divergence,
                             azimuth_range};
    const double *dev[11] = {};
    for (size_t k = 0; k < kIn; k++) {
      if (src[k]) std::memcpy(p->p_in.p + k * npos, src[k], sizeof(double) * npos);
      dev[k] = src[k] ? p->d_in.p + k * npos : nullptr;
    }
    if (channel_lock) std::memcpy(p->p_in.p + lock_at, channel_lock, npos);
    if (excluded) std::memcpy(p->p_in.p + mask_at, excluded, sizeof(uint32_t) * npos);
    const unsigned char *dev_lock = channel_lock ? reinterpret_cast<const unsigned char *>(p->d_in.p + lock_at) : nullptr;
    const uint32_t *dev_mask = excluded ? reinterpret_cast<const uint32_t *>(p->d_in.p + mask_at) : nullptr;
    EARHIP_HIP(hipMemcpyAsync(p->d_in.p, p->p_in.p, sizeof(double) * total, hipMemcpyHostToDevice, ctx->stream));
    EARHIP_HIP(hipMemsetAsync(p->missed.p, 0, sizeof(unsigned), ctx->stream));
    launch_objects(p, npos, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], dev_lock, dev[8], dev[9], dev[10],
                   dev_mask, p->d_out.p, p->d_out.p + npos * N);
    EARHIP_HIP(hipMemcpyAsync(p->p_out.p, p->d_out.p, sizeof(float) * 2 * npos * N, hipMemcpyDeviceToHost, ctx->stream));
    EARHIP_HIP(hipMemcpyAsync(p->p_missed.p, p->missed.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(direct, p->p_out.p, sizeof(float) * npos * N);
    std::memcpy(diffuse_out, p->p_out.p + npos * N, sizeof(float) * npos * N);
    // (the reference dereferences an empty optional when no region takes a position: undefined there,
    // an error here)
    if (*p->p_missed.p != 0) fail_internal("point source panner: a position was not handled by any region");
  });
}

int earhip_panner_calculate_extent(earhip_panner *p, size_t npos, const double *azimuth, const double *elevation,
                                   const double *distance, const double *width, const double *height, const double *depth,
                                   const double *gain, const double *diffuse, float *direct, float *diffuse_out) {
  return earhip_panner_calculate_objects(p, npos, azimuth, elevation, distance, width, height, depth, gain, diffuse, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, direct, diffuse_out);
}

int earhip_panner_calculate(earhip_panner *p, size_t npos, const double *azimuth, const double *elevation,
                            const double *distance, const double *gain, const double *diffuse, float *direct,
                            float *diffuse_out) {
  return earhip_panner_calculate_extent(p, npos, azimuth, elevation, distance, nullptr, nullptr, nullptr, gain, diffuse, direct,
                                        diffuse_out);
}

int earhip_objects_lock_priority(const char *layout, int *order) {
  return guarded_layout([&] {
    require(order != nullptr, "NULL argument");
    const std::vector<ObjSpeaker> sp = objects_speakers(find_layout(layout));
    const std::vector<int> rank = objects_lock_rank(sp);
    for (size_t s = 0; s < sp.size(); s++) order[rank[s]] = sp[s].full;
  });
}

int earhip_objects_excluded_channels(const char *layout, int n_zones, const earhip_exclusion_zone *zones, uint32_t *mask) {
  return guarded_layout([&] {
    require(mask != nullptr && n_zones >= 0 && (zones != nullptr || n_zones == 0), "NULL argument");
    *mask = objects_excluded_channels(objects_speakers(find_layout(layout)), n_zones, zones);
  });
}

int earhip_objects_zone_downmix(const char *layout, uint32_t mask, double *matrix) {
  return guarded_layout([&] {
    require(matrix != nullptr, "NULL argument");
    objects_zone_downmix(find_layout(layout), mask, matrix);
  });
}

}  // extern "C"
