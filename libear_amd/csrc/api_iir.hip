// api_iir.hip — group O of include/earhip.h: a biquad filter matrix on planar float32 rows in device memory (crossovers, bass
// management, EQ).  The kernels: iir_kernels.h; the maths they share with the CPU tests: iir.h.
#include <algorithm>
#include <memory>

#include "bus_stage.h"
#include "iir_kernels.h"

using namespace earhip;

struct earhip_iir : BusStage {
  static constexpr StageWords words = {
      "iir must not be NULL",
      "device pointers must not be NULL", "device pointers must not be NULL",
      "stride too small", "stride too small",
      "in and out must not be NULL", "in and out must not be NULL",
      "a row pointer is NULL", "a row pointer is NULL"};
  earhip_iir() { noun = "IIR stage", room_name = "max_samples"; }
  int R = 0;
  int max_state = 0;    // the largest 2 S of any route
  int most_routes = 0;  // the most routes of one output: picks pass 2's waves
  unsigned cap = 0;              // chunks of e and start per route
  unsigned long long clock = 0;  // samples since create / reset
  // everything a process call touches, made at create
  DevBuf<IirRouteDev> routes;    // [R]
  DevBuf<double> Q;              // [R][kIirPowers][kIirMat]
  DevBuf<double> e, start;       // [R][cap][16] each
  PingPong<double> state;        // [2][R][16]
  DevBuf<int> out_first, out_routes;
  HostRows host;                 // [n_in][max_samples], [n_out][max_samples]

  // everything the handle holds on the device but the few route tables: chunk states, carried states, matrix powers, and the
  // host form's rows
  size_t scratch_bytes() const {
    return sizeof(double) * (e.n + start.n + state.buf.n + Q.n) + sizeof(float) * (host.d_in.n + host.d_out.n);
  }

  void zero() override {
    state.zero(ctx->stream);
    clock = 0;
  }

  void launch(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    const IirPlan p = iir_plan(clock, n);
    if (p.nchunks > cap) fail_internal("an IIR launch of more chunks than its scratch holds");
    IirArgs a;
    a.in = in, a.in_stride = in_stride, a.out = out, a.out_stride = out_stride;
    a.n = p.n, a.off0 = p.off0, a.nchunks = p.nchunks, a.cap = cap;
    a.routes = routes.p, a.Q = Q.p, a.e = e.p, a.start = start.p;
    a.state_in = state.in(), a.state_out = state.out();
    a.out_first = out_first.p, a.out_routes = out_routes.p;
    if (p.nchunks >= 2 && max_state > 0) {
      hipLaunchKernelGGL(k_iir_pass1, dim3((p.nchunks - 1 + 63) / 64, (unsigned)R), dim3(64), 0, ctx->stream, a);
      hipLaunchKernelGGL(k_iir_propagate, dim3((unsigned)R), dim3(64 * kIirScanWaves), 0, ctx->stream, a);
    }
    const dim3 grid((p.nchunks + 63) / 64, (unsigned)n_out);
    if (most_routes <= 1)
      hipLaunchKernelGGL(k_iir_pass2<1>, grid, dim3(64), 0, ctx->stream, a);
    else if (most_routes <= 2)
      hipLaunchKernelGGL(k_iir_pass2<2>, grid, dim3(128), 0, ctx->stream, a);
    else
      hipLaunchKernelGGL(k_iir_pass2<4>, grid, dim3(256), 0, ctx->stream, a);
    EARHIP_HIP(hipGetLastError());
    clock += n;
    state.flip();
  }

  void feed(size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride) override {
    for_each_launch(nsamples, kIirMaxLaunch, [&](size_t at, size_t n, size_t) {
      launch(n, in + at, in_stride, out + at, out_stride);
      return n;
    });
  }
};

extern "C" {

int earhip_iir_create(earhip_ctx *ctx, const earhip_iir_config *cfg, earhip_iir **out) {
  return guarded([&] {
    require(cfg != nullptr, "config must not be NULL");
    if (const char *why = iir_check_shape(cfg->n_in, cfg->n_out, cfg->n_routes, cfg->max_samples)) fail_invalid(why);
    require(cfg->routes != nullptr, "routes must not be NULL");
    const int R = cfg->n_routes;
    std::vector<IirRoute> routes((size_t)R);
    for (int r = 0; r < R; r++) {
      const earhip_iir_route &s = cfg->routes[r];
      IirRoute &d = routes[(size_t)r];
      d.in = s.in, d.out = s.out, d.gain = s.gain, d.S = s.n_sections;
      for (int i = 0; i < kIirMaxSections; i++)
        for (int j = 0; j < 5; j++) d.c[i][j] = (i < s.n_sections && s.n_sections <= kIirMaxSections) ? s.coeffs[i][j] : 0.0;
      if (const char *why = iir_check_route(d, cfg->n_in, cfg->n_out)) fail_invalid(why);
    }
    require(ctx != nullptr && out != nullptr, "ctx and out must not be NULL");
    ctx->use();
    std::unique_ptr<earhip_iir> iir(new earhip_iir);
    iir->ctx = ctx;
    iir->n_in = cfg->n_in, iir->n_out = cfg->n_out, iir->R = R;
    iir->room = cfg->max_samples;
    const size_t longest = std::min(cfg->max_samples, kIirMaxLaunch);
    iir->cap = (unsigned)((longest + kIirChunk - 1) / kIirChunk + 1);  // (a launch may start anywhere in a chunk)
    std::vector<IirRouteDev> dev((size_t)R);
    std::vector<double> Q((size_t)R * kIirPowers * kIirMat);
    std::vector<int> first((size_t)cfg->n_out + 1, 0), order;
    for (int r = 0; r < R; r++) {
      const IirRoute &s = routes[(size_t)r];
      IirRouteDev &d = dev[(size_t)r];
      d.in = s.in, d.out = s.out, d.S = s.S, d.pad = 0, d.gain = s.gain;
      for (int i = 0; i < kIirMaxSections; i++)
        for (int j = 0; j < 5; j++) d.k.c[i][j] = s.c[i][j];
      iir_state_powers(s.c, s.S, &Q[(size_t)r * kIirPowers * kIirMat]);
      iir->max_state = std::max(iir->max_state, 2 * s.S);
    }
    for (int o = 0; o < cfg->n_out; o++) {
      for (int r = 0; r < R; r++)
        if (routes[(size_t)r].out == o) order.push_back(r);
      first[(size_t)o + 1] = (int)order.size();
      iir->most_routes = std::max(iir->most_routes, first[(size_t)o + 1] - first[(size_t)o]);
    }
    iir->routes.upload(dev);
    iir->Q.upload(Q);
    iir->out_first.upload(first);
    iir->out_routes.upload(order);
    iir->e.alloc((size_t)R * iir->cap * kIirMaxState);
    iir->start.alloc((size_t)R * iir->cap * kIirMaxState);
    iir->state.alloc((size_t)R * kIirMaxState);
    iir->host.alloc((size_t)cfg->n_in * cfg->max_samples, (size_t)cfg->n_out * cfg->max_samples);
    stage_ready(iir, out);
  });
}

int earhip_iir_destroy(earhip_iir *iir) { return stage_destroy(iir); }
int earhip_iir_reset(earhip_iir *iir) { return stage_reset(iir); }

int earhip_iir_info(const earhip_iir *iir, int info[6]) {
  return guarded([&] {
    require(iir != nullptr && info != nullptr, "iir and info must not be NULL");
    info[0] = kIirChunk, info[1] = kIirScanLanes, info[2] = kIirScanGroups, info[3] = iir->R, info[4] = iir->max_state;
    info[5] = (int)std::min<size_t>(iir->scratch_bytes(), 0x7fffffff);
  });
}

int earhip_iir_process_device(earhip_iir *iir, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                              size_t out_stride) {
  return guarded([&] { stage_process_device(iir, nsamples, in_dev, in_stride, out_dev, out_stride); });
}

int earhip_iir_process(earhip_iir *iir, size_t nsamples, const float *const *in, float *const *out) {
  return guarded([&] { stage_process_host(iir, nsamples, in, out, reads_every_row); });
}

int earhip_iir_design(int kind, double sample_rate, double f0, double q, double gain_db, double out[5]) {
  return guarded([&] {
    require(out != nullptr, "out must not be NULL");
    if (const char *why = iir_design(kind, sample_rate, f0, q, gain_db, out)) fail_invalid(why);
  });
}

}  // extern "C"
