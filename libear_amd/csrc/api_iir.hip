// api_iir.hip — group O of include/earhip.h: a biquad filter matrix on planar float32 rows in device memory (crossovers, bass
// management, EQ).  The kernels: iir_kernels.h; the maths they share with the CPU tests: iir.h.
#include <algorithm>
#include <memory>

#include "common.h"
#include "iir_kernels.h"

using namespace earhip;

struct earhip_iir {
  earhip_ctx *ctx = nullptr;
  int n_in = 0, n_out = 0, R = 0;
  int max_state = 0;    // the largest 2 S of any route
  int most_routes = 0;  // the most routes of one output: picks pass 2's waves
  size_t max_samples = 0;
  unsigned cap = 0;              // chunks of e and start per route
  unsigned long long clock = 0;  // samples since create / reset
  int par = 0;                   // which half of state holds the state in front of the next launch
  // everything a process call touches, made at create
  DevBuf<IirRouteDev> routes;    // [R]
  DevBuf<double> Q;              // [R][kIirPowers][kIirMat]
  DevBuf<double> e, start;       // [R][cap][16] each
  DevBuf<double> state;          // [2][R][16]
  DevBuf<int> out_first, out_routes;
  DevBuf<float> d_in, d_out;     // the host form's rows: [n_in][max_samples], [n_out][max_samples]

  // everything the handle holds on the device but the few route tables: chunk states, carried states, matrix powers, and the
  // host form's rows
  size_t scratch_bytes() const { return sizeof(double) * (e.n + start.n + state.n + Q.n) + sizeof(float) * (d_in.n + d_out.n); }

  void zero() {
    EARHIP_HIP(hipMemsetAsync(state.p, 0, sizeof(double) * state.n, ctx->stream));
    clock = 0;
    par = 0;
  }

  void check_room(size_t nsamples) const {
    if (nsamples > max_samples) fail_invalid("the call would pass the IIR stage's max_samples (nothing was consumed)");
  }

  void launch(size_t n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    const IirPlan p = iir_plan(clock, n);
    if (p.nchunks > cap) fail_internal("an IIR launch of more chunks than its scratch holds");
    IirArgs a;
    a.in = in, a.in_stride = in_stride, a.out = out, a.out_stride = out_stride;
    a.n = p.n, a.off0 = p.off0, a.nchunks = p.nchunks, a.cap = cap;
    a.routes = routes.p, a.Q = Q.p, a.e = e.p, a.start = start.p;
    const size_t half = (size_t)R * kIirMaxState;
    a.state_in = state.p + (size_t)par * half, a.state_out = state.p + (size_t)(par ^ 1) * half;
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
    par ^= 1;
  }

  // device rows; the caller has checked the room and the strides
  void feed(size_t nsamples, const float *in, size_t in_stride, float *out, size_t out_stride) {
    for (size_t at = 0; at < nsamples;) {
      const size_t n = std::min(kIirMaxLaunch, nsamples - at);
      launch(n, in + at, in_stride, out + at, out_stride);
      at += n;
    }
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
    iir->max_samples = cfg->max_samples;
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
    iir->routes.alloc((size_t)R);
    EARHIP_HIP(hipMemcpy(iir->routes.p, dev.data(), sizeof(IirRouteDev) * dev.size(), hipMemcpyHostToDevice));
    iir->Q.alloc(Q.size());
    EARHIP_HIP(hipMemcpy(iir->Q.p, Q.data(), sizeof(double) * Q.size(), hipMemcpyHostToDevice));
    iir->out_first.alloc(first.size());
    EARHIP_HIP(hipMemcpy(iir->out_first.p, first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice));
    iir->out_routes.alloc(order.size());
    EARHIP_HIP(hipMemcpy(iir->out_routes.p, order.data(), sizeof(int) * order.size(), hipMemcpyHostToDevice));
    iir->e.alloc((size_t)R * iir->cap * kIirMaxState);
    iir->start.alloc((size_t)R * iir->cap * kIirMaxState);
    iir->state.alloc(2 * (size_t)R * kIirMaxState);
    iir->d_in.alloc((size_t)cfg->n_in * cfg->max_samples);
    iir->d_out.alloc((size_t)cfg->n_out * cfg->max_samples);
    iir->zero();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    *out = iir.release();
  });
}

int earhip_iir_destroy(earhip_iir *iir) {
  return guarded([&] {
    if (!iir) return;
    (void)hipSetDevice(iir->ctx->device);
    (void)hipStreamSynchronize(iir->ctx->stream);
    delete iir;
  });
}

int earhip_iir_reset(earhip_iir *iir) {
  return guarded([&] {
    require(iir != nullptr, "iir must not be NULL");
    iir->ctx->use();
    iir->zero();
  });
}

int earhip_iir_info(const earhip_iir *iir, int info[6]) {
  return guarded([&] {
    require(iir != nullptr && info != nullptr, "iir and info must not be NULL");
    info[0] = kIirChunk, info[1] = kIirScanLanes, info[2] = kIirScanGroups, info[3] = iir->R, info[4] = iir->max_state;
    info[5] = (int)std::min<size_t>(iir->scratch_bytes(), 0x7fffffff);
  });
}

int earhip_iir_process_device(earhip_iir *iir, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                              size_t out_stride) {
  return guarded([&] {
    require(iir != nullptr, "iir must not be NULL");
    iir->check_room(nsamples);
    if (nsamples == 0) return;
    require(in_dev != nullptr && out_dev != nullptr, "device pointers must not be NULL");
    require(in_stride >= nsamples && out_stride >= nsamples, "stride too small");
    iir->ctx->use();
    iir->feed(nsamples, in_dev, in_stride, out_dev, out_stride);
  });
}

int earhip_iir_process(earhip_iir *iir, size_t nsamples, const float *const *in, float *const *out) {
  return guarded([&] {
    require(iir != nullptr, "iir must not be NULL");
    iir->check_room(nsamples);
    if (nsamples == 0) return;
    require(in != nullptr && out != nullptr, "in and out must not be NULL");
    for (int c = 0; c < iir->n_in; c++) require(in[c] != nullptr, "a row pointer is NULL");
    for (int c = 0; c < iir->n_out; c++) require(out[c] != nullptr, "a row pointer is NULL");
    earhip_ctx *ctx = iir->ctx;
    ctx->use();
    const size_t n = nsamples;
    rows_to_device(iir->d_in.p, in, iir->n_in, n, ctx->stream);
    iir->feed(n, iir->d_in.p, n, iir->d_out.p, n);
    rows_from_device(out, iir->d_out.p, iir->n_out, n, ctx->stream);
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
  });
}

int earhip_iir_design(int kind, double sample_rate, double f0, double q, double gain_db, double out[5]) {
  return guarded([&] {
    require(out != nullptr, "out must not be NULL");
    if (const char *why = iir_design(kind, sample_rate, f0, q, gain_db, out)) fail_invalid(why);
  });
}

}  // extern "C"
