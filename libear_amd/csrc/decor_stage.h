// decor_stage.h — the decorrelator stage (K2) of the renderer as a type: the FIR spectra and the state between calls (overlap
// tails, delay lines, diffuse-bus history, double-buffered), made by create() and run once per span of a call.  The decisions:
// decor_plan.h; the kernels: render_kernels.h.  For api_render.hip only, which compiles the K2 kernels.
#pragma once
#include <algorithm>

#include "common.h"
#include "decor_plan.h"
#include "fft_kernels.h"
#include "fft_launch.h"
#include "render_kernels.h"

namespace earhip {

// whether transform size L has an instantiation of the workgroup kernel (launch_decor: else the run-time shape kernel)
static bool decor_fixed_size(int L) {
  bool fixed = false;
  fft_size_switch<128>(L, [&](auto) { fixed = true; }, [] {});
  return fixed;
}

// the workgroup-per-run kernel at transform size L
static void launch_decor(int L, const DecorParams &P, dim3 grid, hipStream_t s) {
  fft_size_switch<128>(
      L, [&](auto LL) { hipLaunchKernelGGL((k_decorrelate_delay_mix<decltype(LL)::value>), grid, dim3(256), 0, s, P); },
      [&] {  // any other block size: mixed-radix transforms at run time
        const FftShape S = shape_of(L, "block_size must be in [16, 4096]");
        const size_t lds = fft_rt_lds(k_decorrelate_delay_mix_rt, L, sizeof(float) * (L / 2));
        hipLaunchKernelGGL(k_decorrelate_delay_mix_rt, grid, dim3(256), lds, s, P, S);
      });
  EARHIP_HIP(hipGetLastError());
}

struct DecorStage : DecorPlan {
  int N = 0, B = 0, D = 0;  // loudspeakers, the caller's block size, delay of the direct bus in samples
  DevBuf<cf> H, tw;
  DevBuf<float> tail[2], dly[2], hist[2];  // tails [NP][N][Bk]; diffuse-bus history [N][(NP-1) Bk]
  DevBuf<float> ztail, zdly, zhist;  // all-zero state, never written: what the first call after a reset reads
  bool fresh = true;          // no call since create / reset: the state is zero
  int cur = 0;  // which state buffer holds the current state
  int last_form = 0, last_R = 0;  // of the last run: 0 workgroup template, 1 run-time shape, 2 wave kernel; blocks per run (0: no run yet)

  void create(earhip_ctx *ctx, const earhip_render_config &cfg, int block) {
    static_cast<DecorPlan &>(*this) =
        decor_plan(cfg.n_buses, block, cfg.n_taps, ctx->get(OPT_K2_OWN_BLOCK) != 0, ctx->has(OPT_RUN), ctx->get(OPT_RUN));
    N = cfg.n_out, B = block, D = cfg.delay;
    upload_twiddles(tw, Lk);
    // H[p] = DFT_L(zero-padded partition p of the FIR: taps [p B, (p + 1) B), Filter::Filter,
    // block_convolver_impl.cpp:16-41), computed with the device transform, then made exactly Hermitian so
    // that two real blocks separate cleanly
    const size_t rows = (size_t)NP * N;
    std::vector<float> parts(rows * Bk, 0.0f);  // [NP][N][B]
    for (int n = 0; n < N; n++)
      for (int t = 0; t < cfg.n_taps; t++)
        parts[((size_t)(t / Bk) * N + n) * Bk + t % Bk] = cfg.decorrelators[(size_t)n * cfg.n_taps + t];
    DevBuf<float> taps;
    taps.alloc(parts.size());
    EARHIP_HIP(hipMemcpy(taps.p, parts.data(), sizeof(float) * parts.size(), hipMemcpyHostToDevice));
    H.alloc(rows * Lk);
    launch_spectrum(Lk, taps.p, Bk, Bk, tw.p, H.p, (int)rows, ctx->stream);
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<cf> h(rows * Lk);
    EARHIP_HIP(hipMemcpy(h.data(), H.p, sizeof(cf) * h.size(), hipMemcpyDeviceToHost));
    for (size_t n = 0; n < rows; n++) {
      cf *hn = h.data() + n * Lk;
      hn[0].y = 0.0f;
      hn[Bk].y = 0.0f;
      for (int k = 1; k < Bk; k++) hn[Lk - k] = cf_conj(hn[k]);
    }
    EARHIP_HIP(hipMemcpy(H.p, h.data(), sizeof(cf) * h.size(), hipMemcpyHostToDevice));
    const size_t hist_n = (size_t)N * std::max((NP - 1) * Bk, 1);
    for (int i = 0; i < 2; i++) {
      tail[i].alloc_zero(rows * Bk, ctx->stream);
      dly[i].alloc_zero((size_t)N * std::max(D, 1), ctx->stream);
      hist[i].alloc_zero(hist_n, ctx->stream);
      if (i == 0) {
        ztail.alloc_zero((size_t)N * Bk, ctx->stream);
        zdly.alloc_zero((size_t)N * std::max(D, 1), ctx->stream);
        zhist.alloc_zero(hist_n, ctx->stream);
      }
    }
  }

  // the next call reads the all-zero state and rewrites its own pair completely
  void reset() { fresh = true; }

  // nblocks blocks (nsamples samples) of the buses [nparts][2 N][bus_stride] -> out [N][out_stride]; evp: the call timer's events
  // (nullptr: an untimed call), [4] in front of the stage's first launch and [5] behind its last
  void run(earhip_ctx *ctx, size_t nblocks, int nsamples, float *bus, size_t bus_stride, size_t part_stride, int nparts, float *out,
           size_t out_stride, hipEvent_t *evp) {
    DecorParams P;
    P.bus = bus;
    P.bus_stride = bus_stride;
    P.part_stride = part_stride;
    P.nparts = nparts;
    const bool wave_k2 = decor_wave_kernel(*this, ctx->get(OPT_K2_WG) != 0);
    const int kblocks = (int)(nblocks * (size_t)(B / Bk));  // the call in decorrelator partitions
    if (wave_k2 && nparts > 1) {
      // The wave kernel has one wave per run: summing the object splits there is a chain of
      // dependent loads on the call's critical path (block mode).  Sum them into slab 0 with the
      // whole chip first (2 N rows; in place: a thread reads and writes its own sample only).
      if (evp) EARHIP_HIP(hipEventRecord(evp[4], ctx->stream));
      hipLaunchKernelGGL(k_sum_parts, dim3((nsamples + 255) / 256, 2 * N), dim3(256), 0, ctx->stream, bus, part_stride, nparts,
                         bus_stride, 2 * N, nsamples, bus, bus_stride);
      EARHIP_HIP(hipGetLastError());
      P.nparts = 1;
    }
    P.out = out;
    P.out_stride = out_stride;
    P.tw = tw.p;
    P.dly_in = fresh ? zdly.p : dly[cur].p;
    P.dly_out = dly[cur ^ 1].p;
    P.N = N;
    P.T = kblocks;
    const int R = wave_k2 && !run_len_set ? wave_run_len(kblocks, N, ctx->num_cus, kDecorWaves) : run_len;
    P.R = R;
    last_form = wave_k2 ? 2 : decor_fixed_size(Lk) ? 0 : 1;
    last_R = R;
    P.D = D;
    P.hist_len = (NP - 1) * Bk;
    P.hist_in = fresh ? zhist.p : hist[cur].p;
    P.hist_out = hist[cur ^ 1].p;
    const dim3 grid((unsigned)((kblocks + R - 1) / R), N);
    if (evp && P.nparts == nparts) EARHIP_HIP(hipEventRecord(evp[4], ctx->stream));
    // one launch per partition of the FIRs: partition 0 writes (decorrelated + delayed direct), the
    // others add their share of the decorrelated signal (render_kernels.h)
    for (int part = 0; part < NP; part++) {
      P.H = H.p + (size_t)part * N * Lk;
      P.tail_in = (fresh ? ztail.p : tail[cur].p) + (fresh ? 0 : (size_t)part * N * Bk);
      P.tail_out = tail[cur ^ 1].p + (size_t)part * N * Bk;
      P.shift = part * Bk;
      P.accumulate = part > 0 ? 1 : 0;
      if (wave_k2) {  // one wave per run, kDecorWaves runs per workgroup
        hipLaunchKernelGGL(k_decorrelate_wave, dim3((grid.x + kDecorWaves - 1) / kDecorWaves, grid.y), dim3(64 * kDecorWaves),
                           0, ctx->stream, P);
        EARHIP_HIP(hipGetLastError());
      } else {
        launch_decor(Lk, P, grid, ctx->stream);
      }
    }
    if (evp) EARHIP_HIP(hipEventRecord(evp[5], ctx->stream));
    cur ^= 1;
    fresh = false;
  }
};

}  // namespace earhip
