// api_render.hip — (F) the composed Objects render block of include/earhip.h:
// K0 segment prep -> K1 gain_mix (direct + diffuse buses) -> K2
// decorrelate_delay_mix, `nblocks` blocks per call, state resident in HBM.
// Around it: the taps on its output bus (meter, FIR matrix, limiter), the host-pointer forms (long calls: the chunk pipeline of
// host_pipeline.h) and the forms that take and make interleaved PCM frames (their conversions: api_frames.hip, pcm_frames.h).
// Elsewhere: the gain stage's launches (api_core.hip), the decorrelator stage K2 (decor_stage.h; its decisions: decor_plan.h;
// its kernels are compiled here), the transforms' launch layer (fft_launch.h; launch_spectrum itself: api_conv.hip).
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "bus_stage.h"
#include "curves.h"
#include "decor_stage.h"
#include "host_pipeline.h"
#include "pcm_frames.h"
#include "stream_pipe.h"
#include "timeline.h"

using namespace earhip;

// What a call reports about itself afterwards (the query exports at the end of this file).  A call cut in two (render_spans)
// is reported as its main span, with the blocks of its tail.
struct CallReport {
  int kind = -1;  // gain kernel of the call: 0 VALU (strict), 1 f32 MFMA, 2 f32 MFMA on the tile grid, 3 f16x2 MFMA, 4 f16x2 MFMA over piece lists,
                  // 5 f16x2 MFMA with hinges (gain_hg.h)
  int plan[3] = {0, 0, 0};   // tile samples, tiles, grid-level object splits
  int paired = -1;           // layout of its piece lists: 1 paired, 0 packed, -1 none built
  size_t scratch_bytes = 0;  // K0 / K1 scratch the call needed
  bool gated = false;        // the call was planned for the hinge kernel behind a device-side gate
  bool device_form = false;  // ... its split-operand kernel picked its form (plain / wide) on the device
  bool hg_robust = false;    // ... a gated call beyond the packed kink products' span runs the hinge kernel's robust form (no stand-by lists)
  int tail_blocks = 0;       // blocks of the call that ran as its tail part (0: the call was not cut)
};

struct earhip_render {
  earhip_ctx *ctx = nullptr;
  int M = 0, N = 0, B = 0, K = 1, T = 0;
  std::unique_ptr<CurveSet> curves;
  int64_t t = 0;  // sample clock: absolute time of the next block
  CallReport report;         // of the last call
  long scratch_regrows = 0;  // process calls that had to grow the scratch themselves (none on committed curves)
  // What the last call's gain kernel decided on the device: the kernel that did the call left a copy of the context's mode
  // word in THIS renderer's own slot (rec[0]: the call, or the main span of a call cut in two; rec[1]: the tail span), so the
  // queries below stay valid whatever other renderers of the context do afterwards.
  DevBuf<unsigned> rec;

  DevBuf<SegDesc> desc;
  DevBuf<float> bus;  // [gsplit][K*N][bus_stride], strides chosen per call
  int max_gsplit = 1;
  DecorStage decor;  // K2 (made when K == 2; NP stays 1 on one bus)
  // host-pointer staging
  DevBuf<float> d_in, d_out;
  PinBuf<float> p_in, p_out;
  std::unique_ptr<GatherPool> gather;  // staging threads of long host-pointer calls
  StreamPipe pipe;                     // ... their copy streams and events
  int last_host_chunks = 0;            // time chunks the last host-pointer call ran as (0: one piece)
  // interleaved PCM frames (earhip_render_process_frames): the packed bytes of a call, pinned (staged from pageable memory) and on
  // the device, sized at the first frames call for max_blocks frames of that call's width (grown by a call of wider frames); the
  // interleaved outputs on the device; the device form's own converted rows and render outputs (a device-form call is still in
  // flight when it returns: it keeps off the host forms' buffers)
  PinBuf<unsigned char> p_bytes;
  DevBuf<unsigned char> d_bytes;
  DevBuf<float> d_ilv, d_rows, d_rows_out;
  // PCM frames out (earhip_render_process_frames_pcm): the packed output frames of a call on the device and pinned (pageable
  // out_frames only), sized at the first call of that form for max_blocks frames of its format (grown by a call of a wider
  // format); the levels the conversion kernel keeps, made (zeroed) with them
  DevBuf<unsigned char> d_pcm;
  PinBuf<unsigned char> p_pcm;
  PcmLevels levels;
  // timing
  bool timing = false;
  bool last_timed = false;
  int timing_every = 1;      // time every n-th process call (the event records cost ~3 us of idle GPU each)
  long timing_calls = 0;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // (a call cut into a main part and a tail — process_device — is ONE call of the timing: its two sets of events add up)
  struct Pending { hipEvent_t e[6]; bool has_k2; bool continues; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;
  double acc_ms[3] = {0, 0, 0};
  double acc_n[3] = {0, 0, 0};

  ~earhip_render() {
    for (auto &p : pending)
      for (auto e : p.e)
        if (e) (void)hipEventDestroy(e);
    for (auto e : pool) (void)hipEventDestroy(e);
  }

  // the copy of the context's mode word the last call's gain kernel left in this renderer's slot, valid until this renderer's next
  // call (synchronises the stream)
  unsigned mode_word() {
    ctx->use();
    unsigned word = 0;
    EARHIP_HIP(hipMemcpyAsync(&word, rec.p, sizeof(word), hipMemcpyDeviceToHost, ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    if (!(word & kModeRecorded)) fail_internal("no gain kernel recorded the call's mode word");
    return word;
  }

  hipEvent_t get_event() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e;
    EARHIP_HIP(hipEventCreate(&e));
    return e;
  }

  void drain_timing() {
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    for (auto &p : pending) {
      float ms = 0;
      const double one = p.continues ? 0.0 : 1.0;  // (the second part of a call cut in two adds time, not a call)
      EARHIP_HIP(hipEventElapsedTime(&ms, p.e[0], p.e[1]));
      acc_ms[2] += ms; acc_n[2] += one;
      EARHIP_HIP(hipEventElapsedTime(&ms, p.e[2], p.e[3]));
      acc_ms[0] += ms; acc_n[0] += one;
      if (p.has_k2) {
        EARHIP_HIP(hipEventElapsedTime(&ms, p.e[4], p.e[5]));
        acc_ms[1] += ms; acc_n[1] += one;
      }
      for (auto e : p.e)
        if (e) pool.push_back(e);
    }
    pending.clear();
  }

  // Channel pointers that are evenly spaced inside memory the device reaches (earhip_host_alloc / earhip_host_register: the
  // columns of a pinned matrix) need no staging copy: strided DMA in, and the output rows written in place.  The stride in
  // floats; 0: not that shape.
  size_t direct_stride(const float *const *ch, int count, size_t n) const {
    if (ctx->host_ranges.empty() || count < 1) return 0;
    // (addresses as integers: the channel pointers need not belong to one array as far as C++ knows)
    const uintptr_t a0 = (uintptr_t)ch[0];
    const uintptr_t step = count > 1 ? (uintptr_t)ch[1] - a0 : sizeof(float) * n;
    if ((a0 & 15) != 0 || step % 16 != 0 || step < sizeof(float) * n || step > ((uintptr_t)1 << 40)) return 0;
    for (int c = 1; c < count; c++)
      if ((uintptr_t)ch[c] - (uintptr_t)ch[c - 1] != step) return 0;
    return ctx->host_reachable(ch[0], step * (count - 1) + sizeof(float) * n) ? (size_t)(step / sizeof(float)) : 0;
  }

  // the device frames forms' first step: the call's frames converted into d_rows, rows of the n samples returned (with_out:
  // the form renders into d_rows_out, for interleaved outputs)
  size_t frames_to_device_rows(size_t nblocks, const void *frames_dev, int fmt, int frame_channels, int first_channel, bool with_out) {
    ctx->use();
    const size_t S = (size_t)pcm_sample_bytes(fmt), n = nblocks * (size_t)B, cap = (size_t)T * B;
    if (d_rows.n < cap * M || (with_out && d_rows_out.n < cap * N)) {
      EARHIP_HIP(hipStreamSynchronize(ctx->stream));  // (first use: nothing of this renderer may still read them)
      d_rows.reserve(cap * M);
      if (with_out) d_rows_out.reserve(cap * N);
    }
    launch_pcm_to_rows(fmt, frames_dev, (size_t)frame_channels * S, (size_t)first_channel * S, M, n, d_rows.p, n, ctx->stream);
    return n;
  }
  void reserve_pcm_out(size_t bytes, bool pinned) {
    levels.reserve(N, ctx->stream);
    d_pcm.reserve(bytes);
    if (pinned) p_pcm.reserve(bytes);
  }

  // the chunk plan of a call from host memory (earhip_render_process and _process_frames alike)
  HostChunkPlan host_plan(size_t nblocks, bool direct) const {
    return plan_host_chunks(nblocks, B, M, direct, ctx->has(OPT_HOST_CHUNK_MB), ctx->get(OPT_HOST_CHUNK_MB), ctx->get(OPT_HOST_FIRST, 0));
  }
  // A chunk's planar outputs — samples [at, at + len) of every row, chunk-major in d_out and p_out — on their way back: on pipe.out
  // by strided DMA into the caller's device-reachable rows (out_st: their stride) or into p_out, and from there to the caller's rows.
  hipError_t chunk_rows_d2h(float *out0, size_t out_st, size_t at, size_t len) {
    const float *dout = d_out.p + (size_t)N * at;
    if (out_st)
      return hipMemcpy2DAsync(out0 + at, sizeof(float) * out_st, dout, sizeof(float) * len, sizeof(float) * len, N, hipMemcpyDeviceToHost, pipe.out);
    return hipMemcpyAsync(p_out.p + (size_t)N * at, dout, sizeof(float) * len * N, hipMemcpyDeviceToHost, pipe.out);
  }
  void chunk_rows_scatter(float *const *out, size_t at, size_t len) const {
    for (int ch = 0; ch < N; ch++) std::memcpy(out[ch] + at, p_out.p + (size_t)N * at + (size_t)ch * len, sizeof(float) * len);
  }
  // Short calls, planar outputs, from d_in: K2 writes the few output rows straight into host memory (the caller's own rows when they
  // are reachable, else the pinned staging buffer: no D2H copy to start and wait for, 126 -> 119 us per
  // 512-sample call at the headline shape).  The other direction does not pay — kernels that read their 2 MB
  // of inputs over PCIe themselves are slower than the copy engine plus kernels (129 us) — and neither does
  // spinning on a completion word behind one more launch.
  // (FIRs of several partitions accumulate into the output: that stays in device memory, and out_st is 0 then)
  void process_short_call(size_t nblocks, float *out0, size_t out_st) {
    const size_t n = nblocks * (size_t)B;
    const bool direct_out = decor.NP <= 1;
    process_device(nblocks, d_in.p, n, out_st ? out0 : direct_out ? p_out.p : d_out.p, out_st ? out_st : n);
    if (!out_st && !direct_out) EARHIP_HIP(hipMemcpyAsync(p_out.p, d_out.p, sizeof(float) * n * N, hipMemcpyDeviceToHost, ctx->stream));
  }
  // the staging threads of long calls from pageable memory, started at the first such call (option HOST_THREADS: how many)
  GatherPool &staging_threads() {
    if (!gather) {
      gather.reset(new GatherPool);
      const int want = ctx->get(OPT_HOST_THREADS, 0);
      gather->start(want >= 1 && want <= 64 ? want : default_staging_threads());
    }
    return *gather;
  }

  // the launch plan of a call of nblocks blocks at the current sample clock
  MixLaunch plan_call(size_t nblocks, size_t in_stride) {
    const int nsamples = (int)(nblocks * (size_t)B);
    MixLaunch ml = plan_mix(ctx, curves->plan(), M, nsamples, ctx->strict, max_gsplit, curves->stats(t, in_stride, (size_t)nsamples, true));
    const size_t bus_stride = ((size_t)nsamples + 3) & ~(size_t)3;
    while (ml.gsplit > 1 && bus_stride * K * N * ml.gsplit > bus.n) ml.gsplit /= 2;
    return ml;
  }

  // Everything a call on the CURRENT curves can need beyond what earhip_render_create allocated — K0 / K1 scratch for
  // the plan of the call (piece or hinge lists are sized from the curves), the kink rows of the hinge kernel — is made
  // HERE, where curves change (earhip_render_commit, or the implicit commit of the first process call after
  // set_object_points), for the longest call (max_blocks), a call half as long and a single block, with a quarter of
  // headroom: process calls on committed curves neither allocate nor synchronise (include/earhip.h, conventions).
  size_t last_in_stride = 0;
  void reserve_for_curves() {
    size_t need = 0;
    bool hinge = false;
    const size_t lens[3] = {(size_t)T, (size_t)std::max(1, T / 2), (size_t)1};
    for (size_t nb : lens) {
      const MixLaunch ml = plan_call(nb, last_in_stride ? last_in_stride : nb * (size_t)B);
      need = std::max(need, scratch_units(*curves, ml, M));
      hinge = hinge || ml.kind == GainKernel::Hinge;
    }
    if (hinge) curves->ensure_kinks(ctx);
    if (need > desc.n) {
      EARHIP_HIP(hipStreamSynchronize(ctx->stream));  // (the old scratch may still be in use)
      desc.reserve(need + need / 4);
    }
  }

  // Workgroups of the gain kernel the chip holds at once for a plan: the tiles of a call are worked off in rounds of so many
  // (8-wave forms: one workgroup per CU; 4-wave forms: two)
  int resident_workgroups(const MixLaunch &ml) const {
    if (!ml.split_operands()) return 0;
    return ctx->num_cus * (ml.tile() >= 512 ? 1 : 2);
  }

  // A tile of the headline scene is 100 us of one CU: a call of k rounds of tiles PLUS A FEW (1025 blocks; the 513 of a
  // time-sharded rank: its share and a lead block) used to cost k + 1 rounds — 0.306 ms for 513 blocks where 512 take 0.235.
  // Such a call is cut in two: the whole rounds as they were, and the few tiles behind them as a short call of their own,
  // which the planner spreads over the chip by splitting the objects (as in block mode).  The cut costs a second K0, a
  // second K2 launch and the boundaries (~30 us): taken when the tail is at most a quarter of a round.  Results are those
  // of two consecutive calls (every call length is a valid call: the state carries over).
  // The one place every form of process call passes.  The taps on the output bus read the planar rows the call wrote — the
  // caller's, d_out or d_rows_out — behind the call's kernels: after the tail cut, so a call that ran as two spans is seen once per
  // sample.  An attached loudness meter (earhip_render_attach_loudness) only reads.  An attached FIR matrix
  // (earhip_render_attach_firmix) writes its own rows to the caller's sink at the tap's pos, a host counter: the feeds are
  // enqueued in order.  An attached limiter (earhip_render_attach_limiter) comes behind the meter and the matrix, which both see
  // the unlimited bus, and writes the limited rows to its own sink.  Without a tap this is render_spans and nothing else.
  struct BusTap {
    BusStage *stage = nullptr;  // NULL: nothing attached
    float *sink = nullptr;      // (the meter has none)
    size_t stride = 0, cap = 0, pos = 0;
  };
  enum { TAP_METER, TAP_MATRIX, TAP_LIMITER, TAP_COUNT };  // the order they are fed in
  BusTap taps[TAP_COUNT];
  bool tapped() const {
    for (const BusTap &t : taps)
      if (t.stage) return true;
    return false;
  }
  // a stage is attached or (NULL) detached; either way the tap starts at 0.  rows_words: the refusal of a stage with other rows
  // than the bus; a stage that writes brings its sink
  void attach(int which, BusStage *stage, const char *rows_words, bool writes, float *sink_dev, size_t sink_stride,
              size_t sink_capacity) {
    if (stage) {
      const std::string the = std::string("the ") + stage->noun;
      if (stage->ctx != ctx) fail_invalid(the + " must belong to the renderer's context");
      require(stage->n_in == N, rows_words);
      if (stage->block != 1 && stage->block != B) fail_invalid(the + " must have the renderer's block size");
      if (writes) {
        require(sink_dev != nullptr, "sink_dev must not be NULL");
        require(sink_stride >= sink_capacity, "sink_stride must be >= sink_capacity");
      }
    }
    taps[which] = stage && writes ? BusTap{stage, sink_dev, sink_stride, sink_capacity, 0} : BusTap{stage};
  }
  // a tap that has no room for the call refuses it before anything is rendered
  void check_taps(size_t nblocks) const {
    const size_t n = nblocks * (size_t)B;
    for (const BusTap &t : taps) {
      if (!t.stage) continue;
      t.stage->check_room(n / (size_t)t.stage->block);
      if (t.sink && t.pos + n > t.cap)
        fail_invalid(std::string("the call would pass the ") + t.stage->noun + "'s sink_capacity (nothing was rendered)");
    }
  }
  void feed_taps(size_t nblocks, const float *out_dev, size_t out_stride) {
    const size_t n = nblocks * (size_t)B;
    for (BusTap &t : taps) {
      if (!t.stage) continue;
      t.stage->feed(n / (size_t)t.stage->block, out_dev, out_stride, t.sink ? t.sink + t.pos : nullptr, t.stride);
      if (t.sink) t.pos += n;
    }
  }
  void process_device(size_t nblocks, const float *in_dev, size_t in_stride, float *out_dev, size_t out_stride) {
    if (!tapped()) return render_spans(nblocks, in_dev, in_stride, out_dev, out_stride);
    check_taps(nblocks);
    render_spans(nblocks, in_dev, in_stride, out_dev, out_stride);
    feed_taps(nblocks, out_dev, out_stride);
  }
  void render_spans(size_t nblocks, const float *in_dev, size_t in_stride, float *out_dev, size_t out_stride) {
    MixLaunch whole;  // the plan of the uncut call, made once (process_span takes it as it is)
    bool have_plan = false;
    if (!ctx->strict && ctx->get(OPT_TAILCUT, 1) != 0 && nblocks >= 2) {
      last_in_stride = in_stride;
      if (curves->dirty()) {
        curves->commit(ctx);
        reserve_for_curves();
      }
      const MixLaunch ml = whole = plan_call(nblocks, in_stride);
      have_plan = true;
      const int W = resident_workgroups(ml);
      if (W > 0 && ml.gsplit == 1 && ml.ntiles > W) {
        const size_t tile = (size_t)ml.tile();
        const size_t full = (size_t)ml.ntiles / (size_t)W, rest = (size_t)ml.ntiles % (size_t)W;
        const size_t main_samples = full * (size_t)W * tile;
        // (option TAILCUT = v: tails of up to v / 8 of a round are cut off; default 2, 0: never)
        const size_t eighths = (size_t)std::min(std::max(ctx->get(OPT_TAILCUT, 2), 0), 7);
        if (rest > 0 && rest <= (size_t)W * eighths / 8 && main_samples % (size_t)B == 0) {
          const size_t main_blocks = main_samples / (size_t)B;
          process_span(main_blocks, in_dev, in_stride, out_dev, out_stride, false);
          const CallReport main = report;
          process_span(nblocks - main_blocks, in_dev + main_samples, in_stride, out_dev + main_samples, out_stride, true);
          report = main;  // (what the call is reported as: its main part — kernel, plan and what it decided on the device)
          report.tail_blocks = (int)(nblocks - main_blocks);
          return;
        }
      }
    }
    report.tail_blocks = 0;
    process_span(nblocks, in_dev, in_stride, out_dev, out_stride, false, have_plan ? &whole : nullptr);
  }

  void process_span(size_t nblocks, const float *in_dev, size_t in_stride, float *out_dev,
                    size_t out_stride, bool continues, const MixLaunch *planned = nullptr) {
    const int nsamples = (int)(nblocks * (size_t)B);
    last_in_stride = in_stride;
    if (curves->dirty()) {
      curves->commit(ctx);
      reserve_for_curves();
    }
    const bool strict = ctx->strict;
    MixLaunch ml = planned ? *planned : plan_call(nblocks, in_stride);
    if (ml.kind == GainKernel::Hinge) curves->ensure_kinks(ctx);  // (already there unless an option changed the plan since the commit)

    report.kind = (int)ml.kind;
    {
      // K0 / K1 scratch for THIS plan and THESE curves (round 3: 537 MB at the headline's size for any curves): reserved
      // when the curves were committed (reserve_for_curves).  The one exception, documented in earhip.h: a plan that no
      // commit foresaw (an option changed between commit and call, a call on a time grid the curves' phase statistics
      // did not predict) grows it here, geometrically, behind a synchronisation.
      const size_t need = scratch_units(*curves, ml, M);
      if (need > desc.n) {
        EARHIP_HIP(hipStreamSynchronize(ctx->stream));
        desc.reserve(need + need / 2);
        scratch_regrows++;
      }
      report.scratch_bytes = need * 16;
    }
    const size_t bus_stride = ((size_t)nsamples + 3) & ~(size_t)3;
    const size_t part_stride = bus_stride * K * N;
    // (the bus is sized for every plan plan_mix can make, earhip_render_create; should a tuning knob push a plan
    // beyond it, plan_call has taken fewer object splits, always a valid plan)
    if (part_stride * ml.gsplit > bus.n) fail_internal("bus buffer too small for this launch plan");
    report.paired = (ml.kind == GainKernel::Pieces || ml.kind == GainKernel::Hinge) ? (ml.paired ? 1 : 0) : -1;
    report.plan[0] = ml.tile();
    report.plan[1] = ml.ntiles;
    report.plan[2] = ml.gsplit;
    Pending pd;
    hipEvent_t *evp = nullptr;
    // (the second part of a call cut in two is timed when its first part was)
    const bool timed = timing && (continues ? last_timed : (timing_calls++ % timing_every) == 0);
    last_timed = timed;
    if (timed) {
      for (int i = 0; i < 6; i++) pd.e[i] = get_event();
      pd.has_k2 = K == 2;
      pd.continues = continues;
      evp = pd.e;
    }
    unsigned *const record = rec.p + (continues ? 1 : 0);  // (where K1 leaves the call's mode word: this renderer's own slot)
    MixResult mix;
    if (K == 1) {
      // direct bus only: K1 writes the output rows itself
      mix = launch_gain_mix_summed(ctx, *curves, ml, strict, t, nsamples, in_dev, in_stride, out_dev, out_stride, bus.p, bus_stride, desc.p,
                                   record, evp);
    } else {
      mix = launch_gain_mix(ctx, *curves, ml, strict, t, nsamples, in_dev, in_stride, bus.p, bus_stride, part_stride, desc.p, record, evp);
      decor.run(ctx, nblocks, nsamples, bus.p, bus_stride, part_stride, ml.gsplit, out_dev, out_stride, evp);
    }
    if (timed) pending.push_back(pd);
    report.gated = mix.gated, report.device_form = mix.device_form, report.hg_robust = mix.hinge_robust;
    if (mix.grew) scratch_regrows++;  // (a buffer of the context no renderer had announced: earhip.h)
    t += nsamples;
  }
};

extern "C" {

int earhip_render_create(earhip_ctx *ctx, const earhip_render_config *cfg, earhip_render **out) {
  return guarded([&] {
    require(ctx != nullptr && cfg != nullptr && out != nullptr, "NULL argument");
    require(cfg->n_objects >= 1 && cfg->n_out >= 1, "n_objects and n_out must be >= 1");
    require(cfg->n_buses == 1 || cfg->n_buses == 2, "n_buses must be 1 or 2");
    // (any size, as libear's kissfft: 480, 960, 1920 ... through mixed-radix passes, other primes through the
    // generic butterfly; the tuned kernels are the power-of-two sizes from 64)
    FftShape shape;
    require(cfg->block_size >= 16 && cfg->block_size <= 4096 && fft_make_shape(2 * cfg->block_size, &shape),
            "block_size must be in [16, 4096]");
    require(cfg->max_blocks >= 1, "max_blocks must be >= 1");
    require((int64_t)cfg->max_blocks * cfg->block_size < ((int64_t)1 << 30),
            "max_blocks * block_size too large");
    require(cfg->delay >= 0, "delay must be >= 0");
    if (cfg->n_buses == 2) {
      require(cfg->decorrelators != nullptr && cfg->n_taps >= 1,
              "n_buses == 2 needs decorrelator filters");
      require((cfg->n_taps + cfg->block_size - 1) / cfg->block_size <= 64,
              "decorrelator filters of more than 64 blocks are not supported by the fused render "
              "(use BlockConvolver)");
    } else {
      require(cfg->delay == 0, "delay needs n_buses == 2");
    }
    ctx->use();
    std::unique_ptr<earhip_render> r(new earhip_render);
    r->ctx = ctx;
    r->M = cfg->n_objects;
    r->N = cfg->n_out;
    r->B = cfg->block_size;
    r->K = cfg->n_buses;
    r->T = cfg->max_blocks;
    r->curves.reset(new CurveSet(r->M, r->K * r->N, r->K, false));
    const size_t max_samples = (size_t)r->T * r->B;
    reserve_call_words(ctx, r->M, max_samples);  // (the context's words for calls of this size: no process call makes them)
    r->rec.alloc_zero(2, ctx->stream);
    // smallest tile any gain kernel of this context uses (f32 MFMA: 16 * nrt samples)
    const size_t min_tile = (size_t)std::min(16 * ctx->nrt, std::min(64 * ctx->spl, 256));
    const size_t max_tiles = (max_samples + min_tile - 1) / min_tile;
    // (the scratch of K0 / K1 — descriptors, slot, piece or hinge lists — is sized per call from the plan and the curves:
    // process_device; here only what the grid kernel needs for the longest call)
    r->desc.alloc((size_t)r->M * ((max_samples + 255) / 256) + 1);
    (void)max_tiles;  // (the piece-list kernel's tiles: 256 or 512 samples)
    // Buses: [gsplit][K*N][pad4(nsamples)] per call.  Grid-level object splits (gsplit > 1) are only
    // chosen for calls with few tiles: plan_mix doubles gsplit while gsplit * (ntiles / tpw) stays below
    // 2 * num_cus, so gsplit * ntiles < (4 * num_cus + gsplit) * tpw with tiles of at most 256 samples
    // (tpw = 1) or 16 * nrt samples (f32 MFMA kernel, tpw adjacent tiles per workgroup).
    r->max_gsplit = 16;  // block mode: more splits make K2 sum more partial slabs than K1 gains
    if (ctx->has(OPT_GSPLIT)) {  // tuning knob: grid-level splits of short calls
      const int v = ctx->get(OPT_GSPLIT);
      if (v >= 1 && v <= 32) r->max_gsplit = v;
    }
    r->bus.alloc_zero((size_t)r->K * r->N * bus_samples_bound(ctx, max_samples, r->max_gsplit), ctx->stream);
    if (r->K == 2) r->decor.create(ctx, *cfg, r->B);
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    *out = r.release();
  });
}

int earhip_render_destroy(earhip_render *r) {
  return guarded([&] {
    if (!r) return;
    (void)hipSetDevice(r->ctx->device);
    (void)hipStreamSynchronize(r->ctx->stream);
    delete r;
  });
}

int earhip_render_set_object_points(earhip_render *r, int object, int npoints,
                                    const int64_t *times, const float *direct,
                                    const float *diffuse) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    require(npoints >= 1, "interp_points must not be empty");
    require(times != nullptr && direct != nullptr, "times/direct must not be NULL");
    require(r->K == 1 || diffuse != nullptr, "diffuse gains must not be NULL when n_buses == 2");
    const int N = r->N, cols = r->K * N;
    std::vector<float> rows((size_t)npoints * cols);
    for (int k = 0; k < npoints; k++) {
      std::memcpy(&rows[(size_t)k * cols], direct + (size_t)k * N, sizeof(float) * N);
      if (r->K == 2)
        std::memcpy(&rows[(size_t)k * cols + N], diffuse + (size_t)k * N, sizeof(float) * N);
    }
    r->curves->set_object(object, npoints, times, rows.data());
  });
}

// ---- the block timeline (include/earhip.h, group W; the rule, the windows and the row copies: timeline.h) -------------------
static void timeline_guard(const std::function<void()> &f) {
  try {
    f();
  } catch (const TimelineFailure &e) {
    fail_invalid(e.msg);
  }
}

int earhip_timeline_window(int mode, int64_t start, int n_blocks, const earhip_block_timing *blocks, int64_t t0, int64_t t1,
                           int *first_block, int *last_block) {
  return guarded([&] {
    require(first_block != nullptr && last_block != nullptr, "first_block / last_block must not be NULL");
    timeline_guard([&] {
      timeline_check(mode, start, n_blocks, blocks);
      timeline_window(start, n_blocks, blocks, t0, t1, first_block, last_block);
    });
  });
}

int earhip_timeline_points(int mode, int64_t start, int n_blocks, const earhip_block_timing *blocks, int64_t t0, int64_t t1,
                           int capacity, int64_t *times, int32_t *source, int *n_points) {
  return guarded([&] {
    require(n_points != nullptr, "n_points must not be NULL");
    require(capacity >= 0, "capacity must be >= 0");
    require(capacity == 0 || (times != nullptr && source != nullptr), "times / source must not be NULL when capacity > 0");
    timeline_guard([&] {
      timeline_check(mode, start, n_blocks, blocks);
      int b0, b1;
      timeline_window(start, n_blocks, blocks, t0, t1, &b0, &b1);
      const int64_t n = timeline_emit(mode, start, blocks, b0, b1, 0, nullptr, nullptr);
      if (n > (int64_t)0x7fffffff) timeline_fail("more than 2^31 - 1 points: take a window");
      *n_points = (int)n;
      if (capacity == 0) return;
      if (capacity < n) timeline_fail("capacity " + std::to_string(capacity) + " is too small for " + std::to_string(n) + " points");
      timeline_emit(mode, start, blocks, b0, b1, n, times, source);
    });
  });
}

int earhip_render_set_objects_blocks(earhip_render *r, int n_tracks, const int *objects, const int *modes, const int64_t *starts,
                                     const int64_t *block_offsets, const earhip_block_timing *blocks, int64_t t0, int64_t t1,
                                     const float *direct, const float *diffuse) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    timeline_guard([&] {
      timeline_bind(r->M, r->N, r->K, kMaxPointsPerObject, n_tracks, objects, modes, starts, block_offsets, blocks, t0, t1, direct,
                    diffuse, [&](int object, int npoints, const int64_t *times, const float *rows) {
                      r->curves->set_object(object, npoints, times, rows);
                    });
    });
  });
}

int earhip_render_set_object_blocks(earhip_render *r, int object, int mode, int64_t start, int n_blocks,
                                    const earhip_block_timing *blocks, int64_t t0, int64_t t1, const float *direct,
                                    const float *diffuse) {
  const int64_t offsets[2] = {0, n_blocks};
  return earhip_render_set_objects_blocks(r, 1, &object, &mode, &start, offsets, blocks, t0, t1, direct, diffuse);
}

int earhip_render_commit(earhip_render *r) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    r->ctx->use();
    r->curves->commit(r->ctx);
    r->reserve_for_curves();
  });
}

int earhip_render_reset(earhip_render *r, int64_t sample_time) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    r->ctx->use();
    r->t = sample_time;
    r->decor.reset();
    r->levels.zero(r->ctx->stream);  // (only a renderer that has made PCM frames has any)
  });
}

int earhip_render_attach_loudness(earhip_render *r, earhip_loudness *m) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    r->attach(earhip_render::TAP_METER, as_stage(m), "the meter must have n_out channels", false, nullptr, 0, 0);
  });
}

int earhip_render_attach_firmix(earhip_render *r, earhip_firmix *fm, float *sink_dev, size_t sink_stride, size_t sink_capacity) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    r->attach(earhip_render::TAP_MATRIX, as_stage(fm), "the FIR matrix must have n_in = the renderer's n_out", true, sink_dev,
              sink_stride, sink_capacity);
  });
}

int earhip_render_attach_limiter(earhip_render *r, earhip_limiter *lim, float *sink_dev, size_t sink_stride, size_t sink_capacity) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    r->attach(earhip_render::TAP_LIMITER, as_stage(lim), "the limiter must have n_channels = the renderer's n_out", true, sink_dev,
              sink_stride, sink_capacity);
  });
}

static int tap_position(earhip_render *r, int which, size_t *samples) {
  return guarded([&] {
    require(r != nullptr && samples != nullptr, "render and samples must not be NULL");
    *samples = r->taps[which].pos;
  });
}
int earhip_render_firmix_position(earhip_render *r, size_t *samples) { return tap_position(r, earhip_render::TAP_MATRIX, samples); }
int earhip_render_limiter_position(earhip_render *r, size_t *samples) { return tap_position(r, earhip_render::TAP_LIMITER, samples); }

int earhip_render_process_device(earhip_render *r, size_t nblocks, const float *in_dev,
                                 size_t in_stride, float *out_dev, size_t out_stride) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    require(in_dev != nullptr && out_dev != nullptr, "device pointers must not be NULL");
    require(nblocks <= (size_t)r->T, "nblocks exceeds max_blocks");
    r->check_taps(nblocks);  // (an attached meter, FIR matrix or limiter that has no room for the call: nothing is rendered)
    require(in_stride >= nblocks * r->B && out_stride >= nblocks * r->B, "stride too small");
    if (nblocks == 0) return;
    r->ctx->use();
    r->process_device(nblocks, in_dev, in_stride, out_dev, out_stride);
  });
}

int earhip_render_process(earhip_render *r, size_t nblocks, const float *const *in,
                          float *const *out) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    require(in != nullptr && out != nullptr, "in and out must not be NULL");
    require(nblocks <= (size_t)r->T, "nblocks exceeds max_blocks");
    r->check_taps(nblocks);  // (an attached meter, FIR matrix or limiter that has no room for the call: nothing is rendered)
    if (nblocks == 0) return;
    earhip_ctx *ctx = r->ctx;
    ctx->use();
    const size_t n = nblocks * r->B;
    const size_t cap = (size_t)r->T * r->B;
    r->p_in.reserve(cap * r->M);
    r->p_out.reserve(cap * r->N);
    r->d_in.reserve(cap * r->M);
    r->d_out.reserve(cap * r->N);
    const bool dbg = ctx->get(OPT_DEBUG_TIMING) != 0;
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_a = dbg ? now() : 0.0;
    const bool short_call = r->host_plan(nblocks, false).short_call;
    const size_t in_st = r->direct_stride(in, r->M, n);
    const size_t out_st = r->decor.NP <= 1 || !short_call ? r->direct_stride(out, r->N, n) : 0;
    r->last_host_chunks = 0;
    if (!short_call) {
      // Long calls (libear's calling convention for offline renders: host channel pointers, any length) run as the pipeline of
      // time chunks of host_pipeline.h, each chunk an ordinary process call of its blocks (the DSP state carries over): the
      // kernels are ~100 x faster than the bus, so the call takes what its inputs take over PCIe plus one chunk's kernels and
      // output transfer.  Pageable rows are gathered chunk-major into the pinned buffer by the staging threads, a chunk ahead;
      // device-reachable rows (earhip_host_alloc / _register) go by strided DMA both ways, without either copy.
      // (the plan, the same for earhip_render_process_frames: host_gather.h, plan_host_chunks)
      const HostChunkPlan plan = r->host_plan(nblocks, in_st != 0);
      r->pipe.begin(ctx->stream);
      GatherPool *gp = nullptr;
      if (!in_st) {
        gp = &r->staging_threads();
        gp->submit(in, r->p_in.p, n, plan.cstart, plan.nch, r->M, ctx->get(OPT_HOST_BIND, 0) != 0, ctx->get(OPT_HOST_NT, 1) != 0);
      }
      const HostChunkTimes tm = run_host_chunks(
          r->pipe, gp, plan, !out_st, &r->last_host_chunks,
          [&](size_t at, size_t len) {
            float *din = r->d_in.p + (size_t)r->M * at;
            if (in_st)
              return hipMemcpy2DAsync(din, sizeof(float) * len, in[0] + at, sizeof(float) * in_st, sizeof(float) * len, r->M,
                                      hipMemcpyHostToDevice, r->pipe.in);
            return hipMemcpyAsync(din, r->p_in.p + (size_t)r->M * at, sizeof(float) * len * r->M, hipMemcpyHostToDevice, r->pipe.in);
          },
          [&](size_t at, size_t len) {
            r->process_device(len / r->B, r->d_in.p + (size_t)r->M * at, len, r->d_out.p + (size_t)r->N * at, len);
          },
          [&](size_t at, size_t len) { return r->chunk_rows_d2h(out[0], out_st, at, len); },
          [&](size_t at, size_t len) { r->chunk_rows_scatter(out, at, len); },
          [&] { return dbg ? now() : 0.0; });
      if (dbg)
        fprintf(stderr, "render_process: %d chunks of %zu blocks%s: enqueue incl. gather %.1f us, drain %.1f us, scatter of the rest %.1f us\n",
                plan.nch, plan.cb, in_st ? " (device-reachable rows)" : "", tm.enqueued - t_a, tm.drained - tm.enqueued, now() - tm.drained);
      return;
    }
    if (in_st) {
      EARHIP_HIP(hipMemcpy2DAsync(r->d_in.p, sizeof(float) * n, in[0], sizeof(float) * in_st, sizeof(float) * n, r->M,
                                  hipMemcpyHostToDevice, ctx->stream));
    } else {
      // short calls (block mode): one gather, one transfer.  Splitting a 2 MB block into groups whose
      // transfers overlap the gather was measured twice and loses (132 -> 150 us per call at the headline
      // shape: four DMA start-ups cost more than the 30 us of gather they hide).
      // ... in `groups` parts, the transfer of a part starting while the next is gathered (EARHIP_BLOCK_GROUPS;
      // default 2 above 1 MB: a second DMA start-up costs less than the half gather it hides, four cost more:
      // 0.134 / 0.126 / 0.138 ms per 512-sample call of 1024 objects with 1 / 2 / 4 groups, same box.  Enqueueing the
      // segment descriptors — the part of K0 that does not look at the inputs — ahead of the gather was measured
      // too and loses: 0.146 / 0.125 / 0.138: the launch is host time in front of the gather, and the probe it
      // leaves behind the transfer is one more kernel in the chain)
      const int groups_env = ctx->get(OPT_BLOCK_GROUPS);
      const int groups = groups_env >= 1 && groups_env <= 8 ? groups_env : (sizeof(float) * n * r->M >= ((size_t)1 << 20) ? 2 : 1);
      for (int g = 0; g < groups; g++) {
        const int m0 = (int)((int64_t)r->M * g / groups), m1 = (int)((int64_t)r->M * (g + 1) / groups);
        for (int m = m0; m < m1; m++) std::memcpy(r->p_in.p + (size_t)m * n, in[m], sizeof(float) * n);
        if (m1 > m0)
          EARHIP_HIP(hipMemcpyAsync(r->d_in.p + (size_t)m0 * n, r->p_in.p + (size_t)m0 * n, sizeof(float) * n * (m1 - m0),
                                    hipMemcpyHostToDevice, ctx->stream));
      }
    }
    const double t_b = dbg ? now() : 0.0;
    r->process_short_call(nblocks, out[0], out_st);
    const double t_c = dbg ? now() : 0.0;
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    const double t_d = dbg ? now() : 0.0;
    if (!out_st) r->chunk_rows_scatter(out, 0, n);
    if (dbg)
      fprintf(stderr, "render_process: gather+H2D enqueue %.1f us, launches %.1f us, wait %.1f us, scatter %.1f us\n", t_b - t_a,
              t_c - t_b, t_d - t_c, now() - t_d);
  });
}

// ---- interleaved PCM frames (include/earhip.h, group F: earhip_render_process_frames) --------------------------------------
// what both forms refuse before they touch anything
static void check_frames_args(const earhip_render *r, size_t nblocks, const void *frames, int fmt, int frame_channels, int first_channel) {
  require(r != nullptr, "render must not be NULL");
  const int S = pcm_sample_bytes(fmt);
  require(S != 0, "unknown PCM format");
  require(frames != nullptr, "frames must not be NULL");
  require(first_channel >= 0, "first_channel must be >= 0");
  require((int64_t)first_channel + r->M <= (int64_t)frame_channels, "first_channel + n_objects exceeds frame_channels");
  require(nblocks <= (size_t)r->T, "nblocks exceeds max_blocks");
  r->check_taps(nblocks);
  require(fmt == EARHIP_PCM_S24 || reinterpret_cast<uintptr_t>(frames) % (uintptr_t)S == 0, "frames not aligned to the sample size");
}

// The host form of both frames calls (arguments checked by the caller).  po == nullptr: earhip_render_process_frames, float outputs
// through `out`.  po != nullptr: earhip_render_process_frames_pcm: the outputs are interleaved frames of po->format at out_pcm —
// the interleaved float path with k_rows_to_pcm in the place of k_rows_to_frames and frames of n_out * (sample size) bytes.
static void process_frames_host(earhip_render *r, size_t nblocks, const void *frames, int fmt, int frame_channels, int first_channel,
                                float *const *out, int out_interleaved, const earhip_pcm_out *po, void *out_pcm) {
  earhip_ctx *ctx = r->ctx;
  ctx->use();
  const int M = r->M, N = r->N;
  const size_t S = (size_t)pcm_sample_bytes(fmt);
  const size_t n = nblocks * r->B, cap = (size_t)r->T * r->B;
  const size_t fb = (size_t)frame_channels * S, first_byte = (size_t)first_channel * S, bytes = n * fb;
  const bool direct = ctx->host_reachable(frames, bytes);  // (device-reachable frames: DMA straight from the caller's buffer)
  // (the plan of earhip_render_process on rows in the same kind of memory: the same chunks, the same results)
  const HostChunkPlan plan = r->host_plan(nblocks, direct);
  float *const out0 = po ? nullptr : out[0];
  // interleaved outputs, float or PCM, as bytes: a frame is ofb bytes; ilv_host the caller's frames, ilv_dev / ilv_pin ours
  const size_t ofb = (size_t)N * (po ? (size_t)pcm_sample_bytes(po->format) : sizeof(float));
  unsigned char *const ilv_host = po ? static_cast<unsigned char *>(out_pcm) : reinterpret_cast<unsigned char *>(out0);
  const size_t out_st = out_interleaved ? 0 : r->decor.NP <= 1 || !plan.short_call ? r->direct_stride(out, N, n) : 0;
  const bool out_direct = out_interleaved ? ctx->host_reachable(ilv_host, n * ofb) : out_st != 0;
  r->d_in.reserve(cap * M);
  r->d_out.reserve(cap * N);
  if (po) {
    r->reserve_pcm_out(cap * ofb, !out_direct);
  } else {
    r->p_out.reserve(cap * N);
    if (out_interleaved) r->d_ilv.reserve(cap * N);
  }
  unsigned char *const ilv_dev = po ? r->d_pcm.p : reinterpret_cast<unsigned char *>(r->d_ilv.p);
  unsigned char *const ilv_pin = po ? r->p_pcm.p : reinterpret_cast<unsigned char *>(r->p_out.p);
  // planar rows [N][stride] of `len` frames at sample clock t0 -> the interleaved frames at ilv_dev + at * ofb
  auto launch_interleave = [&](const float *rows, size_t stride, size_t len, size_t at, int64_t t0) {
    if (po)
      launch_rows_to_pcm(*po, rows, stride, N, len, ilv_dev + at * ofb, ofb, 0, r->levels.peak.p, r->levels.clip.p, t0, ctx->stream);
    else
      launch_rows_to_frames(rows, stride, N, len, reinterpret_cast<float *>(ilv_dev + at * ofb), N, ctx->stream);
  };
  r->d_bytes.reserve(cap * fb + 16);  // (+16: the conversion kernel reads whole dwords)
  if (!direct) r->p_bytes.reserve(cap * fb);
  const unsigned char *src = static_cast<const unsigned char *>(frames);
  r->last_host_chunks = 0;
  if (plan.short_call) {
    if (!direct) {
      std::memcpy(r->p_bytes.p, frames, bytes);
      src = r->p_bytes.p;
    }
    EARHIP_HIP(hipMemcpyAsync(r->d_bytes.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    launch_pcm_to_rows(fmt, r->d_bytes.p, fb, first_byte, M, n, r->d_in.p, n, ctx->stream);
    if (out_interleaved) {
      const int64_t t0 = r->t;
      r->process_device(nblocks, r->d_in.p, n, r->d_out.p, n);
      launch_interleave(r->d_out.p, n, n, 0, t0);
      EARHIP_HIP(hipMemcpyAsync(out_direct ? ilv_host : ilv_pin, ilv_dev, n * ofb, hipMemcpyDeviceToHost, ctx->stream));
    } else {
      r->process_short_call(nblocks, out0, out_st);
    }
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    if (out_interleaved && !out_direct) std::memcpy(ilv_host, ilv_pin, n * ofb);
    if (!out_interleaved && !out_st) r->chunk_rows_scatter(out, 0, n);
    return;
  }
  // Long calls: the pipeline of earhip_render_process, on the packed bytes.  A chunk is one contiguous byte range of the caller's
  // buffer, staged into the pinned buffer at the same offset by the staging threads (pageable frames) or not at all; its kernels
  // are the conversion into the chunk's rows of d_in, then the chunk's render as an ordinary process call.
  r->pipe.begin(ctx->stream);
  GatherPool *gp = nullptr;
  if (!direct) {
    gp = &r->staging_threads();
    gp->submit_range(frames, r->p_bytes.p, fb, plan.cstart, plan.nch, ctx->get(OPT_HOST_BIND, 0) != 0, ctx->get(OPT_HOST_NT, 1) != 0);
    src = r->p_bytes.p;
  }
  run_host_chunks(
      r->pipe, gp, plan, !out_direct, &r->last_host_chunks,
      [&](size_t at, size_t len) {
        return hipMemcpyAsync(r->d_bytes.p + at * fb, src + at * fb, len * fb, hipMemcpyHostToDevice, r->pipe.in);
      },
      [&](size_t at, size_t len) {
        float *din = r->d_in.p + (size_t)M * at, *dout = r->d_out.p + (size_t)N * at;
        launch_pcm_to_rows(fmt, r->d_bytes.p + at * fb, fb, first_byte, M, len, din, len, ctx->stream);
        const int64_t t0 = r->t;
        r->process_device(len / r->B, din, len, dout, len);
        if (out_interleaved) launch_interleave(dout, len, len, at, t0);
      },
      [&](size_t at, size_t len) {
        if (!out_interleaved) return r->chunk_rows_d2h(out0, out_st, at, len);
        return hipMemcpyAsync((out_direct ? ilv_host : ilv_pin) + at * ofb, ilv_dev + at * ofb, len * ofb, hipMemcpyDeviceToHost, r->pipe.out);
      },
      [&](size_t at, size_t len) {
        if (out_interleaved) std::memcpy(ilv_host + at * ofb, ilv_pin + at * ofb, len * ofb);
        else r->chunk_rows_scatter(out, at, len);
      },
      [] { return 0.0; });
}

int earhip_render_process_frames(earhip_render *r, size_t nblocks, const void *frames, earhip_pcm_format fmt, int frame_channels,
                                 int first_channel, float *const *out, int out_interleaved) {
  return guarded([&] {
    check_frames_args(r, nblocks, frames, fmt, frame_channels, first_channel);
    require(out != nullptr, "out must not be NULL");
    for (int c = 0; c < (out_interleaved ? 1 : r->N); c++) require(out[c] != nullptr, "out must not be NULL");
    if (nblocks == 0) return;
    process_frames_host(r, nblocks, frames, fmt, frame_channels, first_channel, out, out_interleaved, nullptr, nullptr);
  });
}

int earhip_render_process_frames_device(earhip_render *r, size_t nblocks, const void *frames_dev, earhip_pcm_format fmt,
                                        int frame_channels, int first_channel, float *out_dev, size_t out_stride, int out_interleaved) {
  return guarded([&] {
    check_frames_args(r, nblocks, frames_dev, fmt, frame_channels, first_channel);
    require(out_dev != nullptr, "out_dev must not be NULL");
    require(out_interleaved ? out_stride >= (size_t)r->N : out_stride >= nblocks * r->B, "stride too small");
    if (nblocks == 0) return;
    const size_t n = r->frames_to_device_rows(nblocks, frames_dev, fmt, frame_channels, first_channel, out_interleaved != 0);
    if (out_interleaved) {
      r->process_device(nblocks, r->d_rows.p, n, r->d_rows_out.p, n);
      launch_rows_to_frames(r->d_rows_out.p, n, r->N, n, out_dev, out_stride, r->ctx->stream);
    } else {
      r->process_device(nblocks, r->d_rows.p, n, out_dev, out_stride);
    }
  });
}

int earhip_render_process_frames_pcm(earhip_render *r, size_t nblocks, const void *frames, earhip_pcm_format fmt, int frame_channels,
                                     int first_channel, void *out_frames, const earhip_pcm_out *out) {
  return guarded([&] {
    check_frames_args(r, nblocks, frames, fmt, frame_channels, first_channel);
    const size_t So = check_pcm_out(out);
    require(out_frames != nullptr, "out_frames must not be NULL");
    require(So == 3 || reinterpret_cast<uintptr_t>(out_frames) % So == 0, "out_frames not aligned to the sample size");
    if (nblocks == 0) return;
    process_frames_host(r, nblocks, frames, fmt, frame_channels, first_channel, nullptr, 1, out, out_frames);
  });
}

int earhip_render_process_frames_pcm_device(earhip_render *r, size_t nblocks, const void *frames_dev, earhip_pcm_format fmt,
                                            int frame_channels, int first_channel, void *out_dev, size_t out_frame_bytes,
                                            size_t out_first_byte, const earhip_pcm_out *out) {
  return guarded([&] {
    check_frames_args(r, nblocks, frames_dev, fmt, frame_channels, first_channel);
    check_pcm_out_frame(r->N, check_pcm_out(out), out_dev, out_frame_bytes, out_first_byte, "n_out");
    if (nblocks == 0) return;
    earhip_ctx *ctx = r->ctx;
    ctx->use();
    r->levels.reserve(r->N, ctx->stream);
    const size_t n = r->frames_to_device_rows(nblocks, frames_dev, fmt, frame_channels, first_channel, true);
    const int64_t t0 = r->t;
    r->process_device(nblocks, r->d_rows.p, n, r->d_rows_out.p, n);
    launch_rows_to_pcm(*out, r->d_rows_out.p, n, r->N, n, static_cast<unsigned char *>(out_dev), out_frame_bytes, out_first_byte,
                       r->levels.peak.p, r->levels.clip.p, t0, ctx->stream);
  });
}

int earhip_render_output_levels(earhip_render *r, float *peak, uint64_t *clipped, int reset) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    require(peak != nullptr && clipped != nullptr, "peak and clipped must not be NULL");
    earhip_ctx *ctx = r->ctx;
    ctx->use();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    r->levels.read(r->N, peak, clipped);  // (zeros before the first PCM-out call)
    if (reset) r->levels.zero(ctx->stream);
  });
}

/* diagnostic builds (-DEARHIP_K2_PROF) only: the s_memtime stamps wave 0 of two workgroups of the last k_decorrelate_wave launch
 * left at its phase boundaries, out[2][32]; an ordinary build reports "not built in" */
int earhip_debug_k2_prof(earhip_ctx *ctx, unsigned long long *out64) {
  return guarded([&] {
    require(ctx != nullptr && out64 != nullptr, "NULL argument");
#ifdef EARHIP_K2_PROF
    ctx->use();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    EARHIP_HIP(hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_k2_prof), sizeof(unsigned long long) * 64));
#else
    fail_invalid("this build has no K2 phase stamps (-DEARHIP_K2_PROF)");
#endif
  });
}

int earhip_render_enable_timing(earhip_render *r, int enable) {
  return guarded([&] {
    require(r != nullptr, "render must not be NULL");
    r->ctx->use();
    if (r->timing) r->drain_timing();
    r->timing = enable != 0;
    r->timing_every = enable > 1 ? enable : 1;
    r->timing_calls = 0;
    for (int i = 0; i < 3; i++) r->acc_ms[i] = r->acc_n[i] = 0;
  });
}

int earhip_render_get_timing(earhip_render *r, double out[6]) {
  return guarded([&] {
    require(r != nullptr && out != nullptr, "NULL argument");
    r->ctx->use();
    r->drain_timing();
    out[0] = r->acc_ms[0]; out[1] = r->acc_n[0];
    out[2] = r->acc_ms[1]; out[3] = r->acc_n[1];
    out[4] = r->acc_ms[2]; out[5] = r->acc_n[2];
  });
}

int earhip_render_gain_kernel(const earhip_render *r, int *kind) {
  return guarded([&] {
    require(r != nullptr && kind != nullptr, "NULL argument");
    *kind = r->report.kind;
  });
}

int earhip_render_hinge_standby(earhip_render *r, int *standby) {
  return guarded([&] {
    require(r != nullptr && standby != nullptr, "NULL argument");
    *standby = 0;
    if (r->report.kind != 5 || !r->report.gated || r->report.hg_robust) return;  // (robust form allowed: nobody stands by)
    *standby = (r->mode_word() & kGateHingeUnsafe) ? 1 : 0;
  });
}

int earhip_render_hinge_robust(earhip_render *r, int *robust) {
  return guarded([&] {
    require(r != nullptr && robust != nullptr, "NULL argument");
    *robust = 0;
    if (r->report.kind != 5 || !r->report.hg_robust) return;
    *robust = hinge_span_exceeded(r->mode_word(), r->M) ? 1 : 0;
  });
}

int earhip_render_wide_form(earhip_render *r, int *wide) {
  return guarded([&] {
    require(r != nullptr && wide != nullptr, "NULL argument");
    *wide = 1;
    if (r->report.kind < 3) *wide = -1;  // (no split operands at all)
    if (r->report.kind < 3 || !r->report.device_form) return;
    *wide = (r->mode_word() & 1u) ? 1 : 0;
  });
}

int earhip_render_scratch_bytes(const earhip_render *r, size_t *bytes) {
  return guarded([&] {
    require(r != nullptr && bytes != nullptr, "NULL argument");
    *bytes = r->report.scratch_bytes;
  });
}

int earhip_render_scratch_regrows(const earhip_render *r, long *count) {
  return guarded([&] {
    require(r != nullptr && count != nullptr, "NULL argument");
    *count = r->scratch_regrows;
  });
}

int earhip_render_last_tail_blocks(const earhip_render *r, int *blocks) {
  return guarded([&] {
    require(r != nullptr && blocks != nullptr, "NULL argument");
    *blocks = r->report.tail_blocks;
  });
}

int earhip_render_last_host_chunks(const earhip_render *r, int *chunks) {
  return guarded([&] {
    require(r != nullptr && chunks != nullptr, "NULL argument");
    *chunks = r->last_host_chunks;
  });
}

int earhip_render_last_list_layout(const earhip_render *r, int *paired) {
  return guarded([&] {
    require(r != nullptr && paired != nullptr, "NULL argument");
    *paired = r->report.paired;
  });
}

int earhip_render_last_plan(const earhip_render *r, int out[4]) {
  return guarded([&] {
    require(r != nullptr && out != nullptr, "NULL argument");
    out[0] = r->report.kind;
    for (int i = 0; i < 3; i++) out[1 + i] = r->report.plan[i];
  });
}

int earhip_render_last_decor_plan(const earhip_render *r, int out[4]) {
  return guarded([&] {
    require(r != nullptr && out != nullptr, "NULL argument");
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (r->K != 2) return;
    out[0] = r->decor.Bk;
    out[1] = r->decor.NP;
    out[2] = r->decor.last_form;
    out[3] = r->decor.last_R;
  });
}

}  // extern "C"
