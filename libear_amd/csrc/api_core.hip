// api_core.hip — context, error reporting, the interpolation-policy entry
// points (A) and the whole-curve GainInterpolator (A') of include/earhip.h.
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <string>
#include <memory>
#include <mutex>
#include <type_traits>

#include "common.h"
#include "curves.h"
#include "gain_kernels.h"
#include "gain_mfma.h"
#include "gain_h2.h"
#include "gain_h2_t1.h"
#include "gain_p2.h"
#include "gain_hg.h"
#include "gain_f32g.h"

namespace earhip {

static_assert(kSplitTile == 256, "MixLaunch::tile() and tiles_aligned(256, ...) assume the 4-wave tile");

static thread_local std::string g_last_error;
void set_last_error(const std::string &msg) { g_last_error = msg; }

// One of a fixed list of values as a compile-time constant: f(Int<V>{}) for the V that v equals.  Every launcher below turns its
// runtime shape (column tiles, waves, tiles per workgroup) into the template arguments of its kernel this way; the lists are
// the instantiations the library holds.
template <int V>
using Int = std::integral_constant<int, V>;
template <int... Vs, typename F>
static void dispatch(int v, F &&f) {
  if (!((v == Vs ? (f(Int<Vs>{}), true) : false) || ...)) fail_internal("no gain kernel instantiation for this launch plan");
}
template <int... Vs, typename F>
static void for_each(F &&f) {
  (f(Int<Vs>{}), ...);
}

// every instantiation of k_hinge_build, f(tiles per workgroup, waves of the gain kernel): its launch picks one, and
// hinge_build_allow_lds raises the LDS limit of each
template <typename F>
static void for_each_hinge_build(F &&f) {
  for_each<1, 2, 4, 8>([&](auto T) { f(T, Int<4>{}), f(T, Int<8>{}); });
}

// The context's words of one call of a split-operand kernel.  The two level words alternate between calls: this call's probe
// raises `level_cur` (zero since the last such call cleared it), its K1 reads it and clears `level_next`; the mode words (bit 0:
// the grid kernel's wide mode, bit 1: "not the hinge kernel") and the grid kernel's per-tile "some object needs the exact path
// here" words (gain_h2.h) alternate the same way.  Null: the call has no such word.
struct CallWords {
  unsigned *level_cur = nullptr, *level_next = nullptr;
  unsigned *wide_cur = nullptr, *wide_next = nullptr;  // "run this call in wide mode"; wide_cur null: the wide form, not decided on the device
  unsigned *gate = nullptr;                            // the call's mode word (the same word as wide_cur's)
  unsigned *slow_cur = nullptr, *slow_next = nullptr;
  unsigned *obj_level = nullptr;  // per-object levels of the probe (k_level_probe); null: no probe ran
  bool grew = false;
};

// The one place that makes or grows the context's words: level and mode words, the probe's per-object levels for M objects, the
// grid kernel's per-tile words for `ntiles` tiles (0: not needed; grown to tile_cap).  Returns how many buffers it made, behind
// a synchronisation (calls of other stages may be using the old ones).
static int grow_call_words(earhip_ctx *ctx, int M, size_t ntiles, size_t tile_cap) {
  int made = 0;
  if (M > 0 && !ctx->level.p) ctx->level.alloc_zero(4, ctx->stream), made++;  // [0..1] level words, [2..3] mode words
  const bool grow_obj = ctx->obj_level_cap < M, grow_tiles = ctx->tile_slow_cap < ntiles;
  if (grow_obj || grow_tiles) EARHIP_HIP(hipStreamSynchronize(ctx->stream));
  if (grow_obj) {  // (grown with the largest M this context has seen: contexts are shared by gain stages of different sizes)
    ctx->obj_level_cap = M + M / 2 + 64;
    ctx->obj_level.alloc_zero(2 * (size_t)ctx->obj_level_cap, ctx->stream);
    made++;
  }
  if (grow_tiles) {
    ctx->tile_slow_cap = std::max<size_t>(tile_cap, 1024);
    ctx->tile_slow.alloc_zero(2 * ctx->tile_slow_cap, ctx->stream);
    ctx->tile_slow_idx = 0;
    made++;
  }
  return made;
}

// What the split-operand kernels of a call of up to `max_samples` samples on M objects keep PER CONTEXT (tiles of 256 samples at
// the smallest), made where a renderer is created, so that no process call allocates or synchronises for them.
void reserve_call_words(earhip_ctx *ctx, int M, size_t max_samples) {
  const size_t ntiles = (max_samples + 255) / 256;
  grow_call_words(ctx, M, ntiles, ntiles + ntiles / 4);
}

// This call's turn of the words, and the level probe of its inputs in front of everything else (k_level_probe: 64 instants per
// object; rows must allow 16-byte loads; not with a fixed input scale, option XSCALE).  A gain stage that comes here before any
// renderer was created, or a call larger than any renderer of the context announced, grows the words here: counted in
// ctx->lazy_allocs and reported as `grew`.
static CallWords acquire_call_words(earhip_ctx *ctx, const MixLaunch &ml, int M, const float *in_dev, size_t in_stride, int nsamples) {
  CallWords w;
  if (!ml.split_operands()) return w;
  const bool probe = ctx->x_scale_auto && in_stride % 4 == 0 && ((uintptr_t)in_dev & 15) == 0;
  const size_t slow_tiles = ml.kind == GainKernel::Grid ? (size_t)ml.ntiles : 0;
  if (!probe && !slow_tiles) return w;
  if ((probe && (!ctx->level.p || ctx->obj_level_cap < M)) || ctx->tile_slow_cap < slow_tiles) {  // (not on a call a renderer announced)
    ctx->lazy_allocs += grow_call_words(ctx, probe ? M : 0, slow_tiles, 2 * slow_tiles);
    w.grew = true;
  }
  if (slow_tiles) {
    w.slow_cur = ctx->tile_slow.p + (size_t)ctx->tile_slow_idx * ctx->tile_slow_cap;
    w.slow_next = ctx->tile_slow.p + (size_t)(ctx->tile_slow_idx ^ 1) * ctx->tile_slow_cap;
    ctx->tile_slow_idx ^= 1;
  }
  if (!probe) return w;
  w.level_cur = ctx->level.p + ctx->level_idx;
  w.level_next = ctx->level.p + (ctx->level_idx ^ 1);
  // a short call (less than two rounds of workgroups: block mode) runs the wide form only: its latency does not
  // depend on the form, and the second launch — the form that returns at once — is 4-5 us of it
  // (every call clears the word the NEXT call decides with, whether it decides itself or not)
  if ((size_t)ml.ntiles * ml.gsplit >= 2 * (size_t)ctx->num_cus) w.wide_cur = ctx->level.p + 2 + ctx->level_idx;
  w.wide_next = ctx->level.p + 2 + (ctx->level_idx ^ 1);
  w.gate = ctx->level.p + 2 + ctx->level_idx;
  ctx->level_idx ^= 1;
  w.obj_level = ctx->obj_level.p;
  const int v = ctx->get(OPT_PROBE_RUNS);  // tuning knob: runs of consecutive samples per object (1 .. 64)
  const int probe_runs = v >= 1 && v <= 64 && (v & (v - 1)) == 0 ? v : 16;
  hipLaunchKernelGGL(k_level_probe, dim3((M + kProbeObjects - 1) / kProbeObjects), dim3(64 * kProbeObjects), 0, ctx->stream, in_dev,
                     in_stride, nsamples, M, w.level_cur, ctx->obj_level.p, ctx->obj_level_cap, probe_runs);
  return w;
}

// One call of the gain stage as its K0 and K1 functions see it.
struct MixCall {
  earhip_ctx *ctx;
  const CurveSet &cs;
  const MixLaunch &ml;
  const ColumnPlan &cp;
  PointStore ps;
  int M, nsamples;
  int64_t t_call;
  const float *in_dev;
  size_t in_stride;  // of the input rows
  SegDesc *scratch;  // laid out by `lay`
  ScratchLayout lay;
  SlotLists sl;   // the views of the scratch buffer the kind has (else zero)
  PieceLists pl;  // (Hinge: the lists standing by)
  HingeLists hl;
  CallWords w;
  // hinge kernel: what a call whose levels spread beyond the packed-f16 kink products' span gets — the kernel's robust form
  // (default) or, option HG_ROBUST = 0, the piece lists standing by behind it (rounds 4-5): built and launched behind the hinge
  // kernel's, for the call it may not take
  bool hg_robust = false, standby = false;
  GainMixParams P;  // (K1)
  hipStream_t stream() const { return ctx->stream; }
  int64_t t_end() const { return t_call + nsamples; }
  unsigned *gate_word(bool robust) const { return hg_robust == robust ? w.gate : nullptr; }  // (k_hinge_*: [..., gate, robust gate])
  unsigned *standby_gate() const { return ml.kind == GainKernel::Hinge ? w.gate : nullptr; }
  // (the piece lists have tiles of 64 pw samples — behind the hinge kernel whatever its own)
  int piece_tile() const { return 64 * ml.pw; }
  int piece_tiles() const { return lay.piece_tiles; }
  float x_scale() const { return std::ldexp(1.0f, ctx->x_scale_log2); }
  // workgroups of a split-operand kernel's grid, z: column groups
  dim3 tile_grid(int x) const { return dim3(x, ml.gsplit, cp.mnz * cp.mgroups); }
};

// ---- K0

// hinge kernel: the device's decision whose call this is (k_hinge_gate), then its own list builder (k_hinge_build, gain_hg.h)
static void prep_hinge_lists(const MixCall &c) {
  earhip_ctx *ctx = c.ctx;
  const MixLaunch &ml = c.ml;
  const int M = c.M, nw = ml.tile() / 64;
  if (M > kMaxHingeCached || (nw != 4 && nw != 8)) fail_internal("hinge lists: object count or tile out of range");
  // (the kernel addresses input rows and gain rows with 32-bit byte offsets; plan_mix only picks it within these limits)
  if (!c.ps.kink_row0) fail_internal("hinge kernel: the curve set has no kink rows");
  if (!hinge_addressable(M, c.in_stride, c.nsamples, (size_t)c.ps.kink_row0 + c.ps.rows, c.ps.row)) fail_internal("hinge kernel: buffers beyond its 32-bit offsets");
  // with a probe: does the hinge kernel's span of levels cover this call?
  if (c.w.gate)
    hipLaunchKernelGGL(k_hinge_gate, dim3((M + 255) / 256), dim3(256), 0, c.stream(), c.w.obj_level, ctx->obj_level_cap, M, c.w.level_cur, c.w.gate,
                       c.w.wide_cur != nullptr, c.hg_robust);
  int tpw = 1;
  const size_t cached_max = std::min((size_t)kMaxHingeCached, ctx->hinge_build_lds / sizeof(HingeCached));  // (pairs a workgroup may keep)
  if ((size_t)M > cached_max) fail_internal("hinge lists: more objects than the builder's LDS holds on this device");
  while (tpw < 8 && ml.ntiles / (2 * tpw) >= ctx->num_cus && (size_t)M * (2 * tpw) <= cached_max) tpw *= 2;
  if (ctx->has(OPT_HBUILD_TPW)) {  // tuning knob
    const int v = ctx->get(OPT_HBUILD_TPW);
    if ((v == 1 || v == 2 || v == 4 || v == 8) && (size_t)M * v <= cached_max) tpw = v;
  }
  // two kernels (option BUILD_2K = 1; NOT the default here): k_hinge_classify object-major into the staging matrix behind the
  // lists, then the builder from its counting loop on, without the LDS its first pass kept its results in.  Measured: classify
  // 21 us + the builder's second half 42 us against 58 us in one kernel — that half (ranking by ballots over 32 classes between
  // three barriers per batch, two scattered 16-byte stores per pair) is what the builder is made of, and it does not get faster
  // at two workgroups per CU.  The lists are the same bit for bit (tests run both).
  HingeCached *stage = nullptr;
  if (ctx->get(OPT_BUILD_2K, 0) != 0) {
    stage = c.lay.hinge_staging(c.scratch);
    const dim3 cgrid((ml.ntiles + 63) / 64, (M + kClassifyObjects - 1) / kClassifyObjects);
    dispatch<4, 8>(nw, [&](auto NW) {
      hipLaunchKernelGGL((k_hinge_classify<decltype(NW)::value>), cgrid, dim3(64 * kClassifyObjects), 0, c.stream(), c.ps, M, ml.ntiles, c.t_call,
                         c.t_end(), stage, c.w.obj_level, c.w.level_cur, c.gate_word(false), c.gate_word(true));
    });
    if (!ctx->has(OPT_HBUILD_TPW)) {
      tpw = 1;
      while (tpw < 8 && ml.ntiles / (2 * tpw) >= 2 * ctx->num_cus) tpw *= 2;
    }
  }
  const dim3 bgrid((ml.ntiles + tpw - 1) / tpw);
  // (more than 64 KB of dynamic LDS has to be asked for, per device and instantiation: earhip_ctx_create does, hinge_build_allow_lds)
  const size_t lds = stage ? 0 : sizeof(HingeCached) * (size_t)M * tpw;
  for_each_hinge_build([&](auto T, auto NW) {
    if (tpw == T && nw == NW)
      hipLaunchKernelGGL((k_hinge_build<decltype(T)::value, decltype(NW)::value>), bgrid, dim3(kHingeBuildThreads), lds, c.stream(), c.ps, M, ml.ntiles,
                         c.t_call, c.t_end(), c.hl, c.w.obj_level, c.w.level_cur, c.gate_word(false), c.gate_word(true), (const HingeCached *)stage);
  });
}

// piece-list kernel: ONE pass builds the lists (k_piece_build, gain_p2.h) behind the probe launch — the call's own, or those
// standing by behind the hinge kernel's
static void prep_piece_lists(const MixCall &c) {
  earhip_ctx *ctx = c.ctx;
  const MixLaunch &ml = c.ml;
  const int M = c.M, ptile = c.piece_tile(), pnt = c.piece_tiles();
  if (M > kMaxPieceObjects || ptile > kPieceMaxTile) fail_internal("piece lists: object index or tile out of range");
  // tiles per workgroup: as many as leave one workgroup per CU (eight tiles = eight lanes per object reading
  // neighbouring points beat four tiles and two workgroups per CU: 0.084 vs 0.096 ms on the ADM scene)
  int tpw = 1;
  while (tpw < 8 && pnt / (2 * tpw) >= ctx->num_cus) tpw *= 2;
  if (ctx->has(OPT_BUILD_TPW)) {  // tuning knob
    const int v = ctx->get(OPT_BUILD_TPW);
    if (v == 1 || v == 2 || v == 4 || v == 8) tpw = v;
  }
  const PieceLists &pl = c.pl;
  // two kernels (option BUILD_2K; the one-pass builder otherwise): classify object-major into the staging matrix behind the
  // lists, then place tile-major
  // (default: where the lists are PAIRED — curves that hold most of the time: at most one ramp per object and tile nearly
  // everywhere, which the staged pair carries; always-ramping curves on packed lists have several per pair, the placing kernel
  // would walk most pairs itself: 0.097 against 0.076 ms, measured)
  PairRec *stage = nullptr;
  if (ctx->has(OPT_BUILD_2K) ? ctx->get(OPT_BUILD_2K) != 0 : ml.paired) {
    stage = c.lay.piece_staging(c.scratch);
    hipLaunchKernelGGL(k_piece_classify, dim3((pnt + 63) / 64, (M + kClassifyObjects - 1) / kClassifyObjects), dim3(64 * kClassifyObjects), 0,
                       c.stream(), c.ps, M, pnt, ptile, c.t_call, c.t_end(), pl.paired, stage, c.w.obj_level, c.w.level_cur, c.standby_gate());
  }
  dispatch<1, 2, 4, 8>(tpw, [&](auto T) {
    hipLaunchKernelGGL(k_piece_build<decltype(T)::value>, dim3((pnt + tpw - 1) / tpw), dim3(kBuildThreads), 0, c.stream(), c.ps, M, pnt, ptile, c.t_call,
                       c.t_end(), pl, c.w.obj_level, c.w.level_cur, c.standby_gate(), ctx->obj_level_cap, c.w.wide_cur, stage);
  });
}

// segment descriptors (k_seg_prep: 16 lanes per object search its curve), with what the probe found marked in them as they are made
static void prep_descriptors(const MixCall &c) {
  const MixLaunch &ml = c.ml;
  const unsigned objs = (unsigned)(c.M + 15) / 16;
  QuietMark qm;
  if (c.w.obj_level) {
    qm.obj_level = c.w.obj_level, qm.cap = c.ctx->obj_level_cap, qm.level = c.w.level_cur;
    qm.wide = ml.kind == GainKernel::Grid ? c.w.wide_cur : nullptr;
  }
  if (ml.ntiles >= 2048)
    hipLaunchKernelGGL(k_seg_prep<4>, dim3((ml.ntiles + 63) / 64, objs), dim3(256), 0, c.stream(), c.ps, c.M, ml.ntiles, ml.tile(), c.t_call,
                       c.t_end(), c.scratch + c.lay.desc.at, qm, c.w.slow_cur);
  else
    hipLaunchKernelGGL(k_seg_prep<2>, dim3((ml.ntiles + 31) / 32, objs), dim3(256), 0, c.stream(), c.ps, c.M, ml.ntiles, ml.tile(), c.t_call,
                       c.t_end(), c.scratch + c.lay.desc.at, qm, c.w.slow_cur);
}

// f32 MFMA kernel: K0s turns the descriptors into the tiles' slot lists; `own_search`: it finds the segments itself
static void prep_slot_lists(const MixCall &c, bool own_search) {
  hipLaunchKernelGGL(k_slot_list, dim3(c.ml.ntiles), dim3(256), 0, c.stream(), c.ps, c.M, c.ml.tile(), c.t_call, c.t_end(),
                     own_search ? nullptr : c.scratch + c.lay.desc.at, c.sl);
}

// ---- K1

static void launch_valu(const MixCall &c, bool strict) {
  const ColumnPlan &cp = c.cp;
  const dim3 grid(c.ml.ntiles, c.ml.gsplit, cp.nz), block(64 * cp.ngroups * c.ml.wsplit);
  const size_t lds = c.ml.wsplit > 1 ? (size_t)cp.ngroups * cp.nout * c.ml.tile() * sizeof(float) : 0;  // (the object splits' sums)
  dispatch<4, 2>(c.ml.spl, [&](auto SPL) {
    dispatch<8, 16, 24>(cp.nout, [&](auto NOUT) {
      constexpr int spl = decltype(SPL)::value, nout = decltype(NOUT)::value;
      if (!strict) hipLaunchKernelGGL((k_gain_mix<nout, spl, false>), grid, block, lds, c.stream(), c.P);
      else hipLaunchKernelGGL((k_gain_mix<nout, spl, true>), grid, block, lds, c.stream(), c.P);
    });
  });
}

static void launch_slots(const MixCall &c) {
  const ColumnPlan &cp = c.cp;
  const MixLaunch &ml = c.ml;
  const dim3 grid((ml.ntiles + ml.tpw - 1) / ml.tpw, ml.gsplit, cp.mnz), block(64 * cp.mgroups * ml.tpw * ml.wsplit);
  const size_t lds = ml.wsplit > 1 ? (size_t)cp.mgroups * ml.tpw * cp.nct * 16 * ml.tile() * sizeof(float) : 0;
  dispatch<8, 4>(ml.nrt, [&](auto NRT) {
    dispatch<1, 2, 3>(cp.nct, [&](auto NCT) {
      hipLaunchKernelGGL((k_gain_mix_mfma<decltype(NCT)::value, decltype(NRT)::value>), grid, block, lds, c.stream(), c.P);
    });
  });
}

// exact f32 on the tile grid (gain_f32g.h): a workgroup per 512-sample tile, descriptors from k_seg_prep
static void launch_f32grid(const MixCall &c) {
  if (c.nsamples % kF32GridTile != 0) fail_internal("f32 grid kernel: the call is not whole tiles");
  dispatch<1, 2, 3>(c.cp.nct, [&](auto NCT) {
    hipLaunchKernelGGL((k_gain_mix_f32g<decltype(NCT)::value>), c.tile_grid(c.ml.ntiles), dim3(512), 0, c.stream(), c.P, c.ps.zero_row);
  });
}

static void launch_grid(const MixCall &c) {
  earhip_ctx *ctx = c.ctx;
  const ColumnPlan &cp = c.cp;
  const MixLaunch &ml = c.ml;
  const CallWords &w = c.w;
  // as many workgroups as are resident at once (a multiple of 8: a workgroup's tiles stay on its XCD), each working
  // through its share of the tiles in one software pipeline (gain_h2.h)
  const int per_cu = ml.tile() == 512 ? 1 : (cp.nct == 1 ? 3 : 2);  // (the 8-wave forms: 154-243 registers, one workgroup per CU)
  int wgs = std::max(8, (ctx->num_cus * per_cu / std::max(1, ml.gsplit * cp.mnz * cp.mgroups)) & ~7);
  if (ctx->has(OPT_H2_WGS)) wgs = std::max(1, ctx->get(OPT_H2_WGS));  // tuning knob
  wgs = std::max(wgs, ((ml.ntiles + 63) / 64 + 7) & ~7);  // (at most 64 tiles per workgroup: its redo mask)
  if (!h2_persistent(cp.nct, ml.tile() == 512 ? 8 : 4)) wgs = ml.ntiles;  // (a tile per workgroup)
  GainMixParams P = c.P;
  // a workgroup's tiles as one contiguous run (option H2_RUNS: 1 on, 0 off; default: the single-column-tile forms — config 2)
  P.tile_runs = ctx->has(OPT_H2_RUNS) ? (ctx->get(OPT_H2_RUNS) != 0) : 0;
  const dim3 grid = c.tile_grid(std::min(ml.ntiles, wgs));
  const float xs = c.x_scale();
  const float *gs = c.cs.column_scales();
  // two forms of the kernel: the 8-wave kernel carries both and branches on the device-side mode word (round 6); the 4-wave
  // kernels are launched as a pair, back to back: the form the word names runs, the other returns at once
  // (gain_h2.h; the piece-list and hinge kernels carry both forms in one kernel — for this one the merged kernel measured
  // slower: config 2 0.224 -> 0.259 ms, its 4-wave form loses a wave per SIMD to the larger of the two register counts);
  // without a probe only the wide form
  const bool two_launches = ctx->get(OPT_H2_PAIR, 0) != 0;  // (tuning knob: the 8-wave kernel as a pair of launches, as until round 6)
  auto h2 = [&](auto NCT, auto NW, auto WIDE) {
    hipLaunchKernelGGL((k_gain_mix_h2<decltype(NCT)::value, decltype(NW)::value, decltype(WIDE)::value>), grid, dim3(64 * decltype(NW)::value), 0,
                       c.stream(), P, c.ps.zero_row, xs, gs, w.level_cur, w.level_next, w.slow_cur, w.slow_next, w.wide_cur, w.wide_next);
  };
  auto h2_t1 = [&](auto NCT, auto WIDE) {
    hipLaunchKernelGGL((k_gain_mix_h2_t1<decltype(NCT)::value, 4, decltype(WIDE)::value>), grid, dim3(256), 0, c.stream(), P, c.ps.zero_row, xs, gs,
                       w.level_cur, w.level_next, w.slow_cur, w.slow_next, w.wide_cur, w.wide_next);
  };
  // (the kernel's third argument: 0 the plain form, 1 the wide form, 2 both, picked on the device)
  dispatch<1, 2, 3>(cp.nct, [&](auto NCT) {
    if (ml.tile() == 512) {
      if (w.wide_cur && !two_launches) return h2(NCT, Int<8>{}, Int<2>{});
      if (w.wide_cur) h2(NCT, Int<8>{}, Int<0>{});
      h2(NCT, Int<8>{}, Int<1>{});
    } else if (NCT == 1) {
      // (a plain `if`, as it has always been: k_gain_mix_h2_t1<1, 4, *> stays in the library though nothing launches it — the set
      // of instantiated kernels is not this function's to change)
      if (w.wide_cur) h2(Int<1>{}, Int<4>{}, Int<0>{});
      h2(Int<1>{}, Int<4>{}, Int<1>{});
    } else {
      if (w.wide_cur) h2_t1(NCT, std::false_type{});
      h2_t1(NCT, std::true_type{});
    }
  });
}

static void launch_pieces(const MixCall &c) {
  earhip_ctx *ctx = c.ctx;
  const ColumnPlan &cp = c.cp;
  const MixLaunch &ml = c.ml;
  const CallWords &w = c.w;
  const int pnt = c.piece_tiles();
  // as many workgroups as are resident at once (a multiple of 8: a workgroup's tiles stay on its XCD), each carrying its
  // pipeline from one tile's list into the next (gain_p2.h); option P2_WGS: that number (0: a workgroup per tile)
  int wgs = std::max(8, (ctx->num_cus * (ml.pw == 4 ? 2 : 1) / std::max(1, ml.gsplit * cp.mnz * cp.mgroups)) & ~7);
  if (ctx->has(OPT_P2_WGS)) wgs = ctx->get(OPT_P2_WGS) > 0 ? ctx->get(OPT_P2_WGS) : pnt;
  if (!p2_persistent(cp.nct, ml.pw, ml.paired)) wgs = pnt;  // (a tile per workgroup)
  const dim3 grid = c.tile_grid(std::min(pnt, wgs));
  const float xs = c.x_scale();
  const float *gs = c.cs.column_scales();
  // (both forms of the kernel body in one kernel: the device-side mode word picks; without a probe the wide form)
  dispatch<0, 1>(ml.paired ? 1 : 0, [&](auto PAIRED) {
    dispatch<1, 2, 3>(cp.nct, [&](auto NCT) {
      dispatch<4, 8>(ml.pw == 4 ? 4 : 8, [&](auto NW) {
        constexpr int nw = decltype(NW)::value;
        hipLaunchKernelGGL((k_gain_mix_p2<decltype(NCT)::value, nw, decltype(PAIRED)::value != 0>), grid, dim3(64 * nw), 0, c.stream(), c.P, c.pl, xs, gs,
                           w.level_cur, w.level_next, w.wide_cur, w.wide_next, c.standby_gate(), pnt);
      });
    });
  });
}

static void launch_hinge(const MixCall &c) {
  const CallWords &w = c.w;
  const float xs = c.x_scale();
  const float *gs = c.cs.column_scales();
  dispatch<1, 2, 3>(c.cp.nct, [&](auto NCT) {
    dispatch<4, 8>(c.ml.tile() == 256 ? 4 : 8, [&](auto NW) {
      constexpr int nw = decltype(NW)::value;
      hipLaunchKernelGGL((k_gain_mix_hg<decltype(NCT)::value, nw>), c.tile_grid(c.ml.ntiles), dim3(64 * nw), 0, c.stream(), c.P, c.hl, xs, gs, w.level_cur,
                         w.level_next, w.wide_cur, w.wide_next, c.gate_word(false), c.gate_word(true));
    });
  });
}

// the parameter block of K1
static GainMixParams mix_params(const MixCall &c, float *out_dev, size_t out_stride, size_t part_stride, unsigned *record) {
  const float *in_dev = c.in_dev;
  const size_t in_stride = c.in_stride;
  const bool valu = c.ml.kind == GainKernel::Valu;
  GainMixParams P;
  P.mode_word = c.w.gate;
  P.record = c.w.gate ? record : nullptr;
  P.sl = c.sl;
  P.in = in_dev;
  P.in_stride = in_stride;
  P.out = out_dev;
  P.out_stride = out_stride;
  P.part_stride = part_stride;
  P.desc = c.scratch;
  P.ps = c.ps;
  P.t_call = c.t_call;
  P.nsamples = c.nsamples;
  P.ntiles = c.ml.ntiles;
  P.M = c.M;
  P.ncols = c.cs.ncols();
  P.ngroups = valu ? c.cp.ngroups : c.cp.mgroups;
  P.wsplit = c.ml.wsplit;
  P.tiles_per_wg = valu ? 1 : c.ml.tpw;
  P.vec_ok = in_stride % 4 == 0 && out_stride % 4 == 0 && part_stride % 4 == 0 && ((uintptr_t)in_dev & 15) == 0 && ((uintptr_t)out_dev & 15) == 0;
  return P;
}

// K0 (the probe, then what the kind's K1 reads: descriptors or lists, in the call's scratch buffer) + K1
MixResult launch_gain_mix(earhip_ctx *ctx, const CurveSet &cs, const MixLaunch &ml, bool strict, int64_t t_call, int nsamples,
                          const float *in_dev, size_t in_stride, float *out_dev, size_t out_stride, size_t part_stride, SegDesc *desc,
                          unsigned *record, hipEvent_t *ev) {
  const GainKernel kind = ml.kind;
  MixCall c{ctx, cs, ml, cs.plan(), cs.device(), cs.M(), nsamples, t_call, in_dev, in_stride, desc, scratch_layout(cs, ml, cs.M(), nsamples)};
  if (kind == GainKernel::Slots) c.sl = c.lay.slot_lists(desc);
  if (kind == GainKernel::Pieces || kind == GainKernel::Hinge) c.pl = c.lay.piece_lists(desc, ml.paired);
  if (kind == GainKernel::Hinge) c.hl = c.lay.hinge_lists(desc);
  if (kind == GainKernel::Slots && c.M > kMaxSlotObjects) fail_internal("slot lists address objects with 16 bits");
  if (ev) EARHIP_HIP(hipEventRecord(ev[0], ctx->stream));
  c.w = acquire_call_words(ctx, ml, c.M, in_dev, in_stride, nsamples);
  c.hg_robust = kind == GainKernel::Hinge && ctx->get(OPT_HG_ROBUST, 1) != 0;
  c.standby = kind == GainKernel::Hinge && c.w.gate && !c.hg_robust;
  switch (kind) {
    case GainKernel::Hinge:
      prep_hinge_lists(c);
      if (c.standby) prep_piece_lists(c);
      break;
    case GainKernel::Pieces: prep_piece_lists(c); break;
    case GainKernel::Slots: {
      // short curves (static or nearly static gains, <= 8 points per object on average): K0s finds the segments itself and the
      // descriptor pass is skipped; with long curves the 16-lanes-per-object search of k_seg_prep is the faster one (measured both ways)
      const bool own_search = (size_t)c.ps.npoints <= (size_t)8 * c.M;
      if (!own_search) prep_descriptors(c);
      prep_slot_lists(c, own_search);
      break;
    }
    default: prep_descriptors(c); break;
  }
  if (ev) EARHIP_HIP(hipEventRecord(ev[1], ctx->stream));
  c.P = mix_params(c, out_dev, out_stride, part_stride, record);
  if (ev) EARHIP_HIP(hipEventRecord(ev[2], ctx->stream));
  switch (kind) {
    case GainKernel::Valu: launch_valu(c, strict); break;
    case GainKernel::Slots: launch_slots(c); break;
    case GainKernel::F32Grid: launch_f32grid(c); break;
    case GainKernel::Grid: launch_grid(c); break;
    case GainKernel::Pieces: launch_pieces(c); break;
    case GainKernel::Hinge:
      launch_hinge(c);
      if (c.standby) launch_pieces(c);
      break;
  }
  if (ev) EARHIP_HIP(hipEventRecord(ev[3], ctx->stream));
  EARHIP_HIP(hipGetLastError());
  MixResult res;
  res.gated = kind == GainKernel::Hinge && c.w.gate;
  res.device_form = c.w.wide_cur != nullptr;
  res.hinge_robust = res.gated && c.hg_robust;
  res.grew = c.w.grew;
  return res;
}

// k_hinge_build keeps up to 128 KB of dynamic LDS per workgroup: the limit is an attribute of the function ON A DEVICE, so
// every context raises it for its own device when it is created (a process-wide "done" flag left the other GPUs of a
// multi-GPU process at the default 64 KB: launches with more failed there).
// Returns the dynamic LDS a launch of the builder may ask for on this device: `want` (128 KB) where the device has it, else
// what it allows (a device or runtime that refuses the attribute: the 64 KB every kernel has) — the launch picks its tiles
// per workgroup within that (a limit, never a reason for context creation to fail).
size_t hinge_build_allow_lds(const hipDeviceProp_t &prop) {
  const size_t want = 128 * 1024, dflt = 64 * 1024;
  const size_t device_max = std::max((size_t)prop.sharedMemPerBlock, (size_t)prop.maxSharedMemoryPerMultiProcessor);
  size_t ask = std::min(want, device_max > 4096 ? device_max - 4096 : dflt);  // (the kernel's static arrays: ~3 KB)
  if (ask <= dflt) return dflt;
  bool ok = true;
  for_each_hinge_build([&](auto T, auto NW) {
    ok = ok && hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hinge_build<decltype(T)::value, decltype(NW)::value>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)ask) == hipSuccess;
  });
  if (!ok) (void)hipGetLastError();  // (refused: the default limit stands)
  return ok ? ask : dflt;
}

// Device-resident M -> N gain stage with host staging; shared by the policy
// entry points and by earhip_gain_interp.
struct GainStage {
  earhip_ctx *ctx;
  int n_in, n_out;
  CurveSet curves;
  DevBuf<SegDesc> desc;
  DevBuf<float> parts;  // grid-level partial slabs
  std::vector<float> rows;  // scratch of the policy entry points (two gain rows)
  bool force_ramp;
  GainStage(earhip_ctx *c, int ni, int no, bool ramp = false)
      : ctx(c), n_in(ni), n_out(no), curves(ni, no, 1, ramp), force_ramp(ramp) {}

  // in_dev [n_in][in_stride] -> out_dev [n_out][out_stride]
  void run_device(int64_t t_call, int nsamples, const float *in_dev, size_t in_stride,
                  float *out_dev, size_t out_stride) {
    curves.commit(ctx);
    // 1 -> N policies have no accumulation: always use libear's exact arithmetic.  The policy entry points
    // (force_ramp: one ramp per input, extrapolated outside its two points) run it as well: only the VALU kernel's
    // segment descriptors express such a curve (describe_segment's policy mode); the matrix-core kernels' list builders
    // computed something else outside [start, end) for 32 inputs and more.
    const bool strict = ctx->strict || n_in == 1 || force_ramp;
    const MixLaunch ml = plan_mix(ctx, curves.plan(), n_in, nsamples, strict, 32, curves.stats(t_call, in_stride, (size_t)nsamples, false));
    if (ml.kind == GainKernel::Hinge) curves.ensure_kinks(ctx);
    desc.reserve(scratch_units(curves, ml, n_in));
    const size_t row_stride = ((size_t)nsamples + 3) & ~(size_t)3;
    if (ml.gsplit > 1) parts.reserve(row_stride * n_out * ml.gsplit);
    launch_gain_mix_summed(ctx, curves, ml, strict, t_call, nsamples, in_dev, in_stride, out_dev, out_stride, parts.p, row_stride, desc.p,
                           nullptr, nullptr);
  }

  // host planar pointers, samples [r0, r1) of each channel
  void run_host(int64_t t_call, const float *const *in, float *const *out, int64_t r0,
                int64_t r1) {
    const int n = (int)(r1 - r0);
    if (n <= 0) return;
    const size_t stride = ((size_t)n + 3) & ~(size_t)3;
    ctx->pin_in.reserve(stride * n_in);
    ctx->pin_out.reserve(stride * n_out);
    ctx->dev_in.reserve(stride * n_in);
    ctx->dev_out.reserve(stride * n_out);
    for (int c = 0; c < n_in; c++)
      std::memcpy(ctx->pin_in.p + c * stride, in[c] + r0, sizeof(float) * n);
    EARHIP_HIP(hipMemcpyAsync(ctx->dev_in.p, ctx->pin_in.p, sizeof(float) * stride * n_in,
                              hipMemcpyHostToDevice, ctx->stream));
    run_device(t_call, n, ctx->dev_in.p, stride, ctx->dev_out.p, stride);
    EARHIP_HIP(hipMemcpyAsync(ctx->pin_out.p, ctx->dev_out.p, sizeof(float) * stride * n_out,
                              hipMemcpyDeviceToHost, ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < n_out; c++)
      std::memcpy(out[c] + r0, ctx->pin_out.p + c * stride, sizeof(float) * n);
  }
};

}  // namespace earhip

using namespace earhip;

// keys of earhip_ctx_set_option (and, prefixed with EARHIP_, the environment variables read at earhip_ctx_create)
static const char *const kOptNames[OPT_COUNT] = {
    "SPL", "MFMA", "XSCALE", "WAVES", "TPW", "NRT", "H2_TILE", "H2_WGS", "H2_RUNS", "P2_TILE", "P2_PAIRS", "P2_WGS", "HINGE", "HG_TILE", "HBUILD_TPW",
    "BUILD_TPW", "K2_WG", "K2_OWN_BLOCK", "RUN", "GSPLIT", "PROBE_RUNS", "BLOCK_GROUPS", "DEBUG_TIMING", "TAILCUT", "HOST_CHUNK_MB", "HOST_THREADS", "HG_ROBUST", "BUILD_2K", "HOST_BIND", "HOST_NT", "HOST_FIRST", "H2_PAIR"};

// an option's value: a decimal integer (optional sign, surrounding blanks), nothing else — "abc" or "1x" used to read as 0 / 1
static int parse_option_value(const std::string &key, const char *text) {
  char *end = nullptr;
  errno = 0;
  const long v = std::strtol(text, &end, 10);
  while (end && *end && std::isspace((unsigned char)*end)) end++;
  if (end == text || (end && *end) || errno == ERANGE || v < -(1L << 30) || v > (1L << 30))
    fail_invalid("option '" + key + "': '" + std::string(text) + "' is not an integer");
  return (int)v;
}

void earhip_ctx::apply_options() {
  spl = 4, use_mfma = 3, x_scale_log2 = 14, x_scale_auto = true, max_waves = 4, tiles_per_wg = 4, tiles_per_wg_forced = false, nrt = 8;
  if (has(OPT_SPL) && (get(OPT_SPL) == 2 || get(OPT_SPL) == 4)) spl = get(OPT_SPL);  // samples per lane in gain_mix
  if (has(OPT_MFMA)) use_mfma = get(OPT_MFMA);
  if (has(OPT_XSCALE) && get(OPT_XSCALE) >= -64 && get(OPT_XSCALE) <= 64)  // f16x2 kernel: log2 of the input prescale
    x_scale_log2 = get(OPT_XSCALE), x_scale_auto = false;
  if (has(OPT_WAVES) && get(OPT_WAVES) >= 1 && get(OPT_WAVES) <= 8) max_waves = get(OPT_WAVES);
  if (has(OPT_TPW) && get(OPT_TPW) >= 1 && get(OPT_TPW) <= 8) tiles_per_wg = get(OPT_TPW), tiles_per_wg_forced = true;
  if (has(OPT_NRT) && (get(OPT_NRT) == 4 || get(OPT_NRT) == 8)) nrt = get(OPT_NRT);
}

struct earhip_gain_interp {
  std::unique_ptr<GainStage> stage;
};

// policy scratch: one GainStage per (n_in, n_out) shape seen on this context
struct PolicyCache {
  std::vector<std::unique_ptr<GainStage>> stages;
  GainStage *get(earhip_ctx *ctx, int n_in, int n_out, bool ramp) {
    for (auto &s : stages)
      if (s->n_in == n_in && s->n_out == n_out && s->force_ramp == ramp) return s.get();
    stages.emplace_back(new GainStage(ctx, n_in, n_out, ramp));
    return stages.back().get();
  }
};
static std::vector<std::pair<earhip_ctx *, std::unique_ptr<PolicyCache>>> g_policy;
static std::mutex g_policy_mutex;  // contexts are single-owner, the table of them is shared by all threads
static PolicyCache *policy_cache(earhip_ctx *ctx) {
  std::lock_guard<std::mutex> lock(g_policy_mutex);
  for (auto &p : g_policy)
    if (p.first == ctx) return p.second.get();
  g_policy.emplace_back(ctx, std::unique_ptr<PolicyCache>(new PolicyCache));
  return g_policy.back().second.get();
}

static __global__ void k_clock_probe(unsigned long long *out) {
  out[0] = clock64();       // shader clock (s_memtime)
  out[1] = wall_clock64();  // constant-rate counter
}

// Read-bandwidth probes (earhip_debug_read_bandwidth): what this chip delivers to a kernel that does
// nothing but read, (a) one linear stream, (b) the gain stage's pattern — every workgroup reads a 1 KB
// piece of each of `rows` rows that lie `stride` floats apart, 32 rows in flight per wave.
static __global__ void __launch_bounds__(256) k_read_linear(const f32x4 *in, float *out, size_t n4) {
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t step = (size_t)gridDim.x * 256;
  for (; i + 3 * step < n4; i += 4 * step) {
    const f32x4 a = __builtin_nontemporal_load(in + i), b = __builtin_nontemporal_load(in + i + step);
    const f32x4 c = __builtin_nontemporal_load(in + i + 2 * step), d = __builtin_nontemporal_load(in + i + 3 * step);
    acc += (a + b) + (c + d);
  }
  for (; i < n4; i += step) acc += __builtin_nontemporal_load(in + i);
  if (acc[0] + acc[1] + acc[2] + acc[3] == 123.456f) out[0] = 1.0f;  // (keeps the loads alive)
}
static __global__ void __launch_bounds__(256) k_read_rows(const float *in, float *out, int rows, size_t stride) {
  constexpr int DEPTH = 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, kg = lane >> 4;
  const float *base = in + (size_t)blockIdx.x * 256 + w * 64 + li * 4;
  auto row = [&](int r) { return base + (size_t)min(r, rows - 1) * stride; };
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 ring[DEPTH][8];
#pragma unroll
  for (int d = 0; d < DEPTH; d++)
#pragma unroll
    for (int q = 0; q < 8; q++)
      ring[d][q] = __builtin_nontemporal_load((const f32x4 *)row(d * 32 + kg * 8 + q));
  for (int r0 = 0; r0 < rows; r0 += 32 * DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
#pragma unroll
      for (int q = 0; q < 8; q++) acc += ring[d][q];
      const int rn = r0 + 32 * DEPTH + d * 32;
      if (rn < rows)
#pragma unroll
        for (int q = 0; q < 8; q++)
          ring[d][q] = __builtin_nontemporal_load((const f32x4 *)row(rn + kg * 8 + q));
    }
  }
  if (acc[0] + acc[1] + acc[2] + acc[3] == 123.456f) out[0] = 1.0f;
}

extern "C" {

// Measurement aid: time `reps` launches of the two read kernels above over in_dev [rows][stride]
// (nsamples valid floats per row; 16-byte aligned, stride and nsamples multiples of 256) with HIP
// events on the context's stream.  ms[0]: average of the linear read of rows * stride floats,
// ms[1]: average of the row-pattern read of rows * nsamples floats.
int earhip_debug_read_bandwidth(earhip_ctx *ctx, const float *in_dev, size_t rows, size_t stride,
                                size_t nsamples, int reps, double ms[2]) {
  return guarded([&] {
    require(ctx != nullptr && in_dev != nullptr && ms != nullptr, "NULL argument");
    require(rows >= 1 && rows < ((size_t)1 << 24) && reps >= 1 && reps <= 1000, "rows / reps out of range");
    require(stride % 256 == 0 && nsamples % 256 == 0 && nsamples >= 256 && nsamples <= stride &&
                ((uintptr_t)in_dev & 15) == 0,
            "buffer must be 16-byte aligned with stride and nsamples multiples of 256");
    ctx->use();
    if (!ctx->level.p) ctx->level.alloc_zero(4, ctx->stream);
    float *sink = reinterpret_cast<float *>(ctx->level.p);  // never written (the kernels' condition is never true)
    hipEvent_t e[4];
    for (auto &x : e) EARHIP_HIP(hipEventCreate(&x));
    const size_t n4 = rows * stride / 4;
    const unsigned lin_blocks = (unsigned)std::min<size_t>((n4 + 255) / 256, (size_t)ctx->num_cus * 32);
    auto linear = [&] {
      hipLaunchKernelGGL(k_read_linear, dim3(lin_blocks), dim3(256), 0, ctx->stream,
                         reinterpret_cast<const f32x4 *>(in_dev), sink, n4);
    };
    auto pattern = [&] {
      hipLaunchKernelGGL(k_read_rows, dim3((unsigned)(nsamples / 256)), dim3(256), 0, ctx->stream, in_dev, sink,
                         (int)rows, stride);
    };
    linear();  // (warm-up launch of each kernel outside its interval)
    EARHIP_HIP(hipEventRecord(e[0], ctx->stream));
    for (int i = 0; i < reps; i++) linear();
    EARHIP_HIP(hipEventRecord(e[1], ctx->stream));
    pattern();
    EARHIP_HIP(hipEventRecord(e[2], ctx->stream));
    for (int i = 0; i < reps; i++) pattern();
    EARHIP_HIP(hipEventRecord(e[3], ctx->stream));
    EARHIP_HIP(hipGetLastError());
    EARHIP_HIP(hipEventSynchronize(e[3]));
    float t = 0.0f;
    EARHIP_HIP(hipEventElapsedTime(&t, e[0], e[1]));
    ms[0] = (double)t / reps;
    EARHIP_HIP(hipEventElapsedTime(&t, e[2], e[3]));
    ms[1] = (double)t / reps;
    for (auto &x : e) (void)hipEventDestroy(x);
  });
}

int earhip_debug_copy_bandwidth(earhip_ctx *ctx, void *host, size_t bytes, int reps, double ms[2]) {
  return guarded([&] {
    require(ctx != nullptr && host != nullptr && ms != nullptr, "NULL argument");
    require(bytes >= 4 && reps >= 1 && reps <= 1000, "bytes / reps out of range");
    ctx->use();
    DevBuf<char> dev;
    dev.alloc(bytes);
    hipEvent_t e[2];
    for (auto &x : e) EARHIP_HIP(hipEventCreate(&x));
    for (int dir = 0; dir < 2; dir++) {
      auto copy = [&] {
        if (dir == 0) EARHIP_HIP(hipMemcpyAsync(dev.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
        else EARHIP_HIP(hipMemcpyAsync(host, dev.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
      };
      copy();  // (warm-up outside the interval)
      EARHIP_HIP(hipEventRecord(e[0], ctx->stream));
      for (int i = 0; i < reps; i++) copy();
      EARHIP_HIP(hipEventRecord(e[1], ctx->stream));
      EARHIP_HIP(hipEventSynchronize(e[1]));
      float t = 0.0f;
      EARHIP_HIP(hipEventElapsedTime(&t, e[0], e[1]));
      ms[dir] = (double)t / reps;
    }
    for (auto &x : e) (void)hipEventDestroy(x);
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
  });
}

/* diagnostic builds (-DEARHIP_HG_PROF) only: the phase sums every wave of two workgroups of the LAST hinge-kernel launch left
 * (gain_hg.h), out[2][8][8]; an ordinary build reports "not built in" */
int earhip_debug_hg_prof(earhip_ctx *ctx, unsigned long long *out128) {
  return guarded([&] {
    require(ctx != nullptr && out128 != nullptr, "NULL argument");
#ifdef EARHIP_HG_PROF
    ctx->use();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    EARHIP_HIP(hipMemcpyFromSymbol(out128, HIP_SYMBOL(g_hg_prof), sizeof(unsigned long long) * 128));
#else
    fail_invalid("this build has no hinge-kernel phase sums (-DEARHIP_HG_PROF)");
#endif
  });
}

/* diagnostic builds (-DEARHIP_BUILD_PROF) only: the s_memtime stamps thread 0 of two workgroups of the LAST list-builder launch
 * (k_piece_build or k_hinge_build) left at its phase boundaries, out[2][32]; an ordinary build reports "not built in" */
int earhip_debug_build_prof(earhip_ctx *ctx, unsigned long long *out64) {
  return guarded([&] {
    require(ctx != nullptr && out64 != nullptr, "NULL argument");
#ifdef EARHIP_BUILD_PROF
    ctx->use();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    EARHIP_HIP(hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_build_prof), sizeof(unsigned long long) * 64));
#else
    fail_invalid("this build has no list-builder phase stamps (-DEARHIP_BUILD_PROF)");
#endif
  });
}

// Tuning aid: enqueue a probe that samples the shader-cycle and the constant-rate
// counters into device memory `out_dev[2]` (two probes bracket a region to get
// the average shader clock).  wall_clock64 rate: hipDeviceAttributeWallClockRate.
int earhip_debug_clock_probe(earhip_ctx *ctx, void *out_dev) {
  return guarded([&] {
    require(ctx != nullptr && out_dev != nullptr, "NULL argument");
    ctx->use();
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(1), 0, ctx->stream,
                       (unsigned long long *)out_dev);
    EARHIP_HIP(hipGetLastError());
  });
}

int earhip_version(void) { return EARHIP_VERSION; }
const char *earhip_last_error(void) { return g_last_error.c_str(); }

int earhip_device_count(int *count) {
  return guarded([&] {
    require(count != nullptr, "count must not be NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
  });
}

int earhip_ctx_create(int device, void *hip_stream, earhip_ctx **out) {
  return guarded([&] {
    require(out != nullptr, "out must not be NULL");
    int n = 0;
    EARHIP_HIP(hipGetDeviceCount(&n));
    if (n <= 0)
      throw Error{EARHIP_DEVICE_ERROR,
                  "internal error: no HIP device available (libearhip has no CPU fallback)"};
    require(device >= 0 && device < n, "device index out of range");
    // (an owned stream goes with the context whichever way this function is left)
    struct CtxDelete {
      void operator()(earhip_ctx *c) const {
        if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
        delete c;
      }
    };
    std::unique_ptr<earhip_ctx, CtxDelete> c(new earhip_ctx);
    c->device = device;
    EARHIP_HIP(hipSetDevice(device));
    // the options: once, from the environment (EARHIP_<KEY>); afterwards only earhip_ctx_set_option changes them
    for (int o = 0; o < OPT_COUNT; o++) {
      const std::string name = std::string("EARHIP_") + kOptNames[o];
      if (const char *e = getenv(name.c_str())) c->opt[o].set = true, c->opt[o].v = parse_option_value(name, e);
    }
    if (hip_stream) {
      c->stream = (hipStream_t)hip_stream;
    } else {
      EARHIP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
      c->own_stream = true;
    }
    hipDeviceProp_t prop;
    EARHIP_HIP(hipGetDeviceProperties(&prop, device));
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->hinge_build_lds = hinge_build_allow_lds(prop);  // (this device's limit)
    c->apply_options();
    *out = c.release();
  });
}

int earhip_ctx_set_option(earhip_ctx *ctx, const char *key, const char *value) {
  return guarded([&] {
    require(ctx != nullptr && key != nullptr, "NULL argument");
    std::string k(key);
    for (auto &ch : k) ch = (char)std::toupper((unsigned char)ch);
    if (k.compare(0, 7, "EARHIP_") == 0) k = k.substr(7);
    for (int o = 0; o < OPT_COUNT; o++)
      if (k == kOptNames[o]) {
        const bool set = value != nullptr && value[0] != 0;
        const int v = set ? parse_option_value(k, value) : 0;  // (refused before anything changes)
        ctx->opt[o].set = set;
        ctx->opt[o].v = v;
        ctx->apply_options();
        return;
      }
    fail_invalid("unknown option '" + std::string(key) + "'");
  });
}

int earhip_ctx_get_option(const earhip_ctx *ctx, const char *key, int *is_set, int *value) {
  return guarded([&] {
    require(ctx != nullptr && key != nullptr && is_set != nullptr && value != nullptr, "NULL argument");
    std::string k(key);
    for (auto &ch : k) ch = (char)std::toupper((unsigned char)ch);
    if (k.compare(0, 7, "EARHIP_") == 0) k = k.substr(7);
    for (int o = 0; o < OPT_COUNT; o++)
      if (k == kOptNames[o]) {
        *is_set = ctx->opt[o].set ? 1 : 0;
        *value = ctx->opt[o].v;
        return;
      }
    fail_invalid("unknown option '" + std::string(key) + "'");
  });
}

int earhip_ctx_destroy(earhip_ctx *ctx) {
  return guarded([&] {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    {
      std::lock_guard<std::mutex> lock(g_policy_mutex);
      for (size_t i = 0; i < g_policy.size(); i++)
        if (g_policy[i].first == ctx) {
          g_policy.erase(g_policy.begin() + i);
          break;
        }
    }
    for (earhip_vbs *v : ctx->pinned_adapters) vbs_orphan(v);
    ctx->pinned_adapters.clear();
    for (const auto &r : ctx->host_ranges) {
      if (r.owned) (void)hipHostFree(const_cast<char *>(r.base));
      else (void)hipHostUnregister(const_cast<char *>(r.base));
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
  });
}

// ---- host memory the device reaches directly (include/earhip.h, group A) ------------------------------
int earhip_host_alloc(earhip_ctx *ctx, size_t bytes, void **out) {
  return guarded([&] {
    require(ctx != nullptr && out != nullptr && bytes > 0, "NULL argument or zero size");
    ctx->use();
    void *p = nullptr;
    EARHIP_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    ctx->host_ranges.push_back({static_cast<const char *>(p), bytes, true});
    *out = p;
  });
}

int earhip_host_register(earhip_ctx *ctx, void *ptr, size_t bytes) {
  return guarded([&] {
    require(ctx != nullptr && ptr != nullptr && bytes > 0, "NULL argument or zero size");
    ctx->use();
    EARHIP_HIP(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    // the kernels use the host address itself: true on this platform (unified addressing), checked once here
    void *dptr = nullptr;
    if (hipHostGetDevicePointer(&dptr, ptr, 0) != hipSuccess || dptr != ptr) {
      (void)hipHostUnregister(ptr);
      fail_internal("registered host memory is not mapped at its own address on this platform");
    }
    ctx->host_ranges.push_back({static_cast<const char *>(ptr), bytes, false});
  });
}

int earhip_host_release(earhip_ctx *ctx, void *ptr) {
  return guarded([&] {
    require(ctx != nullptr, "ctx must not be NULL");
    if (!ptr) return;
    ctx->use();
    for (size_t i = 0; i < ctx->host_ranges.size(); i++)
      if (ctx->host_ranges[i].base == static_cast<const char *>(ptr)) {
        (void)hipStreamSynchronize(ctx->stream);  // a queued copy or kernel may still use the range
        const bool owned = ctx->host_ranges[i].owned;
        ctx->host_ranges.erase(ctx->host_ranges.begin() + i);
        if (owned) EARHIP_HIP(hipHostFree(ptr));
        else EARHIP_HIP(hipHostUnregister(ptr));
        return;
      }
    fail_invalid("pointer is not the start of a range of earhip_host_alloc / earhip_host_register");
  });
}

int earhip_ctx_synchronize(earhip_ctx *ctx) {
  return guarded([&] {
    require(ctx != nullptr, "ctx must not be NULL");
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
  });
}

int earhip_ctx_set_strict(earhip_ctx *ctx, int strict) {
  return guarded([&] {
    require(ctx != nullptr, "ctx must not be NULL");
    ctx->strict = strict != 0;
  });
}

static void check_policy_args(earhip_ctx *ctx, int n_in, int n_out, const float *const *in,
                              float *const *out, int64_t r0, int64_t r1) {
  require(ctx != nullptr, "ctx must not be NULL");
  require(n_in >= 1 && n_out >= 1, "n_in and n_out must be >= 1");
  require(in != nullptr && out != nullptr, "in and out must not be NULL");
  require(r0 >= 0 && r1 >= r0, "invalid sample range");
  require(r1 - r0 < (int64_t)1 << 30, "sample range too long");
}

int earhip_interp_apply_interp(earhip_ctx *ctx, int n_in, int n_out, const float *const *in,
                               float *const *out, int64_t range_start, int64_t range_end,
                               int64_t block_start, int64_t start, int64_t end,
                               const float *start_point, const float *end_point) {
  return guarded([&] {
    check_policy_args(ctx, n_in, n_out, in, out, range_start, range_end);
    require(start_point && end_point, "points must not be NULL");
    require(end > start, "interpolation curve must have end > start");
    const int64_t first = block_start + range_start - start;
    require(first > -((int64_t)1 << 30) && first + (range_end - range_start) < ((int64_t)1 << 30),
            "sample range too far from the interpolation curve");
    ctx->use();
    GainStage *st = policy_cache(ctx)->get(ctx, n_in, n_out, true);
    // a two-point curve per input channel, evaluated as ONE ramp (also outside
    // [start, end) and between equal points, like a direct call of apply_interp,
    // gain_interpolator.hpp:147-169)
    // (apply_interp ramps between equal points too, (1 - p) s + p s: the "equals the previous point" bit stays clear)
    const int64_t t[2] = {start, end};
    const uint8_t ramp_bits[2] = {0, 0};
    std::vector<float> &rows = st->rows;
    rows.resize(2 * (size_t)n_out);
    for (int m = 0; m < n_in; m++) {
      std::memcpy(rows.data(), start_point + (size_t)m * n_out, sizeof(float) * n_out);
      std::memcpy(rows.data() + n_out, end_point + (size_t)m * n_out, sizeof(float) * n_out);
      st->curves.set_object(m, 2, t, rows.data(), ramp_bits);
    }
    st->curves.commit(ctx);
    st->run_host(block_start + range_start, in, out, range_start, range_end);
  });
}

int earhip_interp_apply_constant(earhip_ctx *ctx, int n_in, int n_out, const float *const *in,
                                 float *const *out, int64_t range_start, int64_t range_end,
                                 const float *point) {
  return guarded([&] {
    check_policy_args(ctx, n_in, n_out, in, out, range_start, range_end);
    require(point != nullptr, "point must not be NULL");
    ctx->use();
    GainStage *st = policy_cache(ctx)->get(ctx, n_in, n_out, false);
    const int64_t t[1] = {0};
    for (int m = 0; m < n_in; m++) st->curves.set_object(m, 1, t, point + (size_t)m * n_out);
    st->curves.commit(ctx);
    st->run_host(range_start, in, out, range_start, range_end);
  });
}

int earhip_gain_interp_create(earhip_ctx *ctx, int n_in, int n_out, earhip_gain_interp **out) {
  return guarded([&] {
    require(ctx != nullptr && out != nullptr, "ctx/out must not be NULL");
    require(n_in >= 1 && n_out >= 1, "n_in and n_out must be >= 1");
    ctx->use();
    std::unique_ptr<earhip_gain_interp> g(new earhip_gain_interp);
    g->stage.reset(new GainStage(ctx, n_in, n_out));
    *out = g.release();
  });
}

int earhip_gain_interp_destroy(earhip_gain_interp *gi) {
  return guarded([&] {
    if (!gi) return;
    (void)hipStreamSynchronize(gi->stage->ctx->stream);
    delete gi;
  });
}

int earhip_gain_interp_set_points(earhip_gain_interp *gi, int npoints, const int64_t *times,
                                  const float *values) {
  return guarded([&] {
    require(gi != nullptr, "gi must not be NULL");
    require(npoints >= 1, "interp_points must not be empty");
    require(times != nullptr && values != nullptr, "times/values must not be NULL");
    GainStage *st = gi->stage.get();
    st->ctx->use();
    // libear compares whole points (all inputs x outputs) to choose the constant
    // path (gain_interpolator.hpp:68-70,141-143)
    const size_t psz = (size_t)st->n_in * st->n_out;
    std::vector<uint8_t> flat(npoints, 0);
    for (int k = 1; k < npoints; k++) {
      bool same = true;
      for (size_t i = 0; same && i < psz; i++)
        same = values[(size_t)(k - 1) * psz + i] == values[(size_t)k * psz + i];
      flat[k] = same ? 1 : 0;
    }
    // values [npoints][n_in][n_out] -> per input channel [npoints][n_out]
    std::vector<float> rows((size_t)npoints * st->n_out);
    for (int m = 0; m < st->n_in; m++) {
      for (int k = 0; k < npoints; k++)
        std::memcpy(&rows[(size_t)k * st->n_out],
                    values + ((size_t)k * st->n_in + m) * st->n_out, sizeof(float) * st->n_out);
      st->curves.set_object(m, npoints, times, rows.data(), flat.data());
    }
    st->curves.commit(st->ctx);
  });
}

int earhip_gain_interp_process(earhip_gain_interp *gi, int64_t block_start, size_t nsamples,
                               const float *const *in, float *const *out) {
  return guarded([&] {
    require(gi != nullptr, "gi must not be NULL");
    require(in != nullptr && out != nullptr, "in and out must not be NULL");
    require(nsamples < ((size_t)1 << 30), "nsamples too large");
    gi->stage->ctx->use();
    gi->stage->run_host(block_start, in, out, 0, (int64_t)nsamples);
  });
}

int earhip_gain_interp_process_device(earhip_gain_interp *gi, int64_t block_start,
                                      size_t nsamples, const float *in_dev, size_t in_stride,
                                      float *out_dev, size_t out_stride) {
  return guarded([&] {
    require(gi != nullptr, "gi must not be NULL");
    require(in_dev != nullptr && out_dev != nullptr, "device pointers must not be NULL");
    require(nsamples < ((size_t)1 << 30), "nsamples too large");
    require(in_stride % 4 == 0 && out_stride % 4 == 0 && ((uintptr_t)in_dev & 15) == 0 &&
                ((uintptr_t)out_dev & 15) == 0,
            "device buffers must be 16-byte aligned with strides that are multiples of 4");
    if (nsamples == 0) return;
    gi->stage->ctx->use();
    gi->stage->run_device(block_start, (int)nsamples, in_dev, in_stride, out_dev, out_stride);
  });
}

}  // extern "C"
