// api_firmix.hip — group M of include/earhip.h: a matrix of FIR filters from n_in rows to n_out rows (binaural monitoring of a
// loudspeaker bus, per-loudspeaker EQ, a filtered fold-down) on the device.  The kernels: firmix_kernels.h; the plan they share
// with the CPU tests: firmix.h.
#include <cstring>
#include <memory>

#include "bus_stage.h"
#include "fft_launch.h"
#include "firmix_kernels.h"

using namespace earhip;

struct earhip_firmix : BusStage {  // (a call's unit is a block of `block` samples)
  static constexpr StageWords words = {
      "matrix must not be NULL",
      "device pointers must not be NULL", "device pointers must not be NULL",
      "stride too small", "stride too small",
      "in and out must not be NULL", "in and out must not be NULL",
      "a row pointer of a channel that is read is NULL", "an output row pointer is NULL"};
  earhip_firmix() { noun = "FIR matrix", room_name = "max_blocks"; }
  ~earhip_firmix() override {
    if (staged) (void)hipEventDestroy(staged);
  }
  FirmixPlan plan;
  int P = 0, R = 0;
  unsigned long long clock = 0;  // blocks since create / reset
  // everything a process call touches, made at create
  DevBuf<cf> H, X, tw;
  PingPong<float> prev;  // [2][ring rows][block]: the block before the next call
  DevBuf<int> rows, group_start;
  DevBuf<FirmixEntry> entries;
  HostRows host;  // [n_in][max_blocks block], [n_out][max_blocks block]
  // filter sets (earhip_firmix_create_sets; n_sets == 0: a plain matrix, none of this is used).  H, entries and group_start
  // hold n_sets slices of the full width; the steady launch points at the current set's, the fade launch at two of them.
  int n_sets = 0, J = 0;
  FirmixFade fade;
  std::vector<char> loaded;
  std::vector<int> set_pairs;
  PinBuf<float> stage;                // one set of taps [K][C][J] ...
  PinBuf<int> stage_gs;               // ... and of lists, on their way to the device
  PinBuf<FirmixEntry> stage_en;
  DevBuf<float> d_stage;              // [K C][P B]: the taps zero-padded to whole partitions (the padding is written once)
  hipEvent_t staged = nullptr;        // the copies out of the staging buffers have run

  // the handle's shape from its plan, and the host form's rows
  void shape_from_plan(int max_blocks) {
    n_in = plan.n_in, n_out = plan.n_out, block = plan.block, P = plan.partitions, R = plan.ring, room = (size_t)max_blocks;
    host.alloc((size_t)n_in * room * (size_t)block, (size_t)n_out * room * (size_t)block);
  }
  size_t rows_used() const { return plan.used.size(); }
  size_t set_spectra() const { return (size_t)n_out * (size_t)n_in * (size_t)P * (size_t)block; }
  size_t set_entries() const { return firmix_set_entries_room(n_in, n_out); }
  size_t set_groups() const { return (size_t)plan.groups() + 1; }
  const cf *H_of(int s) const { return H.p + (size_t)s * set_spectra(); }
  const FirmixEntry *entries_of(int s) const { return entries.p + (size_t)s * set_entries(); }
  const int *groups_of(int s) const { return group_start.p + (size_t)s * set_groups(); }

  void zero() override {
    prev.zero(ctx->stream);
    clock = 0;
    firmix_fade_end(fade);  // (a fade's target is current)
  }

  template <int L>
  void launch_t(int n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    const int slot0 = (int)(clock % (unsigned long long)R);
    if (rows_used()) {
      FirmixSpectraArgs s;
      s.in = in, s.in_stride = in_stride;
      s.rows = rows.p;
      s.prev_in = prev.in(), s.prev_out = prev.out();
      s.X = X.p, s.tw = tw.p;
      s.n = n, s.slot0 = slot0, s.R = R;
      hipLaunchKernelGGL((k_firmix_spectra<L, false>), dim3((unsigned)n, (unsigned)rows_used()), dim3(kFirmixThreads), 0, ctx->stream, s);
    }
    // the first blocks of a call are a fade's (select is host bookkeeping between calls), the others are steady blocks
    const int nfade = n_sets ? firmix_fade_blocks(fade.from, fade.done, fade.total, n) : 0;
    if (nfade) {
      FirmixFadeArgs f;
      f.X = X.p, f.Ha = H_of(fade.from), f.Hb = H_of(fade.current), f.tw = tw.p;
      f.ea = entries_of(fade.from), f.eb = entries_of(fade.current);
      f.ga = groups_of(fade.from), f.gb = groups_of(fade.current);
      f.out = out, f.out_stride = out_stride;
      f.K = n_out, f.P = P, f.slot0 = slot0, f.R = R;
      f.blocks_before = clock;
      f.q0 = fade.done, f.F = fade.total;
      hipLaunchKernelGGL((k_firmix_fade<L>), dim3((unsigned)nfade, (unsigned)plan.groups()), dim3(kFirmixThreads), 0, ctx->stream, f);
      firmix_fade_advance(fade, nfade);
    }
    if (n > nfade) {  // block nfade of the call is block 0 of this launch: the kernel is the plain matrix's
      FirmixMacArgs m;
      m.X = X.p, m.tw = tw.p;
      m.H = n_sets ? H_of(fade.current) : H.p;
      m.entries = n_sets ? entries_of(fade.current) : entries.p;
      m.group_start = n_sets ? groups_of(fade.current) : group_start.p;
      m.out = out + (size_t)nfade * (size_t)block, m.out_stride = out_stride;
      m.K = n_out, m.P = P, m.slot0 = firmix_ring_slot(slot0, nfade, 0, R), m.R = R;
      m.blocks_before = clock + (unsigned long long)nfade;
      hipLaunchKernelGGL((k_firmix_mac_inverse<L>), dim3((unsigned)(n - nfade), (unsigned)plan.groups()), dim3(kFirmixThreads), 0,
                         ctx->stream, m);
    }
    EARHIP_HIP(hipGetLastError());
    clock += (unsigned long long)n;
    prev.flip();
  }

  // `pairs` rows of taps [P B] -> their spectra at Hdst
  template <int L>
  void spectra_of_taps_t(const float *staged, cf *Hdst, int pairs) {
    FirmixSpectraArgs s;
    s.in = staged, s.in_stride = (size_t)P * (size_t)block;
    s.rows = nullptr, s.prev_in = nullptr, s.prev_out = nullptr;
    s.X = Hdst, s.tw = tw.p;
    s.n = P, s.slot0 = 0, s.R = 0;
    hipLaunchKernelGGL((k_firmix_spectra<L, true>), dim3((unsigned)P, (unsigned)pairs), dim3(kFirmixThreads), 0, ctx->stream, s);
    EARHIP_HIP(hipGetLastError());
  }

  // f(the transform size 2 B as a constant): the kernels exist for blocks of 64 ... 4096 samples
  template <typename F>
  void with_transform_size(F &&f) {
    fft_size_switch<128>(2 * block, f, [] { fail_internal("FIR matrix block size without a kernel"); });
  }

  void feed(size_t nblocks, const float *in, size_t in_stride, float *out, size_t out_stride) override {
    with_transform_size([&](auto L) { launch_t<decltype(L)::value>((int)nblocks, in, in_stride, out, out_stride); });
  }
  void spectra_of_taps(const float *staged, cf *Hdst, int pairs) {
    with_transform_size([&](auto L) { spectra_of_taps_t<decltype(L)::value>(staged, Hdst, pairs); });
  }

  // ---- filter sets ----
  void check_loadable(int set) const {
    require(n_sets > 0, "the matrix was not made by earhip_firmix_create_sets");
    require(set >= 0 && set < n_sets, "set index out of range");
    require(!firmix_set_in_use(fade, set), "a set that is current or being faded from cannot be loaded");
  }
  // taps [K][C][J] in memory the device reads (pinned or device): pad to whole partitions, transform into the set's slice
  void transform_set(int set, const float *taps, hipMemcpyKind kind) {
    EARHIP_HIP(hipMemcpy2DAsync(d_stage.p, sizeof(float) * (size_t)P * (size_t)block, taps, sizeof(float) * (size_t)J,
                                sizeof(float) * (size_t)J, (size_t)n_out * (size_t)n_in, kind, ctx->stream));
    spectra_of_taps(d_stage.p, H.p + (size_t)set * set_spectra(), n_out * n_in);
  }
  // the lists of a set to the device, behind every call enqueued so far; the staging buffers are free again at `staged`
  void put_lists(int set, const FirmixSetLists &l) {
    std::memcpy(stage_gs.p, l.group_start.data(), sizeof(int) * l.group_start.size());
    EARHIP_HIP(hipMemcpyAsync(group_start.p + (size_t)set * set_groups(), stage_gs.p, sizeof(int) * l.group_start.size(),
                              hipMemcpyHostToDevice, ctx->stream));
    if (!l.entries.empty()) {
      std::memcpy(stage_en.p, l.entries.data(), sizeof(FirmixEntry) * l.entries.size());
      EARHIP_HIP(hipMemcpyAsync(entries.p + (size_t)set * set_entries(), stage_en.p, sizeof(FirmixEntry) * l.entries.size(),
                                hipMemcpyHostToDevice, ctx->stream));
    }
    set_pairs[(size_t)set] = l.n_pairs;
  }
  void load_host(int set, const float *taps) {
    const size_t ntaps = (size_t)n_out * (size_t)n_in * (size_t)J;
    FirmixSetLists l = firmix_make_set_lists(n_in, n_out, J, taps);
    EARHIP_HIP(hipEventSynchronize(staged));  // an earlier load's copies have left the staging buffers
    std::memcpy(stage.p, taps, sizeof(float) * ntaps);
    transform_set(set, stage.p, hipMemcpyHostToDevice);
    put_lists(set, l);
    EARHIP_HIP(hipEventRecord(staged, ctx->stream));
    loaded[(size_t)set] = 1;
  }
  // a dense set's lists are the same for every set: they went to the device at create, and are copied there on the device
  void load_device(int set, const float *taps_dev) {
    transform_set(set, taps_dev, hipMemcpyDeviceToDevice);
    EARHIP_HIP(hipMemcpyAsync(group_start.p + (size_t)set * set_groups(), dense_gs.p, sizeof(int) * set_groups(),
                              hipMemcpyDeviceToDevice, ctx->stream));
    EARHIP_HIP(hipMemcpyAsync(entries.p + (size_t)set * set_entries(), dense_en.p, sizeof(FirmixEntry) * set_entries(),
                              hipMemcpyDeviceToDevice, ctx->stream));
    set_pairs[(size_t)set] = n_out * n_in;
    loaded[(size_t)set] = 1;
  }
  DevBuf<int> dense_gs;
  DevBuf<FirmixEntry> dense_en;
};

template <>
BusStage *earhip::as_stage<earhip_firmix>(earhip_firmix *h) {
  return h;
}

extern "C" {

int earhip_firmix_create(earhip_ctx *ctx, const earhip_firmix_config *cfg, earhip_firmix **out) {
  return guarded([&] {
    require(ctx != nullptr && cfg != nullptr && out != nullptr, "ctx, config and out must not be NULL");
    if (const char *why = firmix_check_config(cfg->n_in, cfg->n_out, cfg->block_size, cfg->n_taps, cfg->max_blocks)) fail_invalid(why);
    require(cfg->taps != nullptr, "taps must not be NULL");
    const size_t ntaps = (size_t)cfg->n_out * (size_t)cfg->n_in * (size_t)cfg->n_taps;
    require(firmix_taps_finite(cfg->taps, ntaps), "every tap must be finite");
    ctx->use();
    std::unique_ptr<earhip_firmix> fm(new earhip_firmix);
    fm->ctx = ctx;
    fm->plan = firmix_make_plan(cfg->n_in, cfg->n_out, cfg->block_size, cfg->n_taps, cfg->max_blocks, cfg->taps);
    const FirmixPlan &p = fm->plan;
    fm->shape_from_plan(cfg->max_blocks);
    const size_t PB = (size_t)p.partitions * (size_t)p.block;
    upload_twiddles(fm->tw, 2 * p.block);
    fm->H.alloc(p.spectra_elems());
    fm->X.alloc(p.ring_elems());
    fm->prev.alloc(p.state_elems() / 2);
    fm->rows.upload(p.used);
    fm->group_start.upload(p.group_start);
    fm->entries.upload(p.entries);
    if (p.n_pairs) {  // the non-zero pairs' taps, zero-padded to whole partitions, through the forward pass
      std::vector<float> staged((size_t)p.n_pairs * PB, 0.0f);
      for (int k = 0; k < p.n_out; k++)
        for (int c : p.pairs[(size_t)k]) {
          const size_t at = (size_t)p.pair_index[(size_t)k * (size_t)p.n_in + (size_t)c];
          std::memcpy(staged.data() + at * PB, cfg->taps + ((size_t)k * (size_t)p.n_in + (size_t)c) * (size_t)p.n_taps,
                      sizeof(float) * (size_t)p.n_taps);
        }
      DevBuf<float> d_taps;
      d_taps.upload(staged);
      fm->spectra_of_taps(d_taps.p, fm->H.p, p.n_pairs);
      EARHIP_HIP(hipStreamSynchronize(ctx->stream));  // (d_taps goes away)
    }
    stage_ready(fm, out);
  });
}

int earhip_firmix_create_sets(earhip_ctx *ctx, const earhip_firmix_config *cfg, int n_sets, earhip_firmix **out) {
  return guarded([&] {
    require(ctx != nullptr && cfg != nullptr && out != nullptr, "ctx, config and out must not be NULL");
    if (const char *why = firmix_check_config(cfg->n_in, cfg->n_out, cfg->block_size, cfg->n_taps, cfg->max_blocks)) fail_invalid(why);
    require(n_sets >= 1 && n_sets <= kFirmixMaxSets, "n_sets must be in [1, 4096]");
    require(cfg->taps != nullptr, "taps must not be NULL");
    const size_t ntaps = (size_t)cfg->n_out * (size_t)cfg->n_in * (size_t)cfg->n_taps;
    require(firmix_taps_finite(cfg->taps, ntaps), "every tap must be finite");
    ctx->use();
    std::unique_ptr<earhip_firmix> fm(new earhip_firmix);
    fm->ctx = ctx;
    // the plan of a dense matrix of this shape: every channel has a ring row, row = channel
    FirmixPlan &p = fm->plan;
    p.n_in = cfg->n_in, p.n_out = cfg->n_out, p.block = cfg->block_size, p.n_taps = cfg->n_taps;
    p.partitions = firmix_partitions(cfg->n_taps, cfg->block_size);
    p.ring = firmix_ring_slots(p.partitions, cfg->max_blocks);
    for (int c = 0; c < p.n_in; c++) p.used.push_back(c), p.row_of.push_back(c);
    fm->shape_from_plan(cfg->max_blocks);
    fm->n_sets = n_sets, fm->J = cfg->n_taps;
    fm->loaded.assign((size_t)n_sets, 0);
    fm->set_pairs.assign((size_t)n_sets, 0);
    const size_t B = (size_t)p.block;
    upload_twiddles(fm->tw, 2 * p.block);
    fm->H.alloc((size_t)n_sets * fm->set_spectra());
    fm->X.alloc(p.ring_elems());
    fm->prev.alloc(p.state_elems() / 2);
    fm->rows.upload(p.used);
    fm->group_start.alloc((size_t)n_sets * fm->set_groups());
    fm->entries.alloc((size_t)n_sets * fm->set_entries());
    const FirmixSetLists dense = firmix_make_set_lists(p.n_in, p.n_out, p.n_taps, nullptr);
    fm->dense_gs.upload(dense.group_start);
    fm->dense_en.upload(dense.entries);
    fm->stage.reserve(ntaps);
    fm->stage_gs.reserve(fm->set_groups());
    fm->stage_en.reserve(fm->set_entries());
    fm->d_stage.alloc_zero((size_t)p.n_out * (size_t)p.n_in * (size_t)p.partitions * B, ctx->stream);
    EARHIP_HIP(hipEventCreateWithFlags(&fm->staged, hipEventDisableTiming));
    EARHIP_HIP(hipEventRecord(fm->staged, ctx->stream));
    fm->load_host(0, cfg->taps);
    stage_ready(fm, out);
  });
}

int earhip_firmix_load_set(earhip_firmix *fm, int set, const float *taps) {
  return guarded([&] {
    require(fm != nullptr && taps != nullptr, "matrix and taps must not be NULL");
    fm->check_loadable(set);
    require(firmix_taps_finite(taps, (size_t)fm->n_out * (size_t)fm->n_in * (size_t)fm->J), "every tap must be finite");
    fm->ctx->use();
    fm->load_host(set, taps);
  });
}

int earhip_firmix_load_set_device(earhip_firmix *fm, int set, const float *taps_dev) {
  return guarded([&] {
    require(fm != nullptr && taps_dev != nullptr, "matrix and taps must not be NULL");
    fm->check_loadable(set);
    fm->ctx->use();
    fm->load_device(set, taps_dev);
  });
}

int earhip_firmix_select(earhip_firmix *fm, int set, int fade_blocks) {
  return guarded([&] {
    require(fm != nullptr, "matrix must not be NULL");
    require(fm->n_sets > 0, "the matrix was not made by earhip_firmix_create_sets");
    if (const char *why = firmix_select_check(fm->fade, fm->n_sets, fm->loaded.data(), set, fade_blocks)) fail_invalid(why);
    firmix_select_apply(fm->fade, set, fade_blocks);
  });
}

int earhip_firmix_state(const earhip_firmix *fm, int state[4]) {
  return guarded([&] {
    require(fm != nullptr && state != nullptr, "matrix and state must not be NULL");
    state[0] = fm->fade.current, state[1] = fm->fade.from, state[2] = fm->fade.done, state[3] = fm->fade.total;
  });
}

int earhip_firmix_set_info(const earhip_firmix *fm, int set, int info[2]) {
  return guarded([&] {
    require(fm != nullptr && info != nullptr, "matrix and info must not be NULL");
    require(set >= 0 && set < (fm->n_sets ? fm->n_sets : 1), "set index out of range");
    info[0] = fm->n_sets ? fm->loaded[(size_t)set] : 1;
    info[1] = fm->n_sets ? fm->set_pairs[(size_t)set] : fm->plan.n_pairs;
  });
}

int earhip_firmix_destroy(earhip_firmix *fm) { return stage_destroy(fm); }
int earhip_firmix_reset(earhip_firmix *fm) { return stage_reset(fm); }

int earhip_firmix_info(const earhip_firmix *fm, int info[5]) {
  return guarded([&] {
    require(fm != nullptr && info != nullptr, "matrix and info must not be NULL");
    info[0] = fm->n_in, info[1] = fm->n_out, info[2] = fm->block, info[3] = fm->P;
    info[4] = fm->n_sets ? fm->set_pairs[(size_t)fm->fade.current] : fm->plan.n_pairs;
  });
}

int earhip_firmix_process_device(earhip_firmix *fm, size_t nblocks, const float *in_dev, size_t in_stride, float *out_dev,
                                 size_t out_stride) {
  return guarded([&] { stage_process_device(fm, nblocks, in_dev, in_stride, out_dev, out_stride); });
}

// (a channel without a pair is not read here either: plan.row_of is -1 for it)
int earhip_firmix_process(earhip_firmix *fm, size_t nblocks, const float *const *in, float *const *out) {
  return guarded([&] { stage_process_host(fm, nblocks, in, out, [&](int c) { return fm->plan.row_of[(size_t)c] >= 0; }); });
}

}  // extern "C"
