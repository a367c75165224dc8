// api_firmix.hip — group M of include/earhip.h: a matrix of FIR filters from n_in rows to n_out rows (binaural monitoring of a
// loudspeaker bus, per-loudspeaker EQ, a filtered fold-down) on the device.  The kernels: firmix_kernels.h; the plan they share
// with the CPU tests: firmix.h.
#include <cstring>
#include <memory>

#include "common.h"
#include "firmix_kernels.h"

using namespace earhip;

namespace earhip {
std::vector<cf> make_twiddles(int L);  // api_render.hip
}

struct earhip_firmix {
  earhip_ctx *ctx = nullptr;
  FirmixPlan plan;
  int C = 0, K = 0, B = 0, P = 0, R = 0, max_blocks = 0;
  unsigned long long clock = 0;  // blocks since create / reset
  int par = 0;                   // which half of `prev` holds the block before the next call
  // everything a process call touches, made at create
  DevBuf<cf> H, X, tw;
  DevBuf<float> prev;  // [2][ring rows][B]
  DevBuf<int> rows, group_start;
  DevBuf<FirmixEntry> entries;
  DevBuf<float> d_in, d_out;  // the host form's rows: [C][max_blocks B], [K][max_blocks B]

  size_t rows_used() const { return plan.used.size(); }

  void zero() {
    EARHIP_HIP(hipMemsetAsync(prev.p, 0, sizeof(float) * prev.n, ctx->stream));
    clock = 0;
    par = 0;
  }

  void check_room(size_t nblocks) const {
    if (nblocks > (size_t)max_blocks) fail_invalid("the call would pass the FIR matrix's max_blocks (nothing was consumed)");
  }

  template <int L>
  void launch_t(int n, const float *in, size_t in_stride, float *out, size_t out_stride) {
    const int slot0 = (int)(clock % (unsigned long long)R);
    if (rows_used()) {
      FirmixSpectraArgs s;
      s.in = in, s.in_stride = in_stride;
      s.rows = rows.p;
      s.prev_in = prev.p + (size_t)par * rows_used() * (size_t)B;
      s.prev_out = prev.p + (size_t)(par ^ 1) * rows_used() * (size_t)B;
      s.X = X.p, s.tw = tw.p;
      s.n = n, s.slot0 = slot0, s.R = R;
      hipLaunchKernelGGL((k_firmix_spectra<L, false>), dim3((unsigned)n, (unsigned)rows_used()), dim3(kFirmixThreads), 0, ctx->stream, s);
    }
    FirmixMacArgs m;
    m.X = X.p, m.H = H.p, m.tw = tw.p;
    m.entries = entries.p, m.group_start = group_start.p;
    m.out = out, m.out_stride = out_stride;
    m.K = K, m.P = P, m.slot0 = slot0, m.R = R;
    m.blocks_before = clock;
    hipLaunchKernelGGL((k_firmix_mac_inverse<L>), dim3((unsigned)n, (unsigned)plan.groups()), dim3(kFirmixThreads), 0, ctx->stream, m);
    EARHIP_HIP(hipGetLastError());
    clock += (unsigned long long)n;
    par ^= 1;
  }

  template <int L>
  void spectra_of_taps_t(const float *staged) {
    FirmixSpectraArgs s;
    s.in = staged, s.in_stride = (size_t)P * (size_t)B;
    s.rows = nullptr, s.prev_in = nullptr, s.prev_out = nullptr;
    s.X = H.p, s.tw = tw.p;
    s.n = P, s.slot0 = 0, s.R = 0;
    hipLaunchKernelGGL((k_firmix_spectra<L, true>), dim3((unsigned)P, (unsigned)plan.n_pairs), dim3(kFirmixThreads), 0, ctx->stream, s);
    EARHIP_HIP(hipGetLastError());
  }

#define EARHIP_FIRMIX_SIZES(F, ...)             \
  switch (B) {                                  \
    case 64: F<128>(__VA_ARGS__); break;        \
    case 128: F<256>(__VA_ARGS__); break;       \
    case 256: F<512>(__VA_ARGS__); break;       \
    case 512: F<1024>(__VA_ARGS__); break;      \
    case 1024: F<2048>(__VA_ARGS__); break;     \
    case 2048: F<4096>(__VA_ARGS__); break;     \
    case 4096: F<8192>(__VA_ARGS__); break;     \
    default: fail_internal("FIR matrix block size without a kernel"); \
  }

  // device rows; the caller has checked the room and the strides
  void feed(size_t nblocks, const float *in, size_t in_stride, float *out, size_t out_stride) {
    EARHIP_FIRMIX_SIZES(launch_t, (int)nblocks, in, in_stride, out, out_stride)
  }
  void spectra_of_taps(const float *staged) { EARHIP_FIRMIX_SIZES(spectra_of_taps_t, staged) }
#undef EARHIP_FIRMIX_SIZES
};

namespace earhip {
void firmix_check_room(const earhip_firmix *fm, size_t nblocks) { fm->check_room(nblocks); }
void firmix_feed(earhip_firmix *fm, size_t nblocks, const float *in, size_t in_stride, float *out, size_t out_stride) {
  fm->feed(nblocks, in, in_stride, out, out_stride);
}
const earhip_ctx *firmix_ctx(const earhip_firmix *fm) { return fm->ctx; }
int firmix_inputs(const earhip_firmix *fm) { return fm->C; }
int firmix_outputs(const earhip_firmix *fm) { return fm->K; }
int firmix_block(const earhip_firmix *fm) { return fm->B; }
}  // namespace earhip

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
    fm->C = p.n_in, fm->K = p.n_out, fm->B = p.block, fm->P = p.partitions, fm->R = p.ring, fm->max_blocks = cfg->max_blocks;
    const size_t B = (size_t)p.block, PB = (size_t)p.partitions * B;
    const auto tw = make_twiddles(2 * p.block);
    fm->tw.alloc(tw.size());
    EARHIP_HIP(hipMemcpy(fm->tw.p, tw.data(), sizeof(cf) * tw.size(), hipMemcpyHostToDevice));
    fm->H.alloc(p.spectra_elems());
    fm->X.alloc(p.ring_elems());
    fm->prev.alloc(p.state_elems());
    fm->rows.alloc(p.used.size());
    fm->group_start.alloc(p.group_start.size());
    fm->entries.alloc(p.entries.size());
    if (!p.used.empty()) EARHIP_HIP(hipMemcpy(fm->rows.p, p.used.data(), sizeof(int) * p.used.size(), hipMemcpyHostToDevice));
    EARHIP_HIP(hipMemcpy(fm->group_start.p, p.group_start.data(), sizeof(int) * p.group_start.size(), hipMemcpyHostToDevice));
    if (!p.entries.empty())
      EARHIP_HIP(hipMemcpy(fm->entries.p, p.entries.data(), sizeof(FirmixEntry) * p.entries.size(), hipMemcpyHostToDevice));
    fm->d_in.alloc((size_t)p.n_in * (size_t)cfg->max_blocks * B);
    fm->d_out.alloc((size_t)p.n_out * (size_t)cfg->max_blocks * B);
    if (p.n_pairs) {  // the non-zero pairs' taps, zero-padded to whole partitions, through the forward pass
      std::vector<float> staged((size_t)p.n_pairs * PB, 0.0f);
      for (int k = 0; k < p.n_out; k++)
        for (int c : p.pairs[(size_t)k]) {
          const size_t at = (size_t)p.pair_index[(size_t)k * (size_t)p.n_in + (size_t)c];
          std::memcpy(staged.data() + at * PB, cfg->taps + ((size_t)k * (size_t)p.n_in + (size_t)c) * (size_t)p.n_taps,
                      sizeof(float) * (size_t)p.n_taps);
        }
      DevBuf<float> d_taps;
      d_taps.alloc(staged.size());
      EARHIP_HIP(hipMemcpy(d_taps.p, staged.data(), sizeof(float) * staged.size(), hipMemcpyHostToDevice));
      fm->spectra_of_taps(d_taps.p);
      EARHIP_HIP(hipStreamSynchronize(ctx->stream));  // (d_taps goes away)
    }
    fm->zero();
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
    *out = fm.release();
  });
}

int earhip_firmix_destroy(earhip_firmix *fm) {
  return guarded([&] {
    if (!fm) return;
    (void)hipSetDevice(fm->ctx->device);
    (void)hipStreamSynchronize(fm->ctx->stream);
    delete fm;
  });
}

int earhip_firmix_reset(earhip_firmix *fm) {
  return guarded([&] {
    require(fm != nullptr, "matrix must not be NULL");
    fm->ctx->use();
    fm->zero();
  });
}

int earhip_firmix_info(const earhip_firmix *fm, int info[5]) {
  return guarded([&] {
    require(fm != nullptr && info != nullptr, "matrix and info must not be NULL");
    info[0] = fm->C, info[1] = fm->K, info[2] = fm->B, info[3] = fm->P, info[4] = fm->plan.n_pairs;
  });
}

int earhip_firmix_process_device(earhip_firmix *fm, size_t nblocks, const float *in_dev, size_t in_stride, float *out_dev,
                                 size_t out_stride) {
  return guarded([&] {
    require(fm != nullptr, "matrix must not be NULL");
    fm->check_room(nblocks);
    if (nblocks == 0) return;
    require(in_dev != nullptr && out_dev != nullptr, "device pointers must not be NULL");
    require(in_stride >= nblocks * (size_t)fm->B && out_stride >= nblocks * (size_t)fm->B, "stride too small");
    fm->ctx->use();
    fm->feed(nblocks, in_dev, in_stride, out_dev, out_stride);
  });
}

int earhip_firmix_process(earhip_firmix *fm, size_t nblocks, const float *const *in, float *const *out) {
  return guarded([&] {
    require(fm != nullptr, "matrix must not be NULL");
    fm->check_room(nblocks);
    if (nblocks == 0) return;
    require(in != nullptr && out != nullptr, "in and out must not be NULL");
    for (int c : fm->plan.used) require(in[c] != nullptr, "a row pointer of a channel that is read is NULL");
    for (int k = 0; k < fm->K; k++) require(out[k] != nullptr, "an output row pointer is NULL");
    earhip_ctx *ctx = fm->ctx;
    ctx->use();
    const size_t n = nblocks * (size_t)fm->B;
    for (int c : fm->plan.used)  // (a channel without a pair is not read here either)
      EARHIP_HIP(hipMemcpyAsync(fm->d_in.p + (size_t)c * n, in[c], sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
    fm->feed(nblocks, fm->d_in.p, n, fm->d_out.p, n);
    for (int k = 0; k < fm->K; k++)
      EARHIP_HIP(hipMemcpyAsync(out[k], fm->d_out.p + (size_t)k * n, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    EARHIP_HIP(hipStreamSynchronize(ctx->stream));
  });
}

}  // extern "C"
