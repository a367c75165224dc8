/* earhip.h — C ABI of the MI355X-native ADM render DSP path.
 *
 * This is the drop-in boundary: a plain-C shared library (libearhip.so) whose
 * entry points are what a binding for libear's DSP hot path would call.  Each
 * group below names the libear interface it replaces (paths relative to the
 * libear tree).  The C++14 classes in libear_amd/host/ear/dsp/ wrap these entry
 * points behind libear's own class names and signatures and map the status
 * codes back to libear's exception types.
 *
 * Conventions (libear's, include/ear/dsp/ptr_adapter.hpp:10-40):
 *   - audio is planar float32: `const float *const *in` is an array of channel
 *     pointers, each to contiguous samples;
 *   - the caller owns every buffer; the library reads/writes host pointers only
 *     during the call and never retains them;
 *   - `*_device` entry points take device pointers in the same planar layout
 *     (channel c at base + c * stride) and enqueue on the context's stream
 *     without synchronising;
 *   - no entry point allocates host or device memory in a `process` call: buffers
 *     are made at create and where curves are committed (earhip_render_commit; a
 *     process call that finds uncommitted curves commits them first).
 *
 * Errors: every function returns an int status.  Nothing throws across this
 * boundary.  earhip_last_error() returns the message of the calling thread's
 * last failure.
 */
#ifndef EARHIP_H
#define EARHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EARHIP_VERSION 100 /* 0.1.0 */

/* status codes; the C++ shim maps 1 -> ear::invalid_argument, 2,3 -> ear::internal_error,
 * 4 -> ear::not_implemented, 5 -> ear::unknown_layout, 6 -> ear::adm_error
 * (include/ear/exceptions.hpp:8-43) */
#define EARHIP_OK 0
#define EARHIP_INVALID_ARGUMENT 1
#define EARHIP_INTERNAL_ERROR 2
#define EARHIP_DEVICE_ERROR 3
#define EARHIP_NOT_IMPLEMENTED 4 /* ear::not_implemented: a case libear itself refuses */
#define EARHIP_UNKNOWN_LAYOUT 5  /* ear::unknown_layout (an invalid-argument kind: src/bs2051.cpp:19) */
#define EARHIP_ADM_ERROR 6       /* ear::adm_error: invalid ADM metadata (an invalid-argument kind) */

int earhip_version(void);
const char *earhip_last_error(void);
int earhip_device_count(int *count);

/* ------------------------------------------------------------------------
 * Context: one HIP device + one stream.  Not thread-safe (libear's stateful
 * DSP objects are single-owner as well).
 * ---------------------------------------------------------------------- */
typedef struct earhip_ctx earhip_ctx;

/* hip_stream: a hipStream_t to enqueue on (e.g. the caller's current stream),
 * or NULL to let the context create its own. */
int earhip_ctx_create(int device, void *hip_stream, earhip_ctx **out);
int earhip_ctx_destroy(earhip_ctx *ctx);
int earhip_ctx_synchronize(earhip_ctx *ctx);
/* strict != 0: gain kernels reproduce libear's float arithmetic exactly
 * (un-contracted `in * ((1-p)*s + p*e)`, inputs accumulated in channel order),
 * so M->N results are bit-identical to the CPU path.  Default 0: fused
 * multiply-adds and tree accumulation (faster, within 1e-6 relative RMS). */
int earhip_ctx_set_strict(earhip_ctx *ctx, int strict);
/* Run-time configuration (libear has none: its only knob is the FFT plugin; SURVEY 5 asks for "a small runtime config").
 * Every tuning knob is an option of the context: key = one of the names below (case-insensitive, an "EARHIP_" prefix is
 * accepted), value = a decimal integer as text, or NULL / "" to return the option to its default ("the library decides").
 * At earhip_ctx_create every option is taken ONCE from the environment variable EARHIP_<KEY>; after that only this call
 * changes it — no process call reads the environment.  An option takes effect for calls / objects made after it is
 * set.  Unknown key, or a value that is not an integer ("abc", "1x"): EARHIP_INVALID_ARGUMENT, nothing changed (a context
 * is not created from an environment that holds such a value).
 *   gain stage:   MFMA (0 VALU | 1 exact-f32 MFMA | 3 default | 4 grid kernel (curves off its grid: up to 1024 objects per workgroup,
 *                 beyond them the exact-f32 kernel) | 5 piece lists | 6 hinge kernel),
 *                 H2_TILE, P2_TILE, HG_TILE (256 | 512), P2_PAIRS, HINGE (0 | 1), H2_WGS, P2_WGS (workgroups of the launch;
 *                 P2_WGS 0: one per tile), H2_PAIR (1: the 8-wave grid kernel's plain and wide forms as a pair of launches instead of one kernel that
 *                 branches on the device's mode word: rounds 1-5), H2_RUNS (1: a workgroup of the grid kernel takes a contiguous run of tiles instead of
 *                 every n-th: measured slower, kept as a knob), HG_ROBUST (default 1: a call whose levels spread beyond the hinge
 *                 kernel's packed-f16 kink products runs that kernel's f32 form; 0: it is handed to the piece lists standing by,
 *                 rounds 4-5), BUILD_TPW, HBUILD_TPW (1 2 4 8), BUILD_2K (1: the list builders as two kernels — classify every (object,
 *                 tile) pair object-major into a staging matrix, place tile-major: the same lists bit for bit; 0: one pass; default:
 *                 two kernels for the paired piece lists only, where they are faster),
 *                 SPL (2 | 4), WAVES (1..8), TPW (1..8), NRT (4 | 8), XSCALE (log2 of a fixed input prescale), PROBE_RUNS
 *   renderer:     K2_WG, K2_OWN_BLOCK (0 | 1), RUN (odd blocks per decorrelator run), GSPLIT (1..32) — read by
 *                 earhip_render_create; TAILCUT (v = 0..7, default 2: a stream call of k rounds of tiles plus at most v / 8
 *                 of a round runs as two consecutive calls, earhip_render_last_tail_blocks; longer tails measured slower cut)
 *   host pointers: HOST_CHUNK_MB (MB of inputs per time chunk of a long earhip_render_process call: default 32 from device-reachable
 *                 rows, 16 from ordinary ones; <= 0: no pipeline, one transfer), HOST_THREADS (staging threads: default min(8, the CPUs the process may use — affinity mask, cgroup quota — less 2)),
 *                 HOST_BIND (1: the staging threads run on the NUMA node that holds the caller's rows — found with move_pages(2), the
 *                 node's CPUs from /sys; a thread remote to both the rows and the pinned staging buffer gathers at 38 GB/s where any
 *                 other placement reaches 46-48: tools/host_stream_numa.py; default 0: the scheduler's placement, 1.4 % faster
 *                 where it is good), HOST_NT (default 1: the gather writes the staging buffer with streaming stores; 0: memcpy),
 *                 HOST_FIRST (1: the first chunk of staged rows a quarter of the others; measured level, default 0)
 *   diagnostics:  BLOCK_GROUPS, DEBUG_TIMING
 * (K2_WG, K2_OWN_BLOCK, DEBUG_TIMING are "on" for any value other than 0 — rounds 1-4 read the mere presence of the environment
 * variable as "on": EARHIP_K2_WG=0 now means off.) */
int earhip_ctx_set_option(earhip_ctx *ctx, const char *key, const char *value);
int earhip_ctx_get_option(const earhip_ctx *ctx, const char *key, int *is_set, int *value);
/* Host memory the device reaches directly (pinned and mapped).  libear's interfaces take `float **` channel
 * pointers into the caller's own memory (include/ear/dsp/ptr_adapter.hpp:17-24: the columns of a matrix);
 * when those buffers come from earhip_host_alloc, or were registered once with earhip_host_register
 * (hipHostRegister: the range must stay allocated until released), AND the channel pointers of a call are
 * evenly spaced — a column-major matrix — the short-call path of earhip_render_process copies them with
 * one strided DMA instead of gathering them into a staging buffer first, and writes the outputs in place
 * (block mode: 0.12 -> 0.09 ms per 512-sample call at the headline shape); long calls (16 MB of inputs and more) move
 * their time chunks by strided DMA in both directions (0.91-0.95 of the bus's own rate, against 0.83-0.88 through the staging
 * threads).  Any other pointers work as before.  earhip_host_release frees / unregisters a range (by its start);
 * earhip_ctx_destroy the rest. */
int earhip_host_alloc(earhip_ctx *ctx, size_t bytes, void **out);
int earhip_host_register(earhip_ctx *ctx, void *ptr, size_t bytes);
int earhip_host_release(earhip_ctx *ctx, void *ptr);
/* tuning aid: enqueue a 1-thread kernel that writes {shader-cycle counter,
 * constant-rate counter} (2 x uint64) to device memory */
int earhip_debug_clock_probe(earhip_ctx *ctx, void *out_dev);
/* measurement aid (bench.py's `roofline.peak_measured`): average duration in ms, over `reps`
 * launches timed with HIP events on the context's stream, of two kernels that only READ
 * in_dev [rows][stride]: ms[0] a linear stream over rows * stride floats, ms[1] the gain stage's
 * access pattern (each workgroup a 1 KB piece of every row) over rows * nsamples floats.
 * stride and nsamples: multiples of 256, nsamples <= stride; in_dev 16-byte aligned. */
int earhip_debug_read_bandwidth(earhip_ctx *ctx, const float *in_dev, size_t rows, size_t stride,
                                size_t nsamples, int reps, double ms[2]);
/* measurement aid (bench.py's `host_stream`): what the bus gives a plain copy of `bytes` bytes between `host` (pinned or
 * pageable, the caller's) and a device buffer of the call's own — average ms over `reps` copies of ms[0] host -> device and
 * ms[1] device -> host, each between HIP events on the context's stream: the 100 % mark of the host-pointer entry points. */
int earhip_debug_copy_bandwidth(earhip_ctx *ctx, void *host, size_t bytes, int reps, double ms[2]);
/* tuning aid, diagnostic builds (-DEARHIP_K2_PROF) only: the shader-clock stamps wave 0 of two workgroups of the last decorrelator
 * launch left at its phase boundaries, out64[2][32] (tools/k2_phases.py); an ordinary build answers EARHIP_INVALID_ARGUMENT */
int earhip_debug_k2_prof(earhip_ctx *ctx, unsigned long long *out64);
/* the same for the list builders (k_piece_build / k_hinge_build; -DEARHIP_BUILD_PROF; tools/build_phases.py) */
int earhip_debug_build_prof(earhip_ctx *ctx, unsigned long long *out64);
/* the same for the hinge kernel (k_gain_mix_hg; -DEARHIP_HG_PROF; tools/hg_phases.py): per wave of two workgroups the cycles summed
 * over its chunk loop's phases, out128[2][8][8] */
int earhip_debug_hg_prof(earhip_ctx *ctx, unsigned long long *out128);

/* ------------------------------------------------------------------------
 * (A) Interpolation policies — replaces LinearInterpSingle / LinearInterpVector
 * / LinearInterpMatrix ::apply_interp and ::apply_constant
 * (include/ear/dsp/gain_interpolator.hpp:187-208, 214-241, 250-299).
 * n_in x n_out = 1x1 (Single), 1xN (Vector), MxN (Matrix).  Points are dense
 * row-major [n_in][n_out] (libear's Matrix point is vector<vector<float>>
 * indexed [in][out], gain_interpolator.hpp:247).  Writes out[o][range_start ..
 * range_end) for every output o; in and out must not alias.
 * apply_interp evaluates ONE ramp, extrapolated outside [start, end) and
 * ramping between equal points as libear's does, with libear's exact float
 * arithmetic whatever the strict setting; its samples must lie less than 2^30
 * from `start` (EARHIP_INVALID_ARGUMENT otherwise — libear has no such limit).
 * ---------------------------------------------------------------------- */
int earhip_interp_apply_interp(earhip_ctx *ctx, int n_in, int n_out,
                               const float *const *in, float *const *out,
                               int64_t range_start, int64_t range_end,
                               int64_t block_start, int64_t start, int64_t end,
                               const float *start_point, const float *end_point);
int earhip_interp_apply_constant(earhip_ctx *ctx, int n_in, int n_out,
                                 const float *const *in, float *const *out,
                                 int64_t range_start, int64_t range_end,
                                 const float *point);

/* ------------------------------------------------------------------------
 * (A') Whole-curve GainInterpolator with device-resident points — replaces
 * GainInterpolator<InterpType>::process (gain_interpolator.hpp:53-87) for
 * callers that keep the curve fixed across calls.  values: [npoints][n_in]
 * [n_out]; times must be sorted (duplicates = step).  n_in, n_out >= 1, no
 * upper bound (the gain columns are tiled as for the renderer, group F; tested
 * up to 97 outputs).
 * ---------------------------------------------------------------------- */
typedef struct earhip_gain_interp earhip_gain_interp;
int earhip_gain_interp_create(earhip_ctx *ctx, int n_in, int n_out,
                              earhip_gain_interp **out);
int earhip_gain_interp_destroy(earhip_gain_interp *gi);
int earhip_gain_interp_set_points(earhip_gain_interp *gi, int npoints,
                                  const int64_t *times, const float *values);
int earhip_gain_interp_process(earhip_gain_interp *gi, int64_t block_start,
                               size_t nsamples, const float *const *in,
                               float *const *out);
/* in_dev: [n_in][in_stride], out_dev: [n_out][out_stride], device memory */
int earhip_gain_interp_process_device(earhip_gain_interp *gi, int64_t block_start,
                                      size_t nsamples, const float *in_dev,
                                      size_t in_stride, float *out_dev,
                                      size_t out_stride);

/* ------------------------------------------------------------------------
 * (B) FFT plugin — an r2c/c2r transform with libear's FFTPlan contract
 * (include/ear/fft.hpp:27-50): forward n_fft reals -> n_fft/2+1 unpacked
 * complex bins; reverse the inverse; both un-normalised.  Like libear's kissfft
 * plan (src/fft_kiss.cpp:104-107) any even n_fft is taken — here up to 8192
 * (mixed radix 4/2/3/5 + kissfft's generic butterfly for every other prime; the
 * powers of two from 64 have their own kernels).  Cost: a prime factor p > 5 costs
 * n_fft * p complex multiply-adds per transform, as in kissfft — n_fft = 2 * 4093
 * is ~33 M of them, thousands of times a neighbouring size: correct, not fast.
 * Host pointers.
 * ---------------------------------------------------------------------- */
typedef struct earhip_fft_plan earhip_fft_plan;
int earhip_fft_plan_create(earhip_ctx *ctx, size_t n_fft, earhip_fft_plan **out);
int earhip_fft_plan_destroy(earhip_fft_plan *plan);
int earhip_fft_forward(earhip_fft_plan *plan, const float *in, float *out_complex);
int earhip_fft_reverse(earhip_fft_plan *plan, const float *in_complex, float *out);

/* ------------------------------------------------------------------------
 * (C) BlockConvolver — replaces ear::dsp::block_convolver::{Context, Filter,
 * BlockConvolver} (include/ear/dsp/block_convolver.hpp:28-112; behaviour of
 * src/dsp/block_convolver_impl.cpp:10-243).  block_size in [1, 4096], any
 * factorisation (480, 960, 1920, 441, primes ... as well as the powers of two;
 * large prime factors at the cost stated under (B)).
 *
 * libear's Context takes an FFTImpl<float> plugin by reference (block_convolver.hpp:34,
 * include/ear/fft.hpp:54-62) and runs ITS transforms.  Here the transform is part of
 * the device convolver (earhip_conv_ctx_create takes no plugin); the C++ mirror's
 * Context(size_t, FFTImpl<float>&) accepts the plugin that is this transform —
 * ear::get_fft_hip(), which ear::get_fft_kiss<float>() also returns — and REFUSES any
 * other plugin with ear::invalid_argument at construction: a caller's host FFT cannot
 * run inside a device kernel, and routing the convolver through host transforms would
 * be the CPU path this library does not have (tests/cpp/test_dropin.cpp,
 * "foreign FFTImpl is refused").  Callers with their own FFTImpl keep libear's
 * BlockConvolver for that object; results agree to the convolver tests' 1e-6.
 * ---------------------------------------------------------------------- */
typedef struct earhip_conv_ctx earhip_conv_ctx;
typedef struct earhip_conv_filter earhip_conv_filter;
typedef struct earhip_conv earhip_conv;

int earhip_conv_ctx_create(earhip_ctx *ctx, size_t block_size,
                           earhip_conv_ctx **out);
int earhip_conv_ctx_destroy(earhip_conv_ctx *cctx);
int earhip_conv_filter_create(earhip_conv_ctx *cctx, size_t n, const float *taps,
                              earhip_conv_filter **out);
/* Drops the creator's reference.  A convolver keeps its own reference for every queue slot
 * that points at the filter (libear's queue holds shared_ptrs,
 * src/dsp/block_convolver_impl.hpp:154-167), so a filter may be destroyed while it is still
 * in use or fading out; it is freed when the last slot lets go of it. */
int earhip_conv_filter_destroy(earhip_conv_filter *filter);
size_t earhip_conv_filter_num_blocks(const earhip_conv_filter *filter);
/* filter may be NULL (then num_blocks must be > 0); num_blocks 0 = take the
 * partition count from the filter (block_convolver.hpp:67-77) */
int earhip_conv_create(earhip_conv_ctx *cctx, const earhip_conv_filter *filter,
                       size_t num_blocks, earhip_conv **out);
int earhip_conv_destroy(earhip_conv *conv);
/* in may be NULL = a block of silence (block_convolver_impl.cpp:145-147,156) */
int earhip_conv_process(earhip_conv *conv, const float *in, float *out);
/* filter NULL = fade_down() / unset_filter() (src/dsp/block_convolver.cpp:27-37) */
int earhip_conv_crossfade_filter(earhip_conv *conv, const earhip_conv_filter *filter);
int earhip_conv_set_filter(earhip_conv *conv, const earhip_conv_filter *filter);

/* ------------------------------------------------------------------------
 * (D) DelayBuffer — replaces ear::dsp::DelayBuffer
 * (include/ear/dsp/delay_buffer.hpp:12-30, src/dsp/delay_buffer_impl.cpp:19-43)
 * ---------------------------------------------------------------------- */
typedef struct earhip_delay earhip_delay;
int earhip_delay_create(earhip_ctx *ctx, size_t nchannels, size_t nsamples,
                        earhip_delay **out);
int earhip_delay_destroy(earhip_delay *d);
int earhip_delay_process(earhip_delay *d, size_t nsamples, const float *const *in,
                         float *const *out);
int earhip_delay_get_delay(const earhip_delay *d);

/* ------------------------------------------------------------------------
 * (E) VariableBlockSizeAdapter — replaces ear::dsp::VariableBlockSizeAdapter
 * (include/ear/dsp/variable_block_size.hpp:17-40,
 * src/dsp/variable_block_size_impl.cpp:27-85).  Host-side FIFO re-blocking
 * around a user callback; adds block_size samples of delay.
 * ---------------------------------------------------------------------- */
typedef struct earhip_vbs earhip_vbs;
typedef int (*earhip_process_func)(const float *const *in, float *const *out,
                                   void *user); /* returns an earhip status */
int earhip_vbs_create(size_t block_size, size_t num_channels_in,
                      size_t num_channels_out, earhip_process_func process_func,
                      void *user, earhip_vbs **out);
/* the same with the adapter's two FIFO buffers in device-reachable host memory of `ctx` (earhip_host_alloc): a
 * renderer called from process_func then takes its no-staging path (the FIFO rows are evenly spaced channel
 * buffers).  Destroy the adapter before the context. */
int earhip_vbs_create_pinned(earhip_ctx *ctx, size_t block_size, size_t num_channels_in,
                             size_t num_channels_out, earhip_process_func process_func, void *user,
                             earhip_vbs **out);
int earhip_vbs_destroy(earhip_vbs *v);
int earhip_vbs_process(earhip_vbs *v, size_t nsamples, const float *const *in,
                       float *const *out);
int earhip_vbs_get_delay(const earhip_vbs *v);

/* ------------------------------------------------------------------------
 * (G) Decorrelator design (setup path, host code) — replaces designDecorrelators
 * <float> and decorrelatorCompensationDelay (include/ear/decorrelate.hpp:16-34,
 * src/decorrelate.cpp:31-97).  channel_names: the layout's channel names in
 * layout order (the filter id of a channel is the rank of its name);
 * out: [n_channels][512].
 * ---------------------------------------------------------------------- */
int earhip_decorrelator_size(void);               /* 512 */
int earhip_decorrelator_compensation_delay(void); /* 255 */
int earhip_design_decorrelator_basic(int decorrelator_id, int size, double *out);
int earhip_design_decorrelators(int n_channels, const char *const *channel_names, float *out);

/* ------------------------------------------------------------------------
 * (H) ITU-R BS.2051 loudspeaker layouts (setup path, host data) — replaces
 * ear::loadLayouts / ear::getLayout (include/ear/bs2051.hpp:8-11, src/bs2051.cpp:11-22,
 * table src/bs2051_layouts.cpp): what the render path needs of a Layout — channel
 * names in layout order (decorrelator ids), nominal positions (the gain producers) and
 * the LFE flags (zero-gain columns; Layout::withoutLfe, include/ear/layout.hpp).
 * An unknown layout name is EARHIP_UNKNOWN_LAYOUT (libear throws unknown_layout).
 * ---------------------------------------------------------------------- */
int earhip_layout_count(void);
const char *earhip_layout_name(int index); /* NULL when out of range */
int earhip_layout_num_channels(const char *layout, int *n_channels);
/* any output pointer may be NULL; *name points at static storage */
int earhip_layout_channel(const char *layout, int index, const char **name, double *azimuth,
                          double *elevation, int *is_lfe);
/* the ranges BS.2051 allows a real loudspeaker of this channel (Channel::azimuthRange / elevationRange,
 * include/ear/layout.hpp:41-42, table src/bs2051_layouts.cpp): azimuth from [0] anticlockwise to [1],
 * elevation from [0] up to [1], degrees; either pointer may be NULL */
int earhip_layout_channel_ranges(const char *layout, int index, double azimuth_range[2],
                                 double elevation_range[2]);
/* designDecorrelators<float>(getLayout(layout)) — or of getLayout(layout).withoutLfe() —
 * out: [channels kept][512] (include/ear/decorrelate.hpp:26-28) */
int earhip_design_decorrelators_for_layout(const char *layout, int without_lfe, float *out);

/* A loudspeaker layout of the caller's own — libear's Layout(name, channels) is a public constructor and its gain
 * calculators take any such layout, triangulating it with a convex hull (src/common/point_source_panner.cpp:484-487,
 * src/common/convex_hull.cpp).  Here a layout is DEFINED once under a name; from then on every function of this header
 * that takes a layout name accepts it (groups H, I, L and the decorrelator design; earhip_layout_count /
 * earhip_layout_name keep listing the BS.2051 layouts only).  Pure host code: no context, no device.  Definitions are
 * process-wide, thread-safe, never removed or changed, and at most 256.
 * earhip_layout_define: name non-empty, at most 63 characters, not a BS.2051 name; n_channels in [1, 32], of which at
 * least one and at most 22 are not LFE (the objects kernels' lock and zone tables: more is EARHIP_NOT_IMPLEMENTED).
 * Defining a name again with bit-identical content is EARHIP_OK and does nothing; with other content
 * EARHIP_INVALID_ARGUMENT.  All geometry runs here, so that a bad layout fails when it is defined and not at the first
 * create: the augmented loudspeaker set at the nominal positions (the loudspeakers that are not LFE, the extra ones
 * above / below the mid layer, the virtual bottom, the virtual top unless the layout has T+000 or UH+180), its convex
 * hull with libear's tolerance of 1e-5, and a dry run of the panner's region builder.  Three augmented vertices on a
 * line — two loudspeakers in one direction are that — is EARHIP_INVALID_ARGUMENT ("collinear points in convex hull");
 * a facet of more than 4 vertices EARHIP_INTERNAL_ERROR, as in libear; more than 16 loudspeakers around a virtual one
 * EARHIP_NOT_IMPLEMENTED (this library's limit).  A defined layout always takes the full polar panner: only the
 * BS.2051 layout 0+2+0 takes libear's stereo downmix. */
typedef struct earhip_layout_channel_def {
  const char *name;          /* non-empty, <= 31 characters, unique within the layout */
  double azimuth, elevation; /* NOMINAL position, degrees, ADM convention; finite, |elevation| <= 90, azimuth in [-180, 180] */
  int has_ranges;            /* 0: the allowed ranges are the nominal position itself */
  double azimuth_range[2], elevation_range[2]; /* as earhip_layout_channel_ranges returns them */
  int is_lfe;
} earhip_layout_channel_def;
int earhip_layout_define(const char *name, int n_channels, const earhip_layout_channel_def *channels);
/* *kind: 0 unknown, 1 an ITU-R BS.2051 layout, 2 a defined one */
int earhip_layout_kind(const char *name, int *kind);
/* The triangulation of a layout, BS.2051 (its table) or defined (its hull): the augmented vertices at their nominal
 * positions, xyz_nominal [V][3]; mix_to [V], the channel of the full layout a vertex's gain goes to (an extra
 * loudspeaker: the mid-layer one under / over it; a virtual one, which come last: -1); and the facets as
 * {n, v0 .. v(n-1)}* 0 with each facet's vertices ascending.  The counts are always written (*n_facet_ints includes the
 * closing 0); an array is written when its pointer is not NULL, and then its capacity (vertices; ints) must suffice.
 * 0+2+0 has no triangulation of its own: EARHIP_INVALID_ARGUMENT. */
int earhip_layout_hull(const char *name, int vertex_capacity, double *xyz_nominal, int *mix_to, int *n_vertices,
                       int *n_virtual, int facet_capacity, int *facets, int *n_facet_ints);

/* ------------------------------------------------------------------------
 * (I) Gain-vector producer for Objects content — replaces ear::GainCalculatorObjects
 * (include/ear/gain_calculators.hpp:45-56, src/object_based/gain_calculator_objects.cpp:24-57)
 * for point sources: the polar point-source panner (src/common/point_source_panner.cpp:
 * triplets, quads, virtual n-gons, extra height loudspeakers and their downmix, the 0+2+0
 * stereo downmix), zero gains on the LFE channels, gain, and the sqrt(1 - diffuse) /
 * sqrt(diffuse) split into the direct and diffuse vectors that feed (F).  A BATCH of
 * positions per call (one device thread each, double precision): what a renderer needs
 * per (object, metadata block).  Not implemented, as in libear's own calculate(): Cartesian
 * positions, divergence, channel lock, zone exclusion, screen scaling — of these the _objects
 * forms below carry divergence, channel lock and zone exclusion; screen scaling and screen edge
 * lock are a stage of their own in front of them (group R), Cartesian positions come in through
 * group K.
 * The _extent forms add libear's polar extent panner (src/object_based/polar_extent.cpp:
 * 12-302 with its core, polar_extent_scalar.cpp:25-108): width and height in degrees, depth in
 * distance units, each may be NULL (0); one wave per position sums the point source panner's
 * gains over 1652 points on the sphere weighted by the extent's shape (float, as in libear).
 * The float sums run in a different order from libear's scalar core: results agree to 1e-5 of
 * a gain vector's norm, the bound libear's tests put between its own cores
 * (tests/extent_tests.cpp:140-169).  With all three NULL they are the plain forms.
 * layout: an ITU-R BS.2051 name or the name of a defined layout (group H).  Positions are polar: azimuth, elevation in
 * degrees (ADM convention), distance; distance / gain / diffuse may be NULL (1, 1, 0).
 * direct, diffuse_out: [npos][n_channels] float, LFE columns zero.
 * ---------------------------------------------------------------------- */
typedef struct earhip_panner earhip_panner;
int earhip_panner_create(earhip_ctx *ctx, const char *layout, earhip_panner **out);
/* the same for loudspeakers that do not stand at their nominal positions (Channel::polarPosition,
 * include/ear/layout.hpp:32-40): azimuth / elevation in degrees, one per channel of the full layout
 * (LFE channels included, ignored); both NULL (n_channels 0): nominal.  As in libear the layer logic
 * and the triangulation follow the nominal positions and the geometry the real ones
 * (point_source_panner.cpp:256-349, :431-476); M+SC / M-SC outside 5..25 or 35..60 degrees is
 * EARHIP_INVALID_ARGUMENT, wider than 25 degrees EARHIP_NOT_IMPLEMENTED (:558-577). */
int earhip_panner_create_positions(earhip_ctx *ctx, const char *layout, int n_channels,
                                   const double *azimuth, const double *elevation,
                                   earhip_panner **out);
int earhip_panner_destroy(earhip_panner *p);
int earhip_panner_num_channels(const earhip_panner *p, int *n_channels);
/* A self-check of a panner, for set-up time (it synchronises): one device launch pans, in double, the 5200 directions
 * of the HOA design's spherical t-design plus the real direction of each loudspeaker that is not LFE.  A triangulation
 * is sound when missed == 0 (every direction lands in a region), max_power_error is rounding (0+2+0: up to 0.5, its
 * downmix is -3 dB at the back by design) and min_own_gain is 1 (a loudspeaker's own direction gives that loudspeaker).
 * Reductions run per wave, then per workgroup, then on the host in index order — no floating-point atomics: the
 * same panner gives the same report bits.  Changes nothing of the panner (earhip_panner_missed included). */
typedef struct earhip_panner_report {
  int n_directions;
  unsigned missed;
  double max_power_error; /* max |sum g^2 - 1| over the directions a region took */
  double min_own_gain;    /* min over the loudspeakers that are not LFE of their own gain at their real direction */
  int n_regions, n_triplets, n_quads, n_ngons, largest_ngon;
} earhip_panner_report;
int earhip_panner_self_check(earhip_panner *p, earhip_panner_report *report);
/* host pointers: H2D, kernel, D2H, synchronise */
int earhip_panner_calculate(earhip_panner *p, size_t npos, const double *azimuth,
                            const double *elevation, const double *distance, const double *gain,
                            const double *diffuse, float *direct, float *diffuse_out);
/* device pointers: enqueues on the context's stream, does not synchronise */
int earhip_panner_calculate_device(earhip_panner *p, size_t npos, const double *azimuth,
                                   const double *elevation, const double *distance,
                                   const double *gain, const double *diffuse, float *direct,
                                   float *diffuse_out);

int earhip_panner_calculate_extent(earhip_panner *p, size_t npos, const double *azimuth,
                                   const double *elevation, const double *distance,
                                   const double *width, const double *height, const double *depth,
                                   const double *gain, const double *diffuse, float *direct,
                                   float *diffuse_out);
int earhip_panner_calculate_extent_device(earhip_panner *p, size_t npos, const double *azimuth,
                                          const double *elevation, const double *distance,
                                          const double *width, const double *height,
                                          const double *depth, const double *gain,
                                          const double *diffuse, float *direct, float *diffuse_out);
/* The _objects forms: the _extent forms plus channelLock, polar objectDivergence and zoneExclusion
 * of an audioBlockFormat.  libear refuses the three (gain_calculator_objects.cpp:37-44); this comment
 * is their specification, after ITU-R BS.2127-0 7.3.6, 7.3.7 and 7.3.12.  Per object, in EAR's order:
 *   1. p = the Cartesian position of (azimuth, elevation, distance).
 *   2. Channel lock (channel_lock[i] non-zero).  Candidates: the non-LFE loudspeakers at the positions
 *      the panner was created with, on the unit sphere; d_c = |p - s_c|.  With a maxDistance
 *      (lock_max_distance[i]; +inf or a NULL array: none) only d_c < maxDistance + 1e-10 stay; none
 *      left: p is unchanged.  Of those with d_c < min d + 1e-10 the first in the layout's lock priority
 *      order (earhip_objects_lock_priority) wins, and p becomes its position at distance 1.
 *   3. Divergence v = divergence[i] in [0, 1] with azimuthRange r = azimuth_range[i] degrees (NULL: 45).
 *      v == 0: the one position, weight 1.  Else with (az, el, d) the polar coordinates of p (all 0 at the
 *      origin) and the axes x' = cart(az - 90, 0, 1), y' = cart(az, el, 1), z' = cart(az, el + 90, 1):
 *      p_k = q_k.x x' + q_k.y y' + q_k.z z' for q = cart(0, 0, d), cart(+r, 0, d), cart(-r, 0, d), with
 *      power weights (1 - v) / (1 + v), v / (1 + v), v / (1 + v).
 *   4. Each p_k through the polar extent panner with the object's width, height and depth: g_k.
 *   5. g = sqrt((sum_k w_k g_k^2) D), D the downmix matrix of the object's excluded set
 *      (earhip_objects_zone_downmix; excluded[i]: bit c set = channel c of the FULL layout is excluded,
 *      LFE bits are ignored; earhip_objects_excluded_channels turns zones into such a mask).
 *   6. LFE columns zero, gain, the sqrt(1 - diffuse) / sqrt(diffuse) split.
 * If no region of the layout takes one of the p_k the object's rows are zero and it counts once in
 * earhip_panner_missed (the host form: EARHIP_INTERNAL_ERROR).  Any of channel_lock,
 * lock_max_distance, divergence, azimuth_range, excluded may be NULL (0, none, 0, 45, 0).  A row whose
 * lock flag is 0, whose divergence is 0 and whose mask has no non-LFE bit takes the _extent forms'
 * kernels and has their bits.  Layouts have at most 22 loudspeakers that are not LFE (24 channels in BS.2051).
 * The host form refuses, with EARHIP_INVALID_ARGUMENT and a message that names the index: a divergence
 * outside [0, 1] or NaN, a negative or NaN maxDistance, a non-finite azimuth_range, a mask bit at or
 * beyond the layout's channel count.  The _device form cannot look at the values: it clamps a
 * divergence to [0, 1] (NaN: 0), a NaN maxDistance lets no loudspeaker qualify (the position stays),
 * mask bits beyond the layout are ignored, and a non-finite azimuth_range gives positions no region takes (zero rows, counted as missed). */
int earhip_panner_calculate_objects(earhip_panner *p, size_t npos, const double *azimuth,
                                    const double *elevation, const double *distance,
                                    const double *width, const double *height, const double *depth,
                                    const double *gain, const double *diffuse,
                                    const unsigned char *channel_lock,
                                    const double *lock_max_distance, const double *divergence,
                                    const double *azimuth_range, const uint32_t *excluded,
                                    float *direct, float *diffuse_out);
int earhip_panner_calculate_objects_device(earhip_panner *p, size_t npos, const double *azimuth,
                                           const double *elevation, const double *distance,
                                           const double *width, const double *height,
                                           const double *depth, const double *gain,
                                           const double *diffuse, const unsigned char *channel_lock,
                                           const double *lock_max_distance,
                                           const double *divergence, const double *azimuth_range,
                                           const uint32_t *excluded, float *direct,
                                           float *diffuse_out);
/* Pure host functions: no context, no device.
 * The lock priority order of a layout: the full-layout indices of its non-LFE loudspeakers, ascending
 * by (|nominal elevation|, nominal elevation, |nominal azimuth|, nominal azimuth); order: one int per
 * non-LFE loudspeaker. */
int earhip_objects_lock_priority(const char *layout, int *order);
/* an exclusion zone (PolarExclusionZone / CartesianExclusionZone of include/ear/metadata.hpp) */
typedef struct earhip_exclusion_zone {
  int cartesian; /* nonzero: the six Cartesian bounds count, else the four polar ones */
  double min_azimuth, max_azimuth, min_elevation, max_elevation;
  double min_x, max_x, min_y, max_y, min_z, max_z;
} earhip_exclusion_zone;
/* The loudspeakers the union of zones excludes, at their NOMINAL positions on the unit sphere, tol = 1e-6.
 * Polar: min_elevation - tol < el < max_elevation + tol, and |el| > 90 - tol or the azimuth in range:
 * with end' = max_azimuth moved by whole turns into [min_azimuth, min_azimuth + 360] (the two congruent:
 * min_azimuth when max_azimuth <= min_azimuth, else min_azimuth + 360, so -180 .. 180 is the full circle)
 * and x = the azimuth moved into [min_azimuth - tol, min_azimuth - tol + 360): x <= end' + tol.
 * Cartesian: min - tol < c < max + tol for each coordinate.  *mask: bits of the full layout. */
int earhip_objects_excluded_channels(const char *layout, int n_zones,
                                     const earhip_exclusion_zone *zones, uint32_t *mask);
/* The downmix matrix of an excluded set, matrix: [n_channels][n_channels] double, row i = where the signal
 * of channel i goes; LFE rows and columns are identity.  Non-LFE loudspeakers, nominal positions on the
 * unit sphere: layer 0 for el < -10, 1 for el < 10, 2 for el < 60, else 3; fb = +1, 0, -1 for y > 1e-6,
 * within 1e-6 of 0, < -1e-6.  For loudspeaker i every loudspeaker j (itself included) gets the key
 * (LP[layer_i][layer_j], |fb_i - fb_j|, llround(|s_i - s_j| 1e6), llround(|y_i - y_j| 1e6)) with
 * LP = {{0,1,2,3},{3,0,1,2},{3,2,0,1},{3,2,1,0}}; sorted by key, equal keys form a group.  An empty set
 * or one holding every non-LFE loudspeaker: identity.  Else the row of an excluded i has 1/m on the m
 * non-excluded members of the first group of i that has any.  A mask bit at or beyond the channel count
 * is EARHIP_INVALID_ARGUMENT. */
int earhip_objects_zone_downmix(const char *layout, uint32_t mask, double *matrix);

/* positions of the LAST *_device call that no region of the layout took (libear dereferences an empty
 * optional there, src/object_based/gain_calculator_objects.cpp:46; the host-pointer forms turn it into
 * EARHIP_INTERNAL_ERROR themselves): their gain rows are zero.  Synchronises the stream. */
int earhip_panner_missed(earhip_panner *p, unsigned *count);

/* (I, HOA) Decode matrix for scene-based (HOA) content — replaces ear::GainCalculatorHOA
 * (include/ear/gain_calculators.hpp:58-70, src/hoa/gain_calculator_hoa.cpp:8-72,
 * src/hoa/hoa.hpp:16-182): the AllRAD design over the layout's point source panner.  One
 * (order, degree) pair per input channel; normalization "SN3D", "N3D" or "FuMa" (an unknown
 * one is EARHIP_ADM_ERROR: libear throws adm_error); out: [n_channels][n_coef],
 * rows of LFE channels zero.  It is constant over time: feed its COLUMNS to (F) or (A')
 * as single-point gain curves (docs/dsp.rst:73-89).  screenRef and nfcRefDist are ignored
 * by libear (with a warning) and are not parameters here. */
int earhip_hoa_decode_matrix(earhip_ctx *ctx, const char *layout, int n_coef, const int *orders,
                             const int *degrees, const char *normalization, float *out);
/* with the loudspeakers' real positions (see earhip_panner_create_positions) */
int earhip_hoa_decode_matrix_positions(earhip_ctx *ctx, const char *layout, int n_channels,
                                       const double *azimuth, const double *elevation, int n_coef,
                                       const int *orders, const int *degrees,
                                       const char *normalization, float *out);

/* ------------------------------------------------------------------------
 * (I, DirectSpeakers) Gain vectors for channel-based content — replaces
 * ear::GainCalculatorDirectSpeakers (include/ear/gain_calculators.hpp:18-35,
 * src/direct_speakers/gain_calculator_direct_speakers.cpp:58-320).  Per channel, in libear's order:
 *   1. audioPackFormatID without speakerLabels: EARHIP_ADM_ERROR (:247-250); a Cartesian position:
 *      EARHIP_NOT_IMPLEMENTED (:253; group X serves it);
 *   2. LFE or not: lowPass <= 200 Hz without highPass, or a nominal label LFE1 / LFE2; the warnings
 *      FREQ_NOT_LFE and FREQ_SPEAKERLABEL_LFE_MISMATCH (:111-137);
 *   3. nominal label: the capture of ^urn:itu:bs:2051:[0-9]+:speaker:(.*)$ or the label itself, replaced
 *      by a substitution whose key is the ORIGINAL label: LFE -> LFE1, LFEL -> LFE1, LFER -> LFE2, plus
 *      the caller's, which do not override these (:80-83, :139-150);
 *   4. the first label naming a layout channel of the same LFE type gets gain 1 (:280-291);
 *   5. a screenEdgeLock is EARHIP_NOT_IMPLEMENTED from here on, as in libear (:293,
 *      src/common/screen_edge_lock.hpp:15-17; group X serves it); else the one channel of the same LFE type whose NOMINAL
 *      position lies within the position's bounds (tolerance 1e-5), or the nearest of several when it is
 *      more than 1e-5 nearer than the next (distances to the REAL positions) gets gain 1 (:152-242);
 *   6. else an LFE channel goes to LFE1 (silence without one), anything else through the layout's point
 *      source panner (group I, real positions), LFE columns zero (:304-319).
 * A BATCH of channels per call; every channel that reaches the panner goes to the device in one launch.
 *
 * NOT carried: libear's ITU-R BS.2127 mapping rules for the common-definitions packs
 * (src/direct_speakers/mapping_rules.cpp).  A channel whose audioPackFormatID has the common-definitions
 * form AP_0001xxxx (after the checks and warnings of 1-2) is EARHIP_NOT_IMPLEMENTED, the message naming
 * the pack; libear would apply a downmix rule there.  Any other pack follows 3-6, as in libear.
 *
 * layout: an ITU-R BS.2051 name or the name of a defined layout (group H); gains: [n][n_channels] float for the full layout, LFE
 * channels included.  ctx may be NULL: no device panner, and a channel that reaches step 6 as a
 * non-LFE channel is EARHIP_INVALID_ARGUMENT.  from / to: n_subst extra substitutions.
 * ---------------------------------------------------------------------- */
typedef struct earhip_direct_speakers earhip_direct_speakers;

/* one channel's DirectSpeakersTypeMetadata (include/ear/metadata.hpp:11-71).  An absent optional
 * has its has_* flag 0 (bounds default to the position's value). */
typedef struct earhip_ds_metadata {
  int n_labels;
  const char *const *labels; /* speakerLabels, in AXML order */
  int cartesian;             /* nonzero: a CartesianSpeakerPosition (refused) */
  double azimuth, elevation, distance;
  int has_azimuth_min, has_azimuth_max, has_elevation_min, has_elevation_max, has_distance_min,
      has_distance_max;
  double azimuth_min, azimuth_max, elevation_min, elevation_max, distance_min, distance_max;
  int screen_edge_lock_horizontal, screen_edge_lock_vertical; /* nonzero: set (refused, step 5) */
  int has_low_pass, has_high_pass;                            /* channelFrequency */
  double low_pass, high_pass;
  const char *audio_pack_format_id; /* NULL: none */
} earhip_ds_metadata;

int earhip_direct_speakers_create(earhip_ctx *ctx, const char *layout, int n_subst,
                                  const char *const *from, const char *const *to,
                                  earhip_direct_speakers **out);
/* loudspeakers at real positions (as earhip_panner_create_positions; distance 1): the bounds match
 * the nominal positions, the nearest candidate and the panner use the real ones */
int earhip_direct_speakers_create_positions(earhip_ctx *ctx, const char *layout, int n_channels,
                                            const double *azimuth, const double *elevation,
                                            int n_subst, const char *const *from,
                                            const char *const *to, earhip_direct_speakers **out);
int earhip_direct_speakers_destroy(earhip_direct_speakers *ds);
int earhip_direct_speakers_num_channels(const earhip_direct_speakers *ds, int *n_channels);
/* warnings_out (may be NULL): [n][2] Warning::Code values (include/ear/warnings.hpp) in the order
 * libear raises them, 0 where none.  On an error the rows up to and including the failing channel
 * hold what was raised before it; the message names the channel when n > 1. */
int earhip_direct_speakers_calculate(earhip_direct_speakers *ds, size_t n,
                                     const earhip_ds_metadata *md, float *gains,
                                     int *warnings_out);
/* the underlying point source panner's earhip_panner_missed after the last calculate (0 when
 * no channel reached it or there is no panner) */
int earhip_direct_speakers_missed(earhip_direct_speakers *ds, unsigned *count);

/* ------------------------------------------------------------------------
 * (K) Conversion of Objects metadata between polar and Cartesian — replaces ear::conversion
 * (include/ear/conversion.hpp:1-83, src/conversion.cpp:14-281): ITU-R BS.2127 section 10, the
 * mapping of positions through five azimuth sectors (mapping points 0, -30, -110, 110, 30 degrees;
 * elevations through el_top 30 / el_top_tilde 45) and of extents through the source's local
 * coordinate system, in double precision with libear's arithmetic and operation order.
 * The arrays are SoA, one per component, n elements each.  Positions are (x, y, z) or (azimuth,
 * elevation, distance) in degrees (ADM convention).  width / height / depth: the input extents
 * (degrees, degrees, distance units when polar; sizes when Cartesian), each may be NULL (0).
 * width_out / height_out / depth_out: all NULL for the point forms (pointCartToPolar,
 * pointPolarToCart), else all given (extentCartToPolar, extentPolarToCart).  An output may alias
 * the input of the SAME component (in place: azimuth over x, ..., width_out over width), so that
 * toPolar can run in place on the arrays earhip_panner_calculate_extent_device then reads.
 * Per element, as in libear:
 *   - no sector found (a NaN azimuth or coordinate): EARHIP_INTERNAL_ERROR (libear throws
 *     internal_error "could not find sector", conversion.cpp:86-92);
 *   - the sector position p outside [-1e-6, 1 + 1e-6]: EARHIP_INTERNAL_ERROR (libear's ear_assert,
 *     :143);
 *   - inputs for which libear returns NaN (Cartesian infinities, Cartesian extents whose sizes
 *     exceed 1, ...): EARHIP_OK, the NaN passed through.
 * ONE DIFFERENCE from libear: libear reduces angles with while loops that add or subtract 360
 * (src/common/geom.hpp:31-39, geom.cpp:7-28), which never end for an infinite azimuth and in
 * practice not for a huge one.  Here the reduction is an exact fmod followed by at most two
 * steps of 360: the same value wherever libear's loops end.  A polar azimuth that is infinite
 * or beyond +-2^40 degrees is EARHIP_INVALID_ARGUMENT; libear does not return at all.
 *
 * The host forms are computed on the calling thread with the same code as the device kernel,
 * need no context and no device, and are the counterparts of libear's free functions, which take
 * no device either.  They are a deliberate CPU computation, not a fall-back of a device path.  On
 * the first failing element they return its code, and earhip_last_error() names its index and
 * the reason; the elements before it are written, it and those after it are not.
 * The _device forms take device pointers (device-reachable host memory included), run one
 * thread per element on the context's stream and do not synchronise; they never compute on the
 * CPU.  status: [n] per-element codes (the host form's code of that element), may be NULL.  A
 * failed element's outputs are NaN.  n < 2^31.
 * ---------------------------------------------------------------------- */
int earhip_conversion_to_polar(size_t n, const double *x, const double *y, const double *z,
                               const double *width, const double *height, const double *depth,
                               double *azimuth, double *elevation, double *distance,
                               double *width_out, double *height_out, double *depth_out);
int earhip_conversion_to_cartesian(size_t n, const double *azimuth, const double *elevation,
                                   const double *distance, const double *width,
                                   const double *height, const double *depth, double *x, double *y,
                                   double *z, double *width_out, double *height_out,
                                   double *depth_out);
int earhip_conversion_to_polar_device(earhip_ctx *ctx, size_t n, const double *x, const double *y,
                                      const double *z, const double *width, const double *height,
                                      const double *depth, double *azimuth, double *elevation,
                                      double *distance, double *width_out, double *height_out,
                                      double *depth_out, int *status);
int earhip_conversion_to_cartesian_device(earhip_ctx *ctx, size_t n, const double *azimuth,
                                          const double *elevation, const double *distance,
                                          const double *width, const double *height,
                                          const double *depth, double *x, double *y, double *z,
                                          double *width_out, double *height_out, double *depth_out,
                                          int *status);

/* ------------------------------------------------------------------------
 * (F) Composed Objects render block — the chain libear documents but does not
 * implement (docs/dsp.rst:40-71, include/ear/gain_calculators.hpp:45-56):
 *   per object: interpolated direct and diffuse gain vectors (a
 *   GainInterpolator<LinearInterpVector> each) summed into a direct and a
 *   diffuse loudspeaker bus; diffuse bus -> one BlockConvolver per loudspeaker
 *   (decorrelator FIRs); direct bus -> DelayBuffer(delay); out = sum.
 * It has the shape of VariableBlockSizeAdapter::ProcessFunc
 * (variable_block_size.hpp:19) and processes `nblocks` consecutive blocks per
 * call ("stream mode"), which is what lets the device path approach its
 * roofline.
 * ---------------------------------------------------------------------- */
typedef struct earhip_render earhip_render;

typedef struct earhip_render_config {
  int n_objects;  /* M: input channels handled by this instance (this GPU's shard) */
  int n_out;      /* N: loudspeakers, >= 1.  No upper bound: the gain stage tiles the n_buses * N gain columns in groups
                     of 48 (24 in strict mode), as many as it takes.  Every BS.2051 layout is one group (at most 24 x 2
                     columns); every gain kernel is held to the same accuracy bars at 25, 32 (the widest layout
                     earhip_layout_define takes), 48, 49, 97 and 193 loudspeakers on two buses and 49 on one
                     (tests/test_gpu_wide_bus.py).  An attached tap brings its own limit (FIR matrix: n_in in [1, 64]) */
  int block_size; /* B in [16, 4096], any factorisation (as libear's kissfft); the tuned
                     kernels are the powers of two from 64 (512 and 1024 above all) */
  int n_buses;    /* 1: direct bus only, written straight to the output
                     2: direct + diffuse with decorrelation, delay and mix */
  /* n_buses == 2: decorrelator FIRs [n_out][n_taps] (designDecorrelators,
   * include/ear/decorrelate.hpp:26-28); FIRs longer than a block are partitioned like
   * libear's Filter (src/dsp/block_convolver_impl.cpp:16-41), up to 64 partitions */
  const float *decorrelators;
  int n_taps;
  int delay;      /* compensation delay on the direct bus in samples
                     (decorrelatorCompensationDelay() = 255); 0 = none */
  int max_blocks; /* capacity T: largest nblocks of one process call */
} earhip_render_config;

int earhip_render_create(earhip_ctx *ctx, const earhip_render_config *cfg,
                         earhip_render **out);
int earhip_render_destroy(earhip_render *r);
/* Replace one object's gain curve: times[npoints] sorted; direct and diffuse
 * [npoints][n_out] (diffuse ignored / may be NULL when n_buses == 1).  Same
 * semantics as GainInterpolator::interp_points (gain_interpolator.hpp:27-43). */
int earhip_render_set_object_points(earhip_render *r, int object, int npoints,
                                    const int64_t *times, const float *direct,
                                    const float *diffuse);
/* Upload pending curve changes now (otherwise done at the next process), and make everything a call on the new curves
 * can need: the scratch of the list kernels (sized from the curves) and, for curves the hinge kernel is planned for, its
 * kink rows — for calls of max_blocks, max_blocks / 2 and one block.  This is where the library allocates and
 * synchronises when curves outgrow what is there; a process call on committed curves does neither.  What a call keeps per
 * CONTEXT — the level and mode words of the split-operand kernels, the per-object levels of the level probe, the grid
 * kernel's per-tile words — is made by earhip_render_create for max_blocks and n_objects of that renderer.  (The counted
 * exceptions: a process call whose launch plan no commit foresaw — an option changed in between — grows the scratch itself,
 * and a call that finds one of the context's buffers smaller than it needs — none of its renderers announced that size —
 * grows that; earhip_render_scratch_regrows counts the process calls of this renderer that did either: 0 in the
 * library's own tests and benchmarks.) */
int earhip_render_commit(earhip_render *r);
int earhip_render_scratch_regrows(const earhip_render *r, long *count);
/* Zero the DSP state (convolver tails, delay line) and set the sample clock. */
int earhip_render_reset(earhip_render *r, int64_t sample_time);
/* Process nblocks blocks from device memory: in_dev [n_objects][in_stride],
 * out_dev [n_out][out_stride], nblocks*block_size samples per channel.
 * Enqueues on the context's stream; does not synchronise. */
int earhip_render_process_device(earhip_render *r, size_t nblocks,
                                 const float *in_dev, size_t in_stride,
                                 float *out_dev, size_t out_stride);
/* Same from host channel pointers — libear's own calling convention (src/dsp/variable_block_size_impl.cpp:44-81) —: H2D,
 * kernels, D2H, synchronise.  Calls of 16 MB of inputs and more run as a PIPELINE of time chunks (a few blocks each) on three
 * streams: chunk c + 1 on its way to the device while chunk c's kernels run and chunk c - 1's outputs come back; from ordinary
 * pointers persistent staging threads (started at the first such call) gather the next chunk meanwhile.  Each chunk is an
 * ordinary process call of its blocks (the DSP state carries over): the results are those of consecutive calls, and the
 * last-call queries describe the last chunk. */
int earhip_render_process(earhip_render *r, size_t nblocks, const float *const *in,
                          float *const *out);
/* Interleaved PCM frames in — the way BW64 / WAV programmes store them — converted on the DEVICE: the bus carries the
 * packed samples (2 bytes per sample for s16, 3 for s24) instead of 4-byte floats, and the caller has no deinterleave
 * or conversion pass of its own.
 *
 * frames: nblocks * block_size frames of `frame_channels` interleaved little-endian samples; a frame is
 * frame_channels * sample size bytes, no padding (s24: 3 bytes a sample, frames may start at any byte).  The renderer's
 * n_objects inputs are channels [first_channel, first_channel + n_objects) of each frame: one renderer of several
 * sharing a frame buffer (a file whose tracks feed several renderers, a rank of a multi-GPU render taking its shard).
 * Conversion to float, exactly (a caller can reproduce it bit for bit):
 *   EARHIP_PCM_S16: (float)x * 2^-15
 *   EARHIP_PCM_S24: 3 bytes, little-endian, sign-extended from bit 23: (float)x * 2^-23
 *   EARHIP_PCM_S32: (float)x rounded to nearest even, then * 2^-31
 *   EARHIP_PCM_F32: the bits as given (NaN payloads and denormals included)
 * out_interleaved == 0: out = n_out planar float rows, as earhip_render_process; != 0: out[0] is [frames][n_out]
 * interleaved float32 (one contiguous transfer back; for interleaved s16 / s24 / s32 frames out, converted on the device,
 * see earhip_render_process_frames_pcm below).
 * The result is bit-identical to earhip_render_process on the converted planar rows held in the same kind of memory
 * (pageable, or earhip_host_alloc / _register): both take their chunk plan — short call or pipeline, chunk boundaries —
 * from the same function of the FLOAT-EQUIVALENT size of the call (n_objects * frames * 4 bytes; 16 MB and more: a
 * pipeline).  A long call runs the pipeline of earhip_render_process with a time chunk = one contiguous byte range of
 * `frames`: staged into pinned memory by the staging threads (pageable frames) or copied by DMA from the caller's
 * buffer (device-reachable frames); the packed bytes go H2D, and a conversion kernel writes the chunk's planar rows
 * on the device before the chunk's render.
 * Memory, made at the first call of this form and kept (grown by a later call of wider frames): pinned staging of
 * max_blocks * block_size * frame_channels * sample size bytes (pageable frames only), the same on the device, and
 * n_out * max_blocks * block_size floats on the device for interleaved outputs; with the staging of earhip_render_process.
 * EARHIP_INVALID_ARGUMENT, with nothing written to out: an unknown format, first_channel < 0,
 * first_channel + n_objects > frame_channels, a NULL pointer (frames, out, a row of out), nblocks > max_blocks, frames
 * of s16 / s32 / f32 not aligned to the sample size.  (A device error in the middle of a long call leaves in out the
 * chunks that had come back before it, and nothing else.) */
typedef enum {
  EARHIP_PCM_S16 = 1,
  EARHIP_PCM_S24 = 2,
  EARHIP_PCM_S32 = 3,
  EARHIP_PCM_F32 = 4
} earhip_pcm_format;
int earhip_render_process_frames(earhip_render *r, size_t nblocks, const void *frames,
                                 earhip_pcm_format fmt, int frame_channels, int first_channel,
                                 float *const *out, int out_interleaved);
/* The same from device memory (device-reachable host memory included: the conversion kernel reads it where it is) to
 * device memory: out_interleaved == 0: out_dev [n_out][out_stride] (out_stride >= nblocks * block_size);
 * != 0: out_dev [frames][out_stride] (out_stride >= n_out floats between frames).  Bit-identical to
 * earhip_render_process_device on the converted rows with in_stride = nblocks * block_size.  The renderer keeps its own
 * device buffers for the converted rows (n_objects * max_blocks * block_size floats) and, for interleaved outputs, the
 * planar ones (n_out * ...), made at the first call.  The conversion reads the input from the device's memory once more
 * than float rows would be read: in HBM this form moves more bytes than earhip_render_process_device.
 * Errors as earhip_render_process_frames.  Enqueues on the context's stream; does not synchronise. */
int earhip_render_process_frames_device(earhip_render *r, size_t nblocks, const void *frames_dev,
                                        earhip_pcm_format fmt, int frame_channels, int first_channel,
                                        float *out_dev, size_t out_stride, int out_interleaved);
/* Interleaved PCM frames OUT as well: file to file in one call.  The render's float32 output samples are converted on the
 * device, so the bus carries 2 or 3 bytes per output sample too and the caller has no scale / round / saturate / pack pass;
 * on their way out the device keeps a per-channel peak and a count of clipped samples (earhip_render_output_levels).
 *
 * The conversion, exactly (a caller can reproduce it bit for bit).  x is the render's float32 output sample — the one
 * earhip_render_process_frames hands back for the same call —, every step below is ONE float32 operation rounded to
 * nearest even, and "rint" rounds to the nearest integer, ties to even:
 *   EARHIP_PCM_S16: p = x * 2^15 (exact short of overflow); v = p, or with dither v = p + d (one further float32 rounding:
 *                   the multiply and the add are NOT contracted into an fma); q = rint(v) saturated to [-32768, 32767];
 *                   stored as 2 bytes, little-endian
 *   EARHIP_PCM_S24: q = rint(x * 2^23) saturated to [-2^23, 2^23 - 1]; 3 bytes, little-endian, no padding
 *   EARHIP_PCM_S32: q = rint(x * 2^31); x * 2^31 >= 2^31 gives 2147483647, < -2^31 gives -2147483648 (compared in float
 *                   before any integer conversion: 2^31 does not fit); 4 bytes, little-endian
 *   EARHIP_PCM_F32: the bits of x (what out_interleaved != 0 of earhip_render_process_frames gives); 4 bytes
 * NaN is stored as 0 and counts as a clipped sample; +-inf saturates and counts as clipped.  A sample is CLIPPED when
 * saturation changed it (the rounded value lay outside the format's range: 1.0 -> 32767 is clipped, -1.0 -> -32768 is not)
 * or it was NaN.  F32 output never clips.
 * Dither (earhip_pcm_out.dither = 1): TPDF over (-1, 1) LSB, for EARHIP_PCM_S16 only — float32 accumulation has 24
 * significant bits, dithering a 24- or 32-bit word made from it would shape nothing; with another format it is
 * EARHIP_INVALID_ARGUMENT.  d = ((h & 0xFFFF) + (h >> 16) - 65535) * 2^-16 (an exact float32), where h is a 32-bit hash
 * of (seed, sample time t, output channel n), in uint32 arithmetic (wrapping):
 *   mix(a): a ^= a >> 16; a *= 0x7FEB352D; a ^= a >> 15; a *= 0x846CA68B; a ^= a >> 16
 *   h = mix(mix(mix(mix(t_lo + 0x9E3779B9) ^ t_hi) + n * 0x85EBCA6B) ^ seed)
 * t_lo / t_hi: the low and high 32 bits of t as a 64-bit two's complement number.  t is the renderer's own sample clock
 * (earhip_render_reset sets it; each call advances it by its frames), not an index into the call: the dither of a sample does
 * not depend on how the stream is cut into calls, on the pipeline's chunks or on the kernel that rendered it, and a second
 * renderer with another seed (another rank, another layout) is uncorrelated.  Off by default (a zeroed earhip_pcm_out
 * but for its format).
 *
 * out_frames: nblocks * block_size frames of exactly n_out samples of out->format, no padding.  The host form takes its chunk
 * plan from the same function of the float-equivalent INPUT size as earhip_render_process_frames, so the float samples that
 * reach the converter are bit-identical to those that call returns for frames and outputs in the same kind of memory.  In a
 * long call chunk c is converted on the context's stream behind its render, and its packed bytes go back on the third stream
 * while chunk c + 1 renders: into out_frames directly when it is device-reachable (earhip_host_alloc / _register), else
 * through pinned staging and a host memcpy of a contiguous byte range.
 * Memory, made at the first call of this form and kept (grown by a later call of a wider format): max_blocks * block_size *
 * n_out * sample size bytes on the device, and as many pinned at the first call whose out_frames is pageable (a renderer that
 * only ever writes into device-reachable frames has no pinned staging); 768 * n_out bytes of levels (64 copies, so that the waves of a launch do not meet on n_out addresses).
 * EARHIP_INVALID_ARGUMENT, nothing written: everything earhip_render_process_frames refuses, a NULL out / out_frames, an
 * unknown out->format, dither other than 0 / 1 or with a format other than S16, out_frames (out_dev) of s16 / s32 / f32 not
 * aligned to the sample size (s24 may start at any byte); in the device form out_frame_bytes < out_first_byte + n_out *
 * sample size, or out_first_byte / out_frame_bytes not a multiple of the sample size for s16 / s32 / f32.
 * Out of scope: PCM out from planar float rows (earhip_render_process: libear's callers there want floats), noise-shaped
 * dither, big-endian or padded (s24 in 4 bytes) containers, and any file I/O. */
typedef struct earhip_pcm_out {
  earhip_pcm_format format; /* EARHIP_PCM_S16 | _S24 | _S32 | _F32 */
  int dither;               /* 0 | 1 (S16 only) */
  uint32_t seed;            /* of the dither hash */
} earhip_pcm_out;
int earhip_render_process_frames_pcm(earhip_render *r, size_t nblocks, const void *frames,
                                     earhip_pcm_format fmt, int frame_channels, int first_channel,
                                     void *out_frames, const earhip_pcm_out *out);
/* Device memory to device memory.  out_frame_bytes is the distance between output frames; the renderer's samples are bytes
 * [out_first_byte, out_first_byte + n_out * sample size) of each, and every other byte of out_dev is left as it was — never
 * written, never read and written back —, so several renderers may fill their channels of the same frames at the same time.
 * Bit-identical to the conversion above of what earhip_render_process_frames_device gives.  Enqueues on the context's stream;
 * does not synchronise (but for the first call of this form, which makes the renderer's buffers). */
int earhip_render_process_frames_pcm_device(earhip_render *r, size_t nblocks, const void *frames_dev,
                                            earhip_pcm_format fmt, int frame_channels,
                                            int first_channel, void *out_dev, size_t out_frame_bytes,
                                            size_t out_first_byte, const earhip_pcm_out *out);
/* Per output channel, since these numbers were last zeroed: peak[n_out] = the largest |x| that went through a PCM-out call
 * (the float32 render sample, before scaling and dither; NaN ignored, so +inf is possible), clipped[n_out] = the number of
 * clipped samples.  Synchronises the stream.  reset != 0: zero them afterwards.  earhip_render_reset zeroes them too.  The
 * float calls (earhip_render_process*, _process_frames) neither read nor change them. */
int earhip_render_output_levels(earhip_render *r, float *peak, uint64_t *clipped, int reset);
/* Kernel timing (HIP events on the context's stream around each launch).
 * enable != 0 starts collecting and zeroes the counters; enable = n > 1 times
 * every n-th process call only, starting with the next one (each timed call
 * records six events, which costs the GPU about 20 us of idle time). */
int earhip_render_enable_timing(earhip_render *r, int enable);
/* Sums since enable: [0] gain_mix kernel ms, [1] its launches, [2] decorrelate/
 * delay/mix kernel ms, [3] its launches, [4] segment-prep kernel ms, [5] its
 * launches.  Synchronises the stream. */
int earhip_render_get_timing(earhip_render *r, double out[6]);
/* Which gain kernel the last process call used: 0 = VALU with libear's exact
 * arithmetic (strict mode), 1 = f32 MFMA over slot lists, 2 = f32 MFMA on the tile grid (option
 * MFMA = 1 with every curve point on the 512-sample grid of a call of whole tiles), 3 = f16x2-split MFMA (all
 * curve points on the kernel's tile boundaries), 4 = f16x2-split MFMA over piece lists
 * (metadata that ignores the tile grid), 5 = f16x2-split MFMA with hinges (curves that ramp
 * all the time off the tile grid; the piece lists stand by: see below); -1 before the first
 * call. */
int earhip_render_gain_kernel(const earhip_render *r, int *kind);
/* Kernel 5 keeps 1e-6 for inputs down to 16 binades below the call's level (kernel 4: 21), so a
 * call it is planned for is decided ON THE DEVICE, from the level probe of the call's inputs: the
 * hinge kernel or the piece lists launched behind it.  *standby = 1 when the last call of this
 * renderer was planned for kernel 5 and the piece lists did it, else 0.  Synchronises the stream
 * (for benchmarks and tests that must name the kernel they measured).  The kernel that does a call
 * leaves a copy of the context's decision word in the renderer's own device slot: the answer stays
 * valid until the next process call of THIS renderer, whatever other renderers or gain stages of the
 * context do in between. */
int earhip_render_hinge_standby(earhip_render *r, int *standby);
/* Round 6: by default such a call is no longer handed over — kernel 5 has a third form of its body whose kink products are made
 * in f32 (7 instructions per value instead of 3; inputs 21 binades below the call's level keep ~17 bits of their products),
 * picked by the same device-side word; earhip_render_hinge_standby then answers 0 and *robust = 1 tells that the last call
 * of this renderer ran that form (0: the packed-f16 products sufficed, or the call was not kernel 5's).  Option HG_ROBUST = 0
 * restores the hand-over to the piece lists.  Synchronises the stream; valid until this renderer's next process call. */
int earhip_render_hinge_robust(earhip_render *r, int *robust);
/* The split-operand kernels (3, 4, 5) have two forms of their body: plain, and wide (the low pieces of the inputs scaled so
 * that they stay normal f16 numbers 21 binades below the call's level instead of 11).  Long calls (two rounds of workgroups
 * and more) pick on the device, from the level probe; shorter ones run the wide form.  *wide = 1 / 0: the form the last call
 * of this renderer ran (-1: its kernel has no split operands).  Synchronises the stream; valid until the next process call
 * of this renderer, like earhip_render_hinge_standby.  After a call that ran as two spans (earhip_render_last_tail_blocks
 * > 0) both queries — like earhip_render_gain_kernel and earhip_render_last_plan — describe the MAIN span (the whole
 * rounds of tiles: where the call's time goes); the short tail behind it runs the wide form without a hand-over. */
int earhip_render_wide_form(earhip_render *r, int *wide);
/* The launch plan of the last process call: [0] gain kernel (as above), [1] samples per
 * workgroup tile of the gain kernel, [2] number of such tiles, [3] grid-level object splits.
 * For tests and benchmarks that must know which kernel instantiation they measured. */
int earhip_render_last_plan(const earhip_render *r, int out[4]);
/* The decorrelator stage's plan: [0] the partition size of the decorrelator FIRs in samples (the block size, or 512 for
 * blocks of 1024, 2048, 4096 whose FIRs fit 512 taps: option K2_OWN_BLOCK), [1] the number of partitions (ceil(n_taps /
 * [0]): one launch each per call), and of the last process call (of its last span, where it ran as two:
 * earhip_render_last_tail_blocks) [2] the kernel form — 0 the workgroup kernel instantiated for the transform size (powers
 * of two from 128), 1 the workgroup kernel with the transform's shape taken at run time (every other size), 2 the wave
 * kernel (512-sample partitions, one partition; option K2_WG) — and [3] the blocks (partitions) per run of that kernel
 * (option RUN; 0: no call yet).  All zeros for a renderer of one bus, which has no decorrelator stage.  For tests that
 * must know which form of the stage they checked. */
int earhip_render_last_decor_plan(const earhip_render *r, int out[4]);
/* Layout of the piece lists of the last call (kernel 4, or the lists standing by behind kernel 5): *paired = 1 paired
 * (an object's base and delta piece share one input request; curves that hold most of the time), 0 packed (every chunk
 * sums its products among itself before it touches the running total: curves that ramp most of the time ALWAYS get this
 * one, whatever their other statistics — the planner's rule, asserted by the tests), -1: the call built no piece lists. */
int earhip_render_last_list_layout(const earhip_render *r, int *paired);
/* A stream call whose tiles are whole rounds of the chip's workgroups plus a few (1025 blocks of 512 samples on 256 CUs)
 * is run as two consecutive calls — the whole rounds, then the few blocks behind them spread over the chip by object
 * splits — instead of paying a whole round for the few.  *blocks = the blocks of the last call that ran as such a tail
 * (0: the call was not cut).  Results are those of the two calls made by the caller. */
int earhip_render_last_tail_blocks(const earhip_render *r, int *blocks);
/* earhip_render_process from host channel pointers (libear's calling convention, variable_block_size_impl.cpp:44-81) runs a long
 * call — 16 MB of inputs and more — as a pipeline of time chunks on three streams (transfer in / kernels / transfer out; options
 * HOST_CHUNK_MB, HOST_THREADS, HOST_BIND).  *chunks = the chunks the last such call of this renderer ran as (0: one piece). */
int earhip_render_last_host_chunks(const earhip_render *r, int *chunks);
/* Bytes of device scratch (segment descriptors, slot / piece / hinge lists) the last process call needed: sized per call
 * from its launch plan and the curves (the piece lists from the most ramps any window of a tile's length overlaps, per
 * object), not for the worst case. */
int earhip_render_scratch_bytes(const earhip_render *r, size_t *bytes);

/* ------------------------------------------------------------------------
 * (J) Multi-GPU exchange — no libear counterpart (libear is single-device).  Objects are
 * sharded over the GPUs of one node, one process and one earhip_ctx per GPU; every rank
 * renders its shard completely with (F) — everything after the buses is linear and per
 * channel — and the partial outputs are summed by ONE RCCL reduce-scatter over the
 * channel axis on the context's stream (xGMI): rank r ends up owning rows
 * [r * per, (r + 1) * per) of the shared bus.
 *   earhip_comm_unique_id: rank 0 makes the 128-byte id; the caller hands it to every
 *     rank by its own means (MPI, torch.distributed, a socket, a file);
 *   earhip_comm_create: collective over all ranks (ncclCommInitRank);
 *   earhip_comm_channel_range: rows of the exchange buffers (n_out rounded up to a
 *     multiple of the ranks; the rows past n_out must be zero) and the channels [lo, hi)
 *     rank `rank` owns — ragged when the ranks do not divide n_out (10 channels on 4
 *     ranks: 3, 3, 3, 1);
 *   earhip_render_exchange_device: partial_dev [padded_rows][row_stride] ->
 *     owned_dev [rows_per_rank][row_stride].  Ordered behind everything enqueued on the
 *     context's stream so far (the render that wrote partial_dev) but run on the
 *     communicator's own stream, so that it overlaps the next render; does not
 *     synchronise the host.  slot (0 or 1) names one of two exchanges in flight
 *     (double-buffered outputs);
 *   earhip_comm_gather_device: the shared loudspeaker bus in ONE place — collects the
 *     owned slices into full_dev [padded_rows][row_stride], on every rank (root < 0: one
 *     all-gather) or on rank `root` only (the others send their slice straight to it,
 *     world - 1 transfers over world - 1 different links at once; full_dev may be NULL
 *     on the ranks that do not receive).  Runs on the communicator's stream behind the
 *     exchange of the same slot; the first n_out rows of full_dev are the bus;
 *   earhip_comm_wait(slot): work enqueued on the context's stream after this call runs
 *     after the last exchange / gather issued with that slot — call it before rendering
 *     into that slot's partial buffer again and before reading its owned / full buffer;
 *   earhip_comm_last_exchange_ms: what the collectives of a slot took on the
 *     communicator's stream (HIP events around them); waits for them.
 * ---------------------------------------------------------------------- */
typedef struct earhip_comm earhip_comm;
int earhip_comm_unique_id(void *id128);
int earhip_comm_create(earhip_ctx *ctx, int rank, int world, const void *id128, earhip_comm **out);
int earhip_comm_destroy(earhip_comm *comm);
int earhip_comm_channel_range(int n_out, int rank, int world, int *padded_rows, int *lo, int *hi);
int earhip_render_exchange_device(earhip_comm *comm, int slot, const float *partial_dev,
                                  float *owned_dev, size_t rows_per_rank, size_t row_stride);
int earhip_comm_gather_device(earhip_comm *comm, int slot, const float *owned_dev, float *full_dev,
                              size_t rows_per_rank, size_t row_stride, int root);
int earhip_comm_wait(earhip_comm *comm, int slot);
int earhip_comm_last_exchange_ms(earhip_comm *comm, int slot, double *ms);
/* What RCCL says about the communicator: info[0] ranks (ncclCommCount), [1] this rank (ncclCommUserRank), [2] the HIP device it
 * lives on (ncclCommCuDevice), [3] the RCCL version (ncclGetVersion) — a benchmark line shows with it that N ranks really met. */
int earhip_comm_info(earhip_comm *comm, int info[4]);
/* Measured rate of one link direction: every rank sends `bytes` bytes to rank + shift and receives as many from rank - shift
 * (one ncclSend / ncclRecv pair per rank, all at once: the pattern of the exchange's point-to-point steps), `reps` times between
 * HIP events on the communicator's stream.  *GBps = bytes a rank sent per second / 1e9 (0 with one rank).  Collective. */
int earhip_comm_link_probe(earhip_comm *comm, size_t bytes, int shift, int reps, double *GBps);

/* ------------------------------------------------------------------------
 * (L) Programme loudness — ITU-R BS.1770-4, no libear counterpart (libear has no meter).  The number EBU R 128 and ATSC A/85
 * are written around (LKFS), measured on the DEVICE from the render's float32 output rows while they are still in its memory:
 * no transfer of the samples, and the PCM-out forms keep their 2- or 3-byte samples on the bus.
 *
 * The measurement, exactly (a caller can reproduce it).  Per channel a cascade of two biquads in FLOAT64 arithmetic on the
 * float32 samples, y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2], state zero at create and reset.
 * BS.1770-4's coefficients at 48 kHz:
 *     stage 1 (shelf)      b0 1.53512485958697  b1 -2.69169618940638  b2 1.19839281085285  a1 -1.69065929318241  a2 0.73248077421585
 *     stage 2 (high-pass)  b0 1.0               b1 -2.0               b2 1.0               a1 -1.99004745483398  a2 0.99007225036621
 *   - STEP ENERGIES are the meter's raw product: z[s][c] = the mean of y^2 over step s of channel c; a step is 100 ms =
 *     sample_rate / 10 samples, counted on the meter's own sample clock since its reset, not per call.  The samples of an
 *     unfinished last step are kept in the state and belong to no step yet.
 *   - gating block j (400 ms, 75 % overlap) is steps j .. j + 3: P_j = sum over c of G_c (z[j][c] + .. + z[j+3][c]) / 4,
 *     l_j = -0.691 + 10 log10 P_j.
 *   - INTEGRATED loudness, gated twice: J_a = {j : l_j > -70}; Gamma_r = -0.691 + 10 log10(mean over J_a of P_j) - 10;
 *     J_g = {j in J_a : l_j > Gamma_r}; L = -0.691 + 10 log10(mean over J_g of P_j).  With fewer than 4 steps or an empty
 *     J_a, L = -infinity: a valid answer, EARHIP_OK.
 *   - MAXIMUM MOMENTARY loudness = max over j of l_j; MAXIMUM SHORT-TERM loudness = the same formula over 30 consecutive steps
 *     (3 s), hop one step.  Both -infinity when there is no whole window.
 *   - channel weights G_c of a BS.2051 layout, from the nominal positions of group H: 0 for an LFE channel, 1.41 where
 *     |elevation| < 30 and 60 <= |azimuth| <= 120 degrees, else 1.0 (0+5+0: 1 1 1 0 1.41 1.41).
 * Float64 formulations of the cascade differ among themselves by 5e-15 .. 2e-11 relative per step energy (the high-pass poles
 * lie 0.005 inside the unit circle); the device's — the time axis cut into chunks that run in parallel, the filter state carried
 * across them exactly — stays within 1e-9 of scipy.signal.lfilter in float64 (tests), float32 arithmetic would be
 * 1.6e-6 away.  Step energies are summed in a fixed order: the same calls give the same bits.
 *
 *
 * TRUE PEAK (BS.1770-4 annex 2) is measured by a meter made with earhip_loudness_create_tp, over the same samples in the same
 * calls, exactly (a caller can reproduce it):
 *   - the interpolator has `phases` FIR filters of `taps` coefficients each: y[phases n + p] = sum over k = 0 .. taps - 1 of
 *     h[p][k] x[n - k], x the float32 sample stream of one channel on the meter's own clock, zero before create and reset.
 *     The history of taps - 1 samples is carried across calls exactly: how a stream is cut into calls, launches, spans or
 *     pipeline chunks does not change a single bit of any peak.  Arithmetic is float32, the coefficients rounded once to
 *     float32, in a fixed order: an accumulator of zero, then k = 0 first, one fused multiply-add per tap;
 *   - the default table is that of annex 2, phases = 4, taps = 12, every coefficient an integer over 8192 (exact in float32):
 *         h[0] * 8192 =   14    90  -161   272   -487  1125  7964   -838   390  -218   122   -68
 *         h[1] * 8192 = -239   240  -424   730  -1364  3810  6388  -1641   832  -477   271  -155
 *         h[2][k] = h[1][11 - k]      h[3][k] = h[0][11 - k]
 *     (the interleaved 48-tap filter is symmetric; its gain is 3.95 .. 4.05 up to 20 kHz at 48 kHz and below 0.041 from 30 kHz
 *     upwards).  It is allowed at 44100 and 48000 Hz only: another rate brings its own table, e.g. 2 phases at 96 kHz;
 *   - per channel the TRUE PEAK is the largest |y| and the SAMPLE PEAK the largest |x|, both with a max that ignores NaN, as
 *     earhip_render_output_levels does (+infinity is possible), both linear float32: dBTP = 20 log10 is the caller's or the
 *     binding's job.  No 12 dB pad, no output gain;
 *   - both are kept per 100 ms step as well: y[phases n + p] belongs to the step of input sample n.  The filter's group delay
 *     (5.5 samples of the default table) is NOT compensated: a peak within that of a step's end is booked to the next step.
 *     The peaks of the unfinished step are carried to the next call, and earhip_loudness_peaks includes them.
 * A float64 evaluation of the same sums differs from this one by at most (taps + 1) 2^-24 A X_c, A the largest sum over k of
 * |h[p][k]| of any phase (2.023 for the default table), X_c the channel's sample peak.
 *
 * LOUDNESS RANGE (EBU Tech 3342) comes from the step energies on the host: the short-term powers P_j over 30 consecutive steps,
 * hop one step, l_j = -0.691 + 10 log10 P_j; the absolute gate l_j > -70; the relative gate l_j > -0.691 + 10 log10(mean of
 * P_j over the absolute-gated windows) - 20; s[0 .. n - 1] the surviving l_j sorted ascending;
 * low = s[floor((n - 1) 0.10 + 0.5)], high = s[floor((n - 1) 0.95 + 0.5)], LRA = high - low.  With no surviving window
 * LRA = 0 and low = high = -infinity: a valid answer, EARHIP_OK.
 *
 * Out of scope: K-weighting coefficients for other sample rates, any normalisation of the output gain, any file I/O.
 * ---------------------------------------------------------------------- */
typedef struct earhip_loudness earhip_loudness;
/* sample_rate: a multiple of 10.  coeffs: [2][5] = b0 b1 b2 a1 a2 per stage, or NULL = the table above, which is allowed at
 * 48000 only (another rate must bring its own coefficients).  max_steps: capacity of the step store (100 ms each), made HERE
 * with everything else the meter needs: a process call allocates nothing and synchronises nothing. */
int earhip_loudness_create(earhip_ctx *ctx, int n_channels, int sample_rate, const double *coeffs,
                           size_t max_steps, earhip_loudness **out);
/* The same meter with true peak.  tp == NULL is earhip_loudness_create exactly: such a meter runs and costs what it did.
 * tp->coeffs: [phases][taps], phases in [1, 8], taps in [1, 64], every coefficient finite (else EARHIP_INVALID_ARGUMENT), or
 * NULL = the table above (phases and taps are then ignored), which is allowed at 44100 and 48000 only.  The history, the
 * per-step peak stores [max_steps + 1][n_channels] and the table are made here: a process call still allocates nothing and
 * synchronises nothing. */
typedef struct earhip_true_peak {
  int phases;
  int taps;
  const double *coeffs;
} earhip_true_peak;
int earhip_loudness_create_tp(earhip_ctx *ctx, int n_channels, int sample_rate, const double *coeffs,
                              size_t max_steps, const earhip_true_peak *tp, earhip_loudness **out);
/* (detach it from its renderers first: earhip_render_attach_loudness(r, NULL)) */
int earhip_loudness_destroy(earhip_loudness *m);
int earhip_loudness_reset(earhip_loudness *m); /* state, clock, steps, true-peak history and peaks to zero */
/* planar float32 rows in device memory (channel c at rows_dev + c * stride), any nsamples >= 0 (no block size, no alignment);
 * enqueues on the context's stream, does not synchronise.  A call that would pass max_steps is EARHIP_INVALID_ARGUMENT and
 * consumes nothing. */
int earhip_loudness_process_device(earhip_loudness *m, size_t nsamples, const float *rows_dev, size_t stride);
/* host rows: H2D + the above, in pieces through a staging buffer of fixed size made at create; synchronises */
int earhip_loudness_process(earhip_loudness *m, size_t nsamples, const float *const *rows);
int earhip_loudness_num_steps(earhip_loudness *m, size_t *steps); /* finished steps; synchronises */
/* energy [n][n_channels] = z of steps [first, first + n), which must be finished; synchronises */
int earhip_loudness_steps(earhip_loudness *m, size_t first, size_t n, double *energy);
/* the gating above over all finished steps; weights [n_channels]; any output pointer may be NULL; synchronises */
int earhip_loudness_result(earhip_loudness *m, const double *weights, double *integrated,
                           double *max_momentary, double *max_short_term);
/* True and sample peak so far per channel [n_channels], the unfinished step included; either pointer may be NULL;
 * synchronises.  The step stores are reduced on the device (one small kernel over ten rows per second of programme) and
 * 2 x n_channels numbers come back.  EARHIP_INVALID_ARGUMENT on a meter made without true peak, as for earhip_loudness_step_peaks. */
int earhip_loudness_peaks(earhip_loudness *m, float *true_peak, float *sample_peak);
/* [n][n_channels] each, of steps [first, first + n), which must be finished; either pointer may be NULL; synchronises */
int earhip_loudness_step_peaks(earhip_loudness *m, size_t first, size_t n, float *true_peak, float *sample_peak);
/* loudness range over all finished steps (LU; low and high in LKFS); any output pointer may be NULL; synchronises */
int earhip_loudness_result_range(earhip_loudness *m, const double *weights, double *lra, double *low,
                                 double *high);
/* Pure host functions, no context and no device.  Like the host forms of group K they are a deliberate CPU computation on a
 * few numbers, not a fall-back of the device path.
 * earhip_loudness_gate is what a multi-GPU render (group J) uses: after the reduce-scatter each rank owns whole channels of
 * the summed bus (earhip_comm_channel_range) and runs a meter over its own rows; the ranks' energy columns are put side by
 * side — a channel's step energies do not depend on the other channels of its meter — and gated once. */
int earhip_loudness_gate(size_t n_steps, int n_channels, const double *energy /* [n_steps][n_channels] */,
                         const double *weights, double *integrated, double *max_momentary,
                         double *max_short_term);
/* weights [n_channels of the full layout, LFE channels included]; an unknown name is EARHIP_UNKNOWN_LAYOUT */
int earhip_loudness_layout_weights(const char *layout, double *weights);
/* loudness range of step energies, pure host like earhip_loudness_gate and joined over ranks the same way.  (Peak columns
 * of the ranks' meters join by concatenation too: a channel's peaks do not depend on the other channels of its meter.) */
int earhip_loudness_range(size_t n_steps, int n_channels, const double *energy /* [n_steps][n_channels] */,
                          const double *weights, double *lra, double *low, double *high);
/* From now on every process call of r, of EVERY form, feeds its float32 output samples to m on the device, behind its kernels
 * on the context's stream: the samples earhip_render_process_frames would hand back, before any PCM conversion or dither.
 * m == NULL detaches.  m must have n_out channels and the renderer's context (else EARHIP_INVALID_ARGUMENT).
 * earhip_render_reset does not touch m, its true-peak history and peaks included (a programme may be rendered in several
 * passes); earhip_loudness_reset does.  A call
 * that would pass m's max_steps fails with EARHIP_INVALID_ARGUMENT before anything is rendered.  A call that runs as two spans
 * or as a pipeline of chunks is metered once per sample.  Without a meter the render paths are what they were. */
int earhip_render_attach_loudness(earhip_render *r, earhip_loudness *m);

/* ------------------------------------------------------------------------
 * (M) FIR filter matrix — n_in rows to n_out rows through one FIR filter per (output, input) pair, on the device.  libear has
 * no counterpart beyond one BlockConvolver per pair (group C): with n_out = 2 and one HRIR / BRIR pair per loudspeaker this is
 * virtual-loudspeaker binaural monitoring of the render's bus while it is still in device memory; a diagonal matrix is
 * per-loudspeaker EQ / alignment; a narrow one is a filtered fold-down.  The caller brings the impulse responses.
 *
 * The operation, exactly (a caller can reproduce it):
 *     y[k][n] = sum over c < n_in, j < n_taps of  h[k][c][j] * x[c][n - j]
 *   - n runs on the object's own sample clock; x is zero before create and reset.  Inputs, taps and outputs are float32 and
 *     the arithmetic is float32.
 *   - METHOD: uniformly partitioned convolution at the block size B, P = ceil(n_taps / B) partitions (the last zero-padded),
 *     overlap-save on windows of 2B samples [x_{t-1} | x_t].  No latency beyond the filters: output block t is complete when
 *     input block t has been fed.  The forward transform of a window is taken ONCE and kept in a ring for the P - 1 blocks
 *     that follow; the products H[k][c][p] X[c][t - p] are summed over c and p in the frequency domain; there is one inverse
 *     transform per (PAIR of outputs, block) — outputs 2g and 2g + 1 ride through it as real and imaginary part.
 *   - ZERO PAIRS: a pair (k, c) whose taps are all zero (+0.0 or -0.0) is dropped at create.  A diagonal 24 x 24 matrix costs
 *     24 pairs, not 576.  The drop is observable: an input channel with no non-zero pair is never read (a NaN in it reaches
 *     no output), and an output with no non-zero pair is exactly +0.0.  A non-finite sample in a
 *     channel that IS read may reach every output, as 0 * NaN would in the formula.
 *   - ORDER: per frequency bin and output, an inner sum over p ascending (fused multiply-adds from zero) for each input
 *     channel, added to a running sum over c ascending.  No atomics: the same sequence of calls gives the same bits.
 *   - CUTS: a stream may be cut into calls in any way, always in whole blocks.  Different cuts agree within the accuracy of
 *     the method (tests: relative error per output channel <= 1.5 x that of one libear BlockConvolver per pair summed in
 *     float32); bit-identity across different cuts is NOT promised.  (Today every block has a transform of its own — unlike
 *     the decorrelators' kernel, which sends two consecutive blocks of a call through one complex transform, so that which
 *     blocks pair depends on where a call starts — but a faster pairing of blocks must stay possible.)
 * Everything is made at create: the filters' spectra [pairs][P][B] complex, the ring of input spectra
 * [channels read][max_blocks + P - 1][B] complex, one block of input per channel (double-buffered: the workgroups of a call's
 * last block rewrite it), and rows for max_blocks of the host form.  A process call allocates nothing and synchronises nothing.
 *
 * FILTER SETS (earhip_firmix_create_sets): a matrix may be made with room for n_sets filter sets of one shape (n_out, n_in,
 * n_taps, B), of which one is CURRENT at any time, and switched or crossfaded between them while it runs: a binaural monitor
 * that follows the listener's head, an EQ that is retuned.  The ring of input spectra does not depend on the filters, so
 * another set is applied to the SAME history: no restart, no cut-off tail, no second forward transform.  Exactly:
 *   - with y_s = h_s * x the formula above under set s over the WHOLE input history since create / reset,
 *     earhip_firmix_select(fm, set, F) makes the output, from the next block fed, go from the current set (`from`) to `set`
 *     (`to`) over F blocks:
 *         fade block q in [0, F), sample n in [0, B):  a = (float)(q B + n) / (float)(F B),
 *                                                      y = (1 - a) y_from + a y_to   in float32, each operation rounded
 *         every block after the fade:                  y = y_to
 *     F = 0 is a hard switch at the block boundary.  The ramp starts at 0 and never reaches 1 inside the fade, as libear's
 *     fade_down_and_up.
 *   - DIFFERENCE FROM libear's BlockConvolver::crossfade_filter: libear fades on the INPUT side — an input block is faded
 *     between the two filters and its tail rings out under the filter it arrived under.  Here the fade is on the OUTPUT side
 *     and both filters see the whole history: after the fade the output is exactly that of a matrix that had the new set
 *     from the start.
 *   - a fade's progress is a host integer: it runs on across calls, across the chunks of a render call that runs as a
 *     pipeline and across the two spans of a cut call.  The steady blocks of a call run through the same kernels, on the
 *     same ring and clock and in the same order of summation as a plain matrix: before a select and after a fade the output
 *     has the bits of earhip_firmix_create matrices of those sets fed the same calls.
 *   - an output with no non-zero pair in the set(s) applied to a block contributes exactly +0.0 there.
 *   - AGAINST earhip_firmix_create: the set selected next is not known at create, so every input channel has a ring row:
 *     every in[c] of the host form is looked at (none may be NULL) and every channel is read.  A NaN in a channel reaches no
 *     output WHILE NO SET IN USE (current, or being faded from) has a non-zero pair on it.  Everything any later call needs is
 *     made at create: spectra for every set at full width [n_sets][n_out n_in][P][B] complex, per-set pair lists, a pinned
 *     staging buffer for one set of taps.  earhip_firmix_create itself is what it was.
 *
 * Out of scope: block sizes that are not powers of two (480, 960, ...), interpolating HRIRs between measured directions, HRIR
 * data sets and SOFA files, interleaved PCM of the matrix's output, K-weighting of the monitor output (run a
 * second earhip_loudness over the sink), a multi-GPU matrix (after the exchange a rank owns whole channels and the matrix needs
 * all of them: run it on the gathering rank).
 * ---------------------------------------------------------------------- */
typedef struct earhip_firmix earhip_firmix;
typedef struct earhip_firmix_config {
  int n_in;           /* [1, 64] */
  int n_out;          /* [1, 64] */
  int block_size;     /* B: a power of two in [64, 4096] */
  int n_taps;         /* [1, 64 * B]: at most 64 partitions, as the renderer's decorrelators */
  const float *taps;  /* [n_out][n_in][n_taps], every one finite */
  int max_blocks;     /* >= 1: the longest process call */
} earhip_firmix_config;
/* anything outside the limits above is EARHIP_INVALID_ARGUMENT */
int earhip_firmix_create(earhip_ctx *ctx, const earhip_firmix_config *config, earhip_firmix **out);
/* (detach it from its renderers first: earhip_render_attach_firmix(r, NULL, NULL, 0, 0)) */
int earhip_firmix_destroy(earhip_firmix *fm);
/* state and clock to zero; a fade ends at once (its target is current); loaded sets stay loaded */
int earhip_firmix_reset(earhip_firmix *fm);
/* info = n_in, n_out, B, partitions, non-zero pairs (of the current set) */
int earhip_firmix_info(const earhip_firmix *fm, int info[5]);
/* planar float32 rows in device memory: input channel c at in_dev + c * in_stride, output k at out_dev + k * out_stride,
 * nblocks * B samples each, nblocks <= max_blocks (else EARHIP_INVALID_ARGUMENT, and nothing is consumed); enqueues on the
 * context's stream, does not synchronise.  Rows beyond the call's samples and other rows are left alone. */
int earhip_firmix_process_device(earhip_firmix *fm, size_t nblocks, const float *in_dev, size_t in_stride,
                                 float *out_dev, size_t out_stride);
/* host rows in[n_in], out[n_out] (the pointer of an input channel that is never read is not looked at); H2D + the above +
 * D2H; synchronises */
int earhip_firmix_process(earhip_firmix *fm, size_t nblocks, const float *const *in, float *const *out);
/* Filter sets (FILTER SETS above).  n_sets in [1, 4096]; config->taps becomes set 0, which is current; the other sets are
 * unloaded.  Limits as earhip_firmix_create. */
int earhip_firmix_create_sets(earhip_ctx *ctx, const earhip_firmix_config *config, int n_sets, earhip_firmix **out);
/* taps: host [n_out][n_in][n_taps], every one finite.  The set's all-zero pairs are dropped as at create.  Stages the taps and
 * enqueues their forward transforms on the context's stream, behind every call enqueued so far; may wait for an earlier load's
 * staging copy: not a call for the audio thread.  EARHIP_INVALID_ARGUMENT, and nothing changed: a set that is current or being
 * faded from, a set index out of range, a non-finite tap, a matrix made by earhip_firmix_create. */
int earhip_firmix_load_set(earhip_firmix *fm, int set, const float *taps);
/* the same with the taps in device memory (interpolated there, say): no pair is dropped, the host never sees the taps, and
 * finiteness is the caller's duty.  Neither allocates nor synchronises; taps_dev is read on the stream. */
int earhip_firmix_load_set_device(earhip_firmix *fm, int set, const float *taps_dev);
/* fade_blocks F in [0, 64].  Host bookkeeping only: no allocation, no synchronisation, no launch.  EARHIP_INVALID_ARGUMENT, and
 * nothing changed: an unloaded set, a set index out of range, F out of range, a select while a fade has started and not
 * finished (state[2] in [1, F)).  A select before any block of the previous select was fed replaces it (`from` stays).
 * Selecting the current set while no fade runs is a no-op.  While a fade is pending or running its target is `current`. */
int earhip_firmix_select(earhip_firmix *fm, int set, int fade_blocks);
/* state = current set, set being faded from (-1: none), fade blocks done, fade blocks in all */
int earhip_firmix_state(const earhip_firmix *fm, int state[4]);
/* info = loaded (0 / 1), non-zero pairs */
int earhip_firmix_set_info(const earhip_firmix *fm, int set, int info[2]);
/* From now on every process call of r, of EVERY form, feeds its float32 output rows to fm on the device, behind its kernels on
 * the context's stream and where an attached loudness meter is fed: the samples earhip_render_process_frames would hand back,
 * before any PCM conversion or dither.  fm's n_out rows go to sink_dev[k * sink_stride + position], position = the samples fed
 * since the attach (a host counter: the feeds are enqueued in order).  The sink is the caller's: device memory, or
 * earhip_host_alloc memory that a host caller reads after earhip_ctx_synchronize without a copy call.
 * fm must have the renderer's context, n_in = the renderer's n_out and its block size; sink_stride >= sink_capacity (else
 * EARHIP_INVALID_ARGUMENT).  A call that would pass sink_capacity, or fm's max_blocks, fails with EARHIP_INVALID_ARGUMENT
 * before anything is rendered.  A call that runs as two spans or as a pipeline of chunks is fed once per sample.
 * fm == NULL detaches (the other arguments are ignored); attaching again rewinds the position to 0.  A meter and a matrix may
 * be attached together.  earhip_render_reset does not touch fm; earhip_firmix_reset does.  earhip_firmix_select and
 * earhip_firmix_load_set between render calls act on the next block fed.  Without a matrix the render paths
 * are what they were. */
int earhip_render_attach_firmix(earhip_render *r, earhip_firmix *fm, float *sink_dev, size_t sink_stride,
                                size_t sink_capacity);
int earhip_render_firmix_position(earhip_render *r, size_t *samples);

/* ------------------------------------------------------------------------
 * (N) Look-ahead true-peak limiter — the last stage of a delivery chain, on the device.  libear has no counterpart.  The meter
 * of group L and the levels of group F can tell that a render passes -1 dBTP or clips an s16 file; this stage brings the bus
 * under a ceiling while it is still in device memory, with ONE gain for all channels, so that the spatial image is kept.
 *
 * The operation, exactly (a caller can reproduce it).  C channels, one object clock n since create / reset, x zero before the
 * clock starts.  All arithmetic is float32, each operation rounded once; nothing is contracted beyond the interpolator's
 * explicit fused multiply-adds (the library is built with -ffp-contract=off).  c is the ceiling, L the look-ahead, H the hold.
 *   1. DETECTOR.  detect = 1 (true peak): y_c[phases n + p] is the interpolator of group L bit for bit (the same table rules,
 *      the same order of taps), D = taps / 2 in integer division (6 for the annex 2 table), and
 *          e[n] = max over c of max(|x_c[n - D]|, max over p of |y_c[phases n + p]|).
 *      The interleaved 48-tap filter delays by 5.875 samples: y[4n .. 4n + 3] lies between x[n - 6] and x[n - 5], and D lines
 *      the two up.  detect = 0 (sample peak only): D = 0 and e[n] = max over c of |x_c[n]|.  The max ignores NaN, as the
 *      meter's does.
 *   2. REQUIRED GAIN.  r[n] = min(1, c / e[n]), the division one correctly rounded float32 division; e = 0 gives r = 1.
 *   3. SLIDING MINIMUM.  m[n] = min over i in [0, M) of r[n - i], M = L + 2 + H; r = 1 before the clock starts.  (The + 2 where
 *      + 1 would cover the look-ahead lets the window of output sample x[j] include the r of the inter-sample interval on BOTH
 *      its sides.)  min is exact: any algorithm gives the same bits.
 *   4. SMOOTHING.  s[n] = m[n] + m[n - 1] + .. + m[n - L]: K = L + 1 terms, added in that order starting from +0.0f with
 *      plain float32 adds;  g[n] = min(s[n] / (float)K, r[n - L]).  The outer min is a mathematical no-op (every m[n - k],
 *      k <= L, has r[n - L] in its window); it makes the guarantee below hold in float32 without a K 2^-24 slack.
 *   5. OUTPUT.  out_c[n] = x_c[n - D - L] g[n].  The latency is D + L samples (earhip_limiter_latency).  There is no flush call:
 *      a caller that wants the tail feeds D + L zeros.
 * GUARANTEE: for finite input |out_c[n]| <= c (1 + 2^-22) for every sample: g[n] <= r[n - L] <= fl(c / e[n - L]) and
 * |x_c[n - D - L]| <= e[n - L].  The TRUE peak of the output is not bounded exactly by any gain-riding limiter (modulating the
 * gain moves inter-sample peaks); for this design it is a measured property: at most 1.0021 c for L >= 64 on the tests'
 * signals, 1.0001 c for L = 240.
 * CUTS: any nsamples >= 0 per call, no block size.  Not one bit of out or g depends on how the stream is cut into calls,
 * launches, tiles or pipeline chunks (the fixed order of summation and the exact min).  The history — max(D + L, taps - 1)
 * samples per channel and M - 1 + L values of r, double-buffered — is carried exactly and made at create.
 * NON-FINITE INPUT: a NaN is ignored by the detector and passes through as NaN in its own channel only; +-infinity gives
 * r = 0 (the infinite sample itself comes out as inf x 0 = NaN).  Neither is guarded by extra passes.
 * STATISTICS: min_gain is the smallest g so far (1 if there was none below 1), limited_samples the number of n with g[n] < 1;
 * positive floats order like their bit patterns and the count is an integer, so both are independent of order and cuts.
 *
 * Out of scope: per-channel (unlinked) gains, exponential or programme-dependent release, oversampled gain application,
 * loudness normalisation, a multi-GPU limiter (the linked gain needs every channel: run it on the gathering rank), PCM from
 * the attached form (call earhip_limiter_process_pcm_device on rows instead).
 * ---------------------------------------------------------------------- */
typedef struct earhip_limiter earhip_limiter;
typedef struct earhip_limiter_config {
  int n_channels;              /* [1, 64] */
  int sample_rate;             /* > 0; with detect = 1 and no table of the caller's: 44100 or 48000 only, as the meter */
  float ceiling;               /* c: finite, > 0 (0.8913 = -1 dBTP) */
  int lookahead;               /* L in [8, 1024] samples */
  int hold;                    /* H in [0, 8192] samples */
  int detect;                  /* 0 sample peak | 1 true peak */
  const earhip_true_peak *tp;  /* detect = 1: NULL (or coeffs == NULL) = annex 2; else as earhip_loudness_create_tp */
  size_t max_samples;          /* >= 1: the longest process call */
} earhip_limiter_config;
/* Everything is made here: a process call allocates nothing and synchronises nothing.  Anything outside the limits above is
 * EARHIP_INVALID_ARGUMENT. */
int earhip_limiter_create(earhip_ctx *ctx, const earhip_limiter_config *config, earhip_limiter **out);
/* (detach it from its renderers first: earhip_render_attach_limiter(r, NULL, NULL, 0, 0)) */
int earhip_limiter_destroy(earhip_limiter *lim);
int earhip_limiter_reset(earhip_limiter *lim); /* history, clock, stats and levels to zero */
int earhip_limiter_latency(const earhip_limiter *lim, int *samples); /* D + L */
/* planar float32 rows in device memory: channel c at in_dev + c * in_stride and out_dev + c * out_stride, nsamples each; the
 * rows of in and out must not overlap.  gain_dev: [nsamples] g, or NULL.  nsamples > max_samples is EARHIP_INVALID_ARGUMENT
 * and nothing is consumed.  Enqueues on the context's stream, does not synchronise. */
int earhip_limiter_process_device(earhip_limiter *lim, size_t nsamples, const float *in_dev, size_t in_stride,
                                  float *out_dev, size_t out_stride, float *gain_dev);
/* host rows in[n_channels], out[n_channels], gain [nsamples] or NULL: H2D + the above + D2H; synchronises */
int earhip_limiter_process(earhip_limiter *lim, size_t nsamples, const float *const *in, float *const *out,
                           float *gain);
/* The limited rows as interleaved PCM frames in device memory: the conversion rules, argument checks and dither of group F
 * (earhip_render_process_frames_pcm_device), with n_channels in the place of n_out, through rows made at create.  The dither's
 * t is the limiter's own output clock.  The levels are the limiter's own (earhip_limiter_output_levels): with c < 1, clipped
 * stays 0 for s24 / s32 and for s16 without dither. */
int earhip_limiter_process_pcm_device(earhip_limiter *lim, size_t nsamples, const float *in_dev, size_t in_stride,
                                      void *out_dev, size_t out_frame_bytes, size_t out_first_byte,
                                      const earhip_pcm_out *out);
/* as earhip_render_output_levels, of the PCM form above: peak, clipped [n_channels]; synchronises */
int earhip_limiter_output_levels(earhip_limiter *lim, float *peak, uint64_t *clipped, int reset);
/* STATISTICS above; synchronises */
int earhip_limiter_stats(earhip_limiter *lim, float *min_gain, uint64_t *limited_samples, int reset);
/* From now on every process call of r, of EVERY form, feeds its float32 output rows to lim on the device, behind its kernels on
 * the context's stream and behind an attached loudness meter and FIR matrix, which both keep seeing the UNLIMITED bus: the
 * samples earhip_render_process_frames would hand back, before any PCM conversion or dither.  lim's n_channels rows go to
 * sink_dev[c * sink_stride + position], position = the samples fed since the attach (a host counter: the feeds are enqueued in
 * order).  The sink is the caller's: device memory, or earhip_host_alloc memory that a host caller reads after
 * earhip_ctx_synchronize without a copy call.  lim must have the renderer's context and n_channels = the renderer's n_out;
 * sink_stride >= sink_capacity (else EARHIP_INVALID_ARGUMENT).  There is no block-size condition: a feed is nblocks * B
 * samples.  A call that would pass sink_capacity, or lim's max_samples, fails with EARHIP_INVALID_ARGUMENT before anything is
 * rendered.  A call that runs as two spans or as a pipeline of chunks is fed once per sample.  lim == NULL detaches (the
 * other arguments are ignored); attaching again rewinds the position to 0.  earhip_render_reset does not touch lim;
 * earhip_limiter_reset does.  Without a limiter the render paths are what they were. */
int earhip_render_attach_limiter(earhip_render *r, earhip_limiter *lim, float *sink_dev, size_t sink_stride,
                                 size_t sink_capacity);
int earhip_render_limiter_position(earhip_render *r, size_t *samples);

/* ------------------------------------------------------------------------
 * (O) Biquad filter matrix — recursive filters on the output bus, on the device: bass management, loudspeaker or room EQ,
 * Linkwitz-Riley crossovers.  libear has no counterpart.  The FIR matrix of group M can stand in for these only with thousands
 * of taps (a 4th-order crossover at 80 Hz has pole radius 0.993); this stage runs the recursion itself, in parallel along time.
 *
 * The operation, exactly (a caller can reproduce it).  n_in input rows, n_out output rows, a list of R routes; route r is
 * (in_r, out_r, gain_r, S_r sections, coefficients [S_r][5] = b0 b1 b2 a1 a2).  One sample clock n since create / reset; every
 * state is zero before it starts.  Per route, float64 arithmetic on the float32 samples in transposed direct form II, every
 * multiply-add fused (ONE rounding), the sections in list order, x the input sample as a double, per section
 *     y = fma(b0, x, s1);   s1 = fma(-a1, y, fma(b1, x, s2));   s2 = fma(-a2, y, b2 * x);   the next section's x = y,
 * and z_r[n] = the last section's y.  S_r = 0 is a pure gain route: z_r[n] = (double)x[n].
 *     out_k[n] = (float)(sum over the routes with out_r = k, in ASCENDING LIST INDEX, of gain_r z_r[n]):
 * the sum is float64, starts from +0.0, takes one fused multiply-add per route, acc = fma(gain_r, z_r[n], acc), and is
 * rounded to float32 once.  An output without a route is written as +0.0.
 * STABILITY is checked at create: every section needs |a2| < 1 and |a1| < 1 + a2; all coefficients and gains must be finite.
 * DETERMINISM: the same calls give the same bits (no floating-point atomics, fixed orders everywhere).  The stage is NOT
 * bit-identical under different cuttings of the stream into calls: the time axis of a call is cut into chunks of
 * earhip_iir_info's length on the clock's grid, every chunk's start state is carried across the chunks before it with powers of
 * the cascade's transition matrix, and those propagated states round differently from the sample-by-sample recursion and
 * differently for different cuts.  What is promised under any cutting is accuracy:
 *     |out - ref| <= 2^-24 |ref| + 1e-9 (the peak of |ref| over that output row),
 * ref the float64 recursion above run sample by sample (scipy.signal.sosfilt per route, then the ordered sum): the first term is
 * the one rounding to float32.
 * NON-FINITE INPUT: from the first non-finite sample of an input row on, the outputs fed by routes that read that row are
 * unspecified non-finite values until earhip_iir_reset.  Earlier samples are untouched, and so are outputs fed only by other
 * rows.  There are no guard passes.
 *
 * Out of scope: per-route delays (the delay matrix of group S does them, in front of this stage), changing coefficients or
 * gains while running, crossfaded sets, float32 state, a multi-GPU stage (run it on the rank that owns whole channels, as the meter of group L), attaching the stage to a renderer as groups L, M
 * and N attach (feed it the rows a process call wrote: earhip_iir_process_device on the same context follows the call's kernels
 * on the stream).
 * ---------------------------------------------------------------------- */
typedef struct earhip_iir earhip_iir;
typedef struct earhip_iir_route {
  int in;               /* [0, n_in) */
  int out;              /* [0, n_out) */
  double gain;          /* finite */
  int n_sections;       /* S in [0, 8] */
  double coeffs[8][5];  /* the first S rows: b0 b1 b2 a1 a2 (a0 = 1) */
} earhip_iir_route;
typedef struct earhip_iir_config {
  int n_in;                       /* [1, 64] */
  int n_out;                      /* [1, 64] */
  int n_routes;                   /* R in [1, 512] */
  const earhip_iir_route *routes; /* [R]; copied */
  size_t max_samples;             /* >= 1: the longest process call */
} earhip_iir_config;
/* Everything is made here — the routes' states (2 S doubles each, double-buffered: a call reads one and writes the other), the
 * powers of the transition matrices (in long double, rounded once) and the chunk states [routes][chunks of max_samples][2 S]:
 * a process call allocates nothing and synchronises nothing.  Anything outside the limits above is EARHIP_INVALID_ARGUMENT. */
int earhip_iir_create(earhip_ctx *ctx, const earhip_iir_config *config, earhip_iir **out);
int earhip_iir_destroy(earhip_iir *iir);
int earhip_iir_reset(earhip_iir *iir); /* states and clock to zero */
/* info: [0] the chunk length Lc, [1] chunks per scan group, [2] scan groups chained per workgroup (a launch holds at most
 * [1] * [2] + 2 chunks; longer calls run as several launches), [3] routes, [4] the largest state size 2 S, [5] scratch bytes */
int earhip_iir_info(const earhip_iir *iir, int info[6]);
/* planar float32 rows in device memory: input i at in_dev + i * in_stride, output k at out_dev + k * out_stride, nsamples each,
 * any nsamples >= 0; the rows of in and out must not overlap.  nsamples > max_samples is EARHIP_INVALID_ARGUMENT and nothing
 * is consumed.  Enqueues on the context's stream, allocates nothing, does not synchronise. */
int earhip_iir_process_device(earhip_iir *iir, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                              size_t out_stride);
/* host rows in[n_in], out[n_out]: H2D + the above + D2H; synchronises */
int earhip_iir_process(earhip_iir *iir, size_t nsamples, const float *const *in, float *const *out);
/* A pure host function, no context and no device (like the host forms of groups K and L): one section b0 b1 b2 a1 a2 of the
 * RBJ audio EQ cookbook, normalised by a0.  q is the cookbook's Q for every kind (the shelves' too); gain_db is used by the
 * peaking and shelving kinds only.  Two Q = 1/sqrt(2) sections of one kind make a Linkwitz-Riley 4th-order filter.  f0 outside
 * (0, sample_rate / 2), q <= 0, an unknown kind or a non-finite argument is EARHIP_INVALID_ARGUMENT. */
#define EARHIP_IIR_LOWPASS 0
#define EARHIP_IIR_HIGHPASS 1
#define EARHIP_IIR_PEAKING 2
#define EARHIP_IIR_LOW_SHELF 3
#define EARHIP_IIR_HIGH_SHELF 4
int earhip_iir_design(int kind, double sample_rate, double f0, double q, double gain_db, double out[5]);

/* ------------------------------------------------------------------------
 * (P) Polyphase sample-rate converter — a rational rate change on the output bus, on the device: 44.1 or 96 kHz assets to a
 * 48 kHz bed, a 48 kHz render delivered at 44.1 kHz or monitored at 96 kHz.  libear has no counterpart.
 *
 * The operation, exactly (a caller can reproduce it).  The rate is L / M (up by L = `up`, down by M = `down`, gcd(L, M) = 1),
 * with T = `taps_per_phase` taps per phase and a prototype filter h[0 .. L T) given in float64.  The device holds
 *     c[p][k] = (float)h[p + k L],   p in [0, L), k in [0, T).
 * There is ONE input clock N, counted in samples since create or reset, a 64-bit host integer; x[i] is input sample i of a
 * channel's stream and x[i] = +0.0f for i < 0.  Output j of the stream belongs to input index i_j = floor(j M / L) and phase
 * p_j = (j M) mod L:
 *     acc = +0.0f;  for k = 0, 1, .. T - 1 in this order:  acc = fmaf(c[p_j][k], x[i_j - k], acc);   y[j] = acc
 * (float32, every multiply-add fused: ONE rounding each; subnormals are kept).  This is scipy.signal.upfirdn(h, x, L, M) sample
 * for sample, in float32 and in that order.  Every channel is converted alike and alone.
 * OUTPUT COUNT.  Output j exists once input i_j has been fed: after N inputs exactly ceil(N L / M) outputs have been produced
 * in total, and a call produces the difference between the totals before and after it.  That difference may be 0 (L / M =
 * 1 / 2: the second of two one-sample calls).  earhip_src_next_out tells it in advance.
 * FIXED WINDOWS.  Every output is a fixed function of a fixed window of T inputs in a fixed order, so
 *   - the same samples give the same BITS however the stream is cut into calls (the project's rule for non-recursive stages);
 *   - the device form and a plain C++ host form (std::fmaf in the order above) give the same bits;
 *   - a non-finite input sample s makes exactly the outputs with i_j - T + 1 <= s <= i_j non-finite, and no others;
 *   - there are no atomics anywhere.
 * LATENCY.  A linear-phase prototype delays by (L T - 1) / 2 prototype samples = (L T - 1) / (2 L) input samples =
 * (L T - 1) / (2 M) output samples (earhip_src_info); there is no flush call: feed that many zeros to get the tail.
 * LIMITS (anything outside is EARHIP_INVALID_ARGUMENT, checked before any device work): channels in [1, 64]; L, M in
 * [1, 1024] with gcd(L, M) = 1; T in [1, 256]; L T <= 32768; every tap finite, as a float32 too; max_samples >= 1.
 *
 * Out of scope: attaching the stage to a renderer as groups L, M and N attach (feed it the rows a process call wrote:
 * earhip_src_process_device on the same context follows the call's kernels on the stream; a stage that changes the sample
 * count does not fit the renderer's taps), time-varying ratios, float64 accumulation, PCM frames in or out of the stage.
 * ---------------------------------------------------------------------- */
typedef struct earhip_src earhip_src;
typedef struct earhip_src_config {
  int channels;        /* [1, 64] */
  int up;              /* L in [1, 1024] */
  int down;            /* M in [1, 1024], gcd(L, M) = 1 */
  int taps_per_phase;  /* T in [1, 256], L T <= 32768 */
  const double *taps;  /* h[L T]; copied */
  size_t max_samples;  /* >= 1: the longest process call, in input samples */
} earhip_src_config;
typedef struct earhip_src_properties {
  int up, down, taps_per_phase;
  int tile_out;       /* outputs of one tile of the kernel */
  int tile_in;        /* ceil(tile_out M / L): a tile's length in input samples */
  int table_in_lds;   /* 1: the kernel keeps c in LDS; 0: it reads c through the caches (large tables) */
  int window_in_lds;  /* 1: the kernel stages a tile's inputs in LDS; 0: it reads the rows directly (M / L beyond about 11) */
  size_t max_out;     /* ceil(max_samples L / M): no call produces more */
  double latency_prototype, latency_in, latency_out; /* (L T - 1) / 2, / (2 L), / (2 M) */
} earhip_src_properties;
/* Everything is made here — the table, the histories (the last T - 1 inputs per channel, double-buffered: a call reads one and
 * writes the other), device rows and pinned staging for the host form: a process call allocates nothing, and
 * earhip_src_process_device synchronises nothing. */
int earhip_src_create(earhip_ctx *ctx, const earhip_src_config *config, earhip_src **out);
int earhip_src_destroy(earhip_src *src);
int earhip_src_reset(earhip_src *src); /* histories to zero, clock to 0 */
int earhip_src_info(const earhip_src *src, earhip_src_properties *info);
/* what a call of nsamples inputs would produce now (nsamples > max_samples: EARHIP_INVALID_ARGUMENT) */
int earhip_src_next_out(const earhip_src *src, size_t nsamples, size_t *n_out);
/* planar float32 rows in device memory: input c at in_dev + c * in_stride (nsamples each, any nsamples >= 0), output c at
 * out_dev + c * out_stride (*n_out each; n_out may be NULL); the rows of in and out must not overlap.  nsamples > max_samples,
 * or an out_capacity (samples per output row) smaller than the call's outputs, is EARHIP_INVALID_ARGUMENT and nothing is
 * consumed.  A call with no input does nothing; a call with input and no output only advances the clock and the history.
 * Enqueues on the context's stream, allocates nothing, does not synchronise. */
int earhip_src_process_device(earhip_src *src, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                              size_t out_stride, size_t out_capacity, size_t *n_out);
/* host rows in[channels] of nsamples, out[channels] of out_capacity: H2D + the above + D2H; synchronises */
int earhip_src_process(earhip_src *src, size_t nsamples, const float *const *in, float *const *out, size_t out_capacity,
                       size_t *n_out);
/* A pure host function, no context and no device: a Kaiser-windowed sinc of length L T with its cutoff at `cutoff / max(L, M)`
 * of the prototype's Nyquist frequency, cutoff in (0, 1], normalised to unit DC gain and then multiplied by L — that is
 * L * scipy.signal.firwin(L * T, cutoff / max(L, M), window=("kaiser", beta)).  out[L T].  A ratio or T outside the limits
 * above, beta < 0, a cutoff outside (0, 1] or a non-finite argument is EARHIP_INVALID_ARGUMENT. */
int earhip_src_design(int up, int down, int taps_per_phase, double beta, double cutoff, double *out);

/* ------------------------------------------------------------------------
 * (Q) Ambisonic encoder for Objects, and a rotation of the HOA bus — the way INTO the scene-based domain: Objects positions
 * become the gain vectors of an Ambisonics bus (for a scene-based ADM pack, an AmbiX / FuMa file, or binaural monitoring through
 * the SH domain), where earhip_hoa_decode_matrix (group I) is the way out of it.  libear has no counterpart; the conventions
 * are those of its hoa::sph_harm (src/hoa/hoa.hpp:99-112) and therefore of the decoder: D_norm * enc_norm does not depend on
 * the normalization.
 *
 * CHANNELS.  Input channel c of the bus is the pair (n, m) = (orders[c], degrees[c]), 1 <= n_coef <= 64, 0 <= n <= 7,
 * |m| <= n.  Any subset, order or repetition of channels is accepted (AmbiX: earhip_hoa_acn; FuMa W X Y Z: (0,0) (1,1) (1,-1)
 * (1,0)).  normalization is "N3D", "SN3D" or "FuMa"; FuMa requires n <= 3.  An unknown normalization name is EARHIP_ADM_ERROR,
 * as in the decoder; any other violation is EARHIP_INVALID_ARGUMENT.
 *
 * THE ENCODED VALUE, exactly (a caller can reproduce it).  A source at ADM polar azimuth az and elevation el (degrees, azimuth
 * anticlockwise-positive: +90 is left) with linear gain g gives, with a = |m|,
 *     out[i][c] = (float)( g * K(n, a) * P_n^a(x) * T_m(r) ),    x = sin(el * pi/180),   r = fmod(az, 360) * pi/180
 * in float64, the product taken from left to right, ONE rounding to float32 at the end (pi/180 is the double nearest to it, fmod
 * is exact, so any finite azimuth is reduced without error before the conversion to radians, as in group K).
 *   P_n^a is the associated Legendre function WITHOUT the Condon-Shortley phase, by upward recurrence in n:
 *     s = sqrt((1 - x) * (1 + x));   P_a^a = 1 * (1 s) * (3 s) * ... * ((2a - 1) s), one factor (2i - 1) * s at a time;
 *     P_(a+1)^a = x * (2a + 1) * P_a^a;   P_l^a = (x * (2l - 1) * P_(l-1)^a - (l + a - 1) * P_(l-2)^a) / (l - a).
 *   T_m(r) = sqrt2 * cos(m r) for m > 0, 1 for m = 0, -sqrt2 * sin(m r) for m < 0 (m r is the product of the integer m, as a
 *     double, and r).
 *   K(n, a): SN3D = sqrt((n - a)! / (n + a)!); N3D = sqrt(2n + 1) * SN3D; FuMa = f[n][a] * SN3D with f = 1/sqrt2 for (0,0);
 *     1 for (1,0) (1,1) (2,0) (3,0); 2/sqrt3 for (2,1) (2,2); sqrt(45/32) for (3,1); 3/sqrt5 for (3,2); sqrt(8/5) for (3,3).
 * So W = g (SN3D, N3D) or g / sqrt2 (FuMa), and N3D at az 90, el 0 has Y_1^-1 = sqrt3, Y_1^1 = 0.
 * The host form and the device kernel run these operations in this order (one shared core, csrc/hoa_encode.h); they differ only
 * in the math library behind sin, cos, sqrt and fmod, so an output of one is the other's float or its neighbour.
 *
 * earhip_hoa_acn fills (max_order + 1)^2 pairs in ACN order: channel k is n = floor(sqrt k), m = k - n^2 - n; 0 <= max_order
 * <= 7.  Pure host.
 * earhip_hoa_encode is a pure host function, no context and no device (like the host forms of group K it is a deliberate CPU
 * computation on the calling thread, not a fall-back of the device form).  gain may be NULL (1).  out: [n][n_coef] float,
 * row-major.  A non-finite azimuth, elevation or gain, or |el| > 90, is EARHIP_INVALID_ARGUMENT, the message naming the
 * element's index; the rows before it are written, its row and those after it are not.
 * earhip_hoa_encode_device takes SoA float64 device arrays of n elements (device-reachable host memory included; gain_dev may be
 * NULL) and out_dev [n][n_coef] float; it runs ONE kernel on the context's stream, allocates nothing, does not synchronise and
 * never computes on the CPU.  It cannot refuse an element: an element the host form refuses gets NaN in all its n_coef outputs
 * and status 1, every other element status 0 (status_dev: int[n], may be NULL).  n == 0 is a no-op; n < 2^31.  The kernel
 * gives a wave 64 positions: each lane evaluates its position's Legendre and trigonometric terms once, and the wave's 64 rows
 * leave through LDS as full-width stores; no atomics, the same input gives the same bits.
 * As gain curves: a direct-only renderer (group F, n_buses = 1, n_out = n_coef) is an Ambisonics bus as soon as its curves
 * hold these rows (earhip_render_set_object_points).
 *
 * earhip_hoa_rotation_matrix (pure host): the matrix that turns the bus.  q: double[9], row-major, acting on ADM Cartesian
 * column vectors (x right, y front, z up): a source at u moves to q u.  q must be orthonormal with determinant +1 (every entry
 * of q q^T - I and det q - 1 within 1e-9), else EARHIP_INVALID_ARGUMENT.  out: [n_coef][n_coef] float, row-major, with the
 * DEFINING PROPERTY: for every direction u,  enc(q u) = out * enc(u)  — for a channel list that holds every degree of each of
 * its orders exactly once (a rotation mixes the 2n + 1 channels of an order among themselves); for any other list out[i][j] is
 * still the coefficient of channel j's harmonic in the rotated harmonic of channel i.  Entries between channels of different
 * order are exactly 0.  It is computed by quadrature over the 5200-point spherical t-design the decoder uses, in N3D,
 *     R[i][j] = (1/5200) * sum_p Y_i(q x_p) Y_j(x_p),   out[i][j] = (float)( R[i][j] * (K(i) / K_N3D(i)) * (K_N3D(j) / K(j)) )
 * (the design integrates products of harmonics up to order 7 to 2.3e-12; the property holds to 2.4e-11 before the rounding to
 * float).  How to apply it: a static rotation by earhip_interp_apply_constant (n_in = n_out = n_coef, point[j * n_coef + i] =
 * out[i][j]: input channel j to output channel i); a head-tracked one as the interpolation points of earhip_gain_interp_*
 * (group A'), one matrix per head pose at its sample time.
 *
 * Out of scope: extent or diffuse in the SH domain, per-order weights (max-rE, in-phase), orders above 7, near-field
 * compensation, attaching anything to a renderer, a device form of the rotation matrix (64 x 64 host arithmetic per head pose).
 * ---------------------------------------------------------------------- */
int earhip_hoa_acn(int max_order, int *orders, int *degrees);
int earhip_hoa_encode(int n_coef, const int *orders, const int *degrees, const char *normalization, size_t n,
                      const double *azimuth, const double *elevation, const double *gain, float *out);
int earhip_hoa_encode_device(earhip_ctx *ctx, int n_coef, const int *orders, const int *degrees, const char *normalization,
                             size_t n, const double *azimuth_dev, const double *elevation_dev, const double *gain_dev,
                             float *out_dev, int *status_dev);
int earhip_hoa_rotation_matrix(int n_coef, const int *orders, const int *degrees, const char *normalization, const double *q,
                               float *out);

/* ------------------------------------------------------------------------
 * (R) The screen of an Objects block: screenRef scaling and screenEdgeLock (ITU-R BS.2127-0 sections 7.3.3 and 7.3.4).  libear
 * refuses screenRef (src/object_based/gain_calculator_objects.cpp:37-44) and so does every calculator of group I; this group is
 * the stage that turns a reference screen and a reproduction screen into positions.  In the renderer's order both steps are
 * transforms of the polar position that run before channel lock, divergence, extent and zone exclusion, so the stage stands in
 * front of earhip_panner_calculate_objects[_device] as group K does: SoA float64 arrays, rewritten in place on the device, which
 * the panner then reads.  A Cartesian block goes earhip_conversion_to_polar_device, this stage, the panner: three launches and
 * no host round trip.  Distance is never changed by either step, so it is not an argument.  This comment is the specification.
 *
 * A SCREEN is earhip_screen: cartesian 0 is libear's PolarScreen (aspect_ratio, centre azimuth / elevation / distance,
 * width_azimuth: the full width in degrees), anything else its CartesianScreen (aspect_ratio, centre x / y / z, width_x: the
 * full width); the fields of the other kind are not read.  earhip_screen_default: polar, 1.78, (0, 0, 1), 58 degrees.
 *
 * EDGES (earhip_screen_edges, pure host, float64): edges[4] = left azimuth, right azimuth, bottom elevation, top elevation, in
 * degrees.  With cart(az, el, d) = (sin(-az) cos(el) d, cos(-az) cos(el) d, sin(el) d), azim(v) = -atan2(v.x, v.y) and
 * elev(v) = atan2(v.z, hypot(v.x, v.y)):
 *   polar:     c = cart(az, el, d), W = d tan(width_azimuth / 2), H = W / aspect_ratio,
 *              xv = W cart(az - 90, 0, 1), zv = H cart(az, el + 90, 1);
 *   Cartesian: c = (x, y, z), W = width_x / 2, H = W / aspect_ratio, xv = (W, 0, 0), zv = (0, 0, H);
 *   both:      left = azim(c - xv), right = azim(c + xv), bottom = elev(c - zv), top = elev(c + zv).
 * The default screen's edges are 29, -29, -17.297..., 17.297....  EARHIP_INVALID_ARGUMENT, the message naming the field: a
 * non-finite field; aspect_ratio <= 0; width_azimuth outside (0, 180) or width_x <= 0; a polar distance <= 0 or |elevation| >
 * 90; edges that do not satisfy -180 < right < left < 180 and -90 < bottom < top < 90 (a screen across the rear seam or over a
 * pole, where the scaling has no ordered breakpoints).
 *
 * APPLY, per element i.  A NULL reference is the default screen.  With a NULL reproduction both steps are the identity: every
 * element is copied bit for bit and none is checked.  A NULL flag array means all 0, except a NULL screen_ref, which means all
 * 1.  Lock codes: horizontal 0 none, 1 left, 2 right; vertical 0 none, 1 bottom, 2 top.
 *   1. An element with screen_ref[i] == 0 and both lock codes 0 is copied bit for bit, whatever it holds (a NaN too; status 0).
 *   2. Any other element is checked first: a non-finite azimuth or elevation, |azimuth| > 2^40 (group K's bound), |elevation| >
 *      90 or a lock code above 2 is refused.  The host form returns EARHIP_INVALID_ARGUMENT, the message naming the index; the
 *      elements before it are written, it and those after it are not.  The device form cannot refuse: such an element gets NaN
 *      in both outputs and status[i] = 1, every other element status[i] = 0 (status: int[n], may be NULL).
 *   3. SCALE, when screen_ref[i] is nonzero.  a = fmod(azimuth, 360), then one step of -+360 brings it into [-180, 180] (fmod is
 *      exact, as in group K).  The new azimuth is the piecewise-linear map of a through the breakpoints (-180, ref.right,
 *      ref.left, 180) -> (-180, rep.right, rep.left, 180); the new elevation that of the elevation through (-90, ref.bottom,
 *      ref.top, 90) -> (-90, rep.bottom, rep.top, 90).  A segment is (x0, y0, slope), slope = (y1 - y0) / (x1 - x0) computed on
 *      the host; the segment of x is the one whose x0 is the largest breakpoint <= x; the value is fma(slope, x - x0, y0), ONE
 *      explicit fused multiply-add on host and device alike.  x >= 180 gives exactly 180 and x >= 90 exactly 90: the seam and
 *      the poles map to themselves, and a reference edge maps to the reproduction edge exactly.
 *   4. LOCK, after the scale: horizontal 1 / 2 sets the azimuth to rep.left / rep.right, vertical 1 / 2 the elevation to
 *      rep.bottom / rep.top.
 *   5. A component that is neither scaled nor locked keeps its input bits (the azimuth under a vertical lock alone is not even
 *      reduced).
 * Each output may alias its own input, so the stage can run in place.  n == 0 is a no-op; n < 2^31.
 *
 * earhip_screen_apply is a deliberate CPU computation on the calling thread, no context and no device, like the host forms of
 * group K.  earhip_screen_apply_device takes the two screens in host memory and the arrays as device pointers (device-reachable
 * host memory included); it runs ONE kernel on the context's stream (one thread per element, the six segments a by-value
 * argument), allocates nothing, does not synchronise and never computes on the CPU.  The per-element arithmetic has no libm call
 * but the exact fmod and its only contraction is explicit (one shared core, csrc/screen.h), so THE DEVICE FORM RETURNS THE HOST
 * FORM'S BITS.
 *
 * Out of scope: screenRef for HOA, a reproduction screen on a layout,
 * fusing the stage into the producer's kernels.
 * ---------------------------------------------------------------------- */
typedef struct earhip_screen {
  int cartesian;                       /* 0: PolarScreen, else CartesianScreen */
  double aspect_ratio;
  double azimuth, elevation, distance; /* polar centrePosition */
  double x, y, z;                      /* Cartesian centrePosition */
  double width_azimuth;                /* polar: full width in degrees */
  double width_x;                      /* Cartesian: full width */
} earhip_screen;

int earhip_screen_default(earhip_screen *out);
int earhip_screen_edges(const earhip_screen *s, double edges[4]);
int earhip_screen_apply(const earhip_screen *reference, const earhip_screen *reproduction, size_t n, const double *azimuth,
                        const double *elevation, const unsigned char *screen_ref, const unsigned char *lock_horizontal,
                        const unsigned char *lock_vertical, double *azimuth_out, double *elevation_out);
int earhip_screen_apply_device(earhip_ctx *ctx, const earhip_screen *reference, const earhip_screen *reproduction, size_t n,
                               const double *azimuth, const double *elevation, const unsigned char *screen_ref,
                               const unsigned char *lock_horizontal, const unsigned char *lock_vertical, double *azimuth_out,
                               double *elevation_out, int *status);

/* ------------------------------------------------------------------------
 * (S) Delay matrix — delays that differ per channel on the output bus, on the device: time alignment of loudspeakers at
 * unequal distances, a subwoofer against its mains, a lip-sync offset on the whole bus.  Group D (libear's DelayBuffer) delays
 * every channel by one amount; this stage is a sparse matrix of delayed short FIRs in the time domain.
 *
 * The operation, exactly (a caller can reproduce it).  n_in input rows, n_out output rows, a list of R routes; route r is
 * (in_r, out_r, D_r, T_r, h_r[0 .. T_r)): D_r a whole delay in samples, h_r T_r float32 taps.  A pure gain or polarity is
 * T = 1; a fractional delay is a designed h (earhip_delaymix_fractional).  One sample clock n counts since create or reset;
 * x_c[i] = +0.0f for i < 0.
 *     acc = +0.0f
 *     for the routes with out_r = k, in ASCENDING LIST INDEX:
 *       for j = 0 .. T_r - 1 in this order:
 *         acc = fmaf(h_r[j], x_{in_r}[n - D_r - j], acc)
 *     out_k[n] = acc
 * (float32, every multiply-add fused: ONE rounding each; subnormals are kept).  An output without a route is written as +0.0f.
 * An input without a route is never read: a NaN in it reaches nothing, and the host form does not look at its pointer.
 * FIXED WINDOWS.  Every output is a fixed function of fixed windows in a fixed order, so
 *   - the same samples give the same BITS however the stream is cut into calls (the project's rule for non-recursive stages);
 *   - the device form and a plain C++ host form (std::fmaf in the order above) give the same bits;
 *   - a non-finite input sample s of row c makes non-finite exactly those outputs n of the rows fed by a route r reading c for
 *     which n - D_r - T_r + 1 <= s <= n - D_r, and no others;
 *   - there are no atomics anywhere.
 * LIMITS (anything outside is EARHIP_INVALID_ARGUMENT, checked before any device work): n_in and n_out in [1, 64]; R in
 * [1, 512]; T_r in [1, 32]; D_r in [0, 65536]; every tap finite; max_samples >= 1.
 *
 * Out of scope: changing or crossfading routes while running, time-varying delays, PCM frames in or out of the stage, a
 * multi-GPU stage, attaching the stage to a renderer as groups L, M and N attach (feed it the rows a process call wrote:
 * earhip_delaymix_process_device on the same context follows the call's kernels on the stream).
 * ---------------------------------------------------------------------- */
typedef struct earhip_delaymix earhip_delaymix;
typedef struct earhip_delaymix_route {
  int in;          /* [0, n_in) */
  int out;         /* [0, n_out) */
  int delay;       /* D in [0, 65536] */
  int n_taps;      /* T in [1, 32] */
  float taps[32];  /* the first T: h[0 .. T), finite */
} earhip_delaymix_route;
typedef struct earhip_delaymix_config {
  int n_in;                            /* [1, 64] */
  int n_out;                           /* [1, 64] */
  int n_routes;                        /* R in [1, 512] */
  const earhip_delaymix_route *routes; /* [R]; copied */
  size_t max_samples;                  /* >= 1: the longest process call */
} earhip_delaymix_config;
typedef struct earhip_delaymix_properties {
  int tile_out;        /* outputs of one tile of the kernel */
  size_t launch_in;    /* inputs of one launch: a longer call runs as several launches */
  int routes;          /* R */
  int history;         /* H = max_r (D_r + T_r - 1) */
  int max_fan_in;      /* the most routes into one output */
  int total_taps;      /* sum of T_r */
  size_t device_bytes; /* device memory the stage holds */
} earhip_delaymix_properties;
/* Everything is made here — the tap and route tables, the histories (the last H = max_r (D_r + T_r - 1) inputs of every row
 * that is read, double-buffered: a call reads one and writes the other; a call shorter than H keeps the tail of the old
 * history in front of its own samples), device rows and pinned staging for the host form: a process call allocates nothing,
 * and earhip_delaymix_process_device synchronises nothing. */
int earhip_delaymix_create(earhip_ctx *ctx, const earhip_delaymix_config *config, earhip_delaymix **out);
int earhip_delaymix_destroy(earhip_delaymix *dm);
int earhip_delaymix_reset(earhip_delaymix *dm); /* histories and clock to zero */
int earhip_delaymix_info(const earhip_delaymix *dm, earhip_delaymix_properties *info);
/* planar float32 rows in device memory: input i at in_dev + i * in_stride, output k at out_dev + k * out_stride, nsamples each,
 * any nsamples in [0, max_samples]; the rows of in and out must not overlap; no alignment beyond a float's is asked of a row.
 * nsamples > max_samples is EARHIP_INVALID_ARGUMENT and nothing is consumed.  Samples beyond nsamples and other rows are left
 * alone.  Enqueues on the context's stream, allocates nothing, does not synchronise. */
int earhip_delaymix_process_device(earhip_delaymix *dm, size_t nsamples, const float *in_dev, size_t in_stride, float *out_dev,
                                   size_t out_stride);
/* host rows in[n_in], out[n_out] (in[c] of a row no route reads may be anything): H2D + the above + D2H; synchronises */
int earhip_delaymix_process(earhip_delaymix *dm, size_t nsamples, const float *const *in, float *const *out);
/* Two pure host designers, no context and no device.
 * earhip_delaymix_fractional: a delay of `delay` samples as a route's whole delay and n_taps = T taps (taps[T], float64; the
 * route takes them as float32).  T = 1: whole = floor(delay + 0.5), the tap is 1.  T even in [2, 32]: with c = T / 2 - 1
 * (delay >= c is required), whole = floor(delay - c), mu = delay - c - whole, t_j = j - c - mu,
 *     h_j = sinc(t_j) I0(beta sqrt(max(0, 1 - (2 t_j / T)^2))) / I0(beta),   sinc(t) = sin(pi t) / (pi t), sinc(0) = 1,
 * and h is then divided by its sum.  An odd T > 1, T outside [1, 32], beta < 0, a delay that is negative, non-finite or gives
 * whole > 65536 is EARHIP_INVALID_ARGUMENT.
 * earhip_delaymix_align: loudspeakers at distance_m[n] brought to the farthest one's arrival time and level:
 * delay_samples[c] = (d_max - d_c) / speed_of_sound * sample_rate, gain[c] = d_c / d_max.  n < 1, a distance <= 0 or non-finite,
 * a rate or speed <= 0 or non-finite is EARHIP_INVALID_ARGUMENT. */
int earhip_delaymix_fractional(double delay, int n_taps, double beta, int *whole, double *taps);
int earhip_delaymix_align(int n, const double *distance_m, double sample_rate, double speed_of_sound, double *delay_samples,
                          double *gain);

/* ------------------------------------------------------------------------
 * (T) The allocentric (Cartesian) point-source panner for Objects — what ITU-R BS.2127-0 section 7.3.10 sends an
 * audioBlockFormat with cartesian == 1 to.  It stands the loudspeakers on a cube and pans along z, then y, then x.  The other
 * way to render such a block, earhip_conversion_to_polar[_device] (group K) and then the polar panner (group I), gives
 * different gains, and an object at the centre of the room, (0, 0, 0), has no polar direction at all.  libear carries only a
 * stub (AllocentricPanner::handle returns boost::none), and ear::GainCalculatorObjects and ear::hip::ObjectsGainCalculator keep
 * refusing Cartesian blocks.  THIS COMMENT IS THE SPECIFICATION.  It was written after BS.2127-0 7.3.10 WITHOUT A REFERENCE
 * IMPLEMENTATION TO COMPARE AGAINST; the loudspeaker table can be replaced by the caller (earhip_allo_create_positions), so a
 * disagreement about a table entry does not block a user.
 *
 * THE HANDLE is pure host data: no context, no device.  layout is a BS.2051 name or a layout defined through group H, looked up
 * once, at creation; an unknown name is EARHIP_UNKNOWN_LAYOUT.  earhip_allo_create takes the built-in table below and is
 * EARHIP_NOT_IMPLEMENTED for a defined layout, which has no table.  earhip_allo_create_positions takes one (x, y, z) per channel
 * of the full layout (at most 32, the registry's limit); LFE entries are ignored; a non-finite coordinate of a channel that is
 * not an LFE, or n_channels other than the layout's channel count, is EARHIP_INVALID_ARGUMENT.
 *   SNAPPING, once, at creation, per axis: the coordinates of the loudspeakers that are not LFE are sorted ascending and
 *   walked; a value within 1e-6 of the FIRST value of the current group takes that first value, any other value starts a
 *   group.  After this "the same plane, row or column" is exact equality.  Two loudspeakers that end up on the same (x, y, z)
 *   are EARHIP_INVALID_ARGUMENT.
 * earhip_allo_positions returns the snapped positions, xyz [n_channels][3], the rows of LFE channels NaN.
 * earhip_allo_excluded_channels sets bit c of *mask when loudspeaker c (not an LFE) lies in at least one zone, by the Cartesian
 * rule of group I against the HANDLE'S positions: min - 1e-6 < c < max + 1e-6 for each coordinate.  Only Cartesian zones
 * count: a polar zone is EARHIP_INVALID_ARGUMENT (earhip_objects_excluded_channels takes polar zones, on nominal positions).
 *
 * THE BUILT-IN TABLE.  ADM axes: x right, y front, z up; s = sqrt(2) - 1; a +- row gives the + name (left) first.
 *     M+000 (0, 1, 0)        M+-030 (-+1, 1, 0), except in 9+10+3: (-+s, 1, 0)          M+-SC (-+s, 1, 0)
 *     M+-060 (-+1, s, 0)     M+-090 (-+1, 0, 0)     M+-110 (-+1, -1, 0)     M+-135 (-+1, -1, 0)     M+180 (0, -1, 0)
 *     U+000 (0, 1, 1)        U+-030 (-+1, 1, 1)     U+-045 (-+1, 1, 1)      U+-090 (-+1, 0, 1)      U+-110 (-+1, -1, 1)
 *     U+-135 (-+1, -1, 1)    U+180 (0, -1, 1)       UH+180 (0, -1, 1)       T+000 (0, 0, 1)
 *     B+000 (0, 1, -1)       B+-045 (-+1, 1, -1)
 * Every channel of the ten layouts of group H that is not an LFE is in this list (csrc/allo_table.h, keyed by (layout, name)).
 *
 * THE GAINS, exactly (a caller can reproduce them).  Let A be the loudspeakers (channels that are not LFE) whose bit in the
 * object's excluded mask is clear; if that leaves none, A is every loudspeaker.
 *   bracket(V, v), for a non-empty set V of distinct doubles: lo = the largest element <= v, hi = the smallest element >= v.
 *     No lo: {hi: 1}.  No hi: {lo: 1}.  lo == hi: {lo: 1}.  Otherwise, with f = (v - lo) / (hi - lo):
 *     {lo: cos(f * (pi/2)), hi: sin(f * (pi/2))}, pi/2 the double nearest to it, the product f * (pi/2) taken first.
 *     A position outside the loudspeakers' box is therefore clipped to it.
 *   For an object at (x, y, z):
 *     1. for each (Z, wz) in bracket({z_i : i in A}, z):  P = {i in A : z_i == Z};
 *     2. for each (Y, wy) in bracket({y_i : i in P}, y):  R = {i in P : y_i == Y};
 *     3. for each (X, wx) in bracket({x_i : i in R}, x):  the one i in R with x_i == X gets w_i = (wz * wy) * wx;
 *     4. every other channel gets 0.
 *   At most 8 channels are non-zero, sum w^2 = 1 up to rounding, and a position on a loudspeaker gives exactly 1 there and
 *   exactly 0 elsewhere.
 *   Outputs, in float64, left to right, ONE rounding to float32:
 *     direct[i][c] = (float)(w_c * gain * sqrt(1 - diffuse)),   diffuse_out[i][c] = (float)(w_c * gain * sqrt(diffuse)).
 *   The columns of LFE channels are +0.
 * The host form and the kernel run these operations in this order (one shared core, csrc/allo.h, which also compiles without
 * HIP); they differ only in the math library behind cos, sin and sqrt, so an output of one is the other's float or its
 * neighbour.
 *
 * ENTRY POINTS.  gain, diffuse and excluded may be NULL (1, 0 and 0); diffuse_out may be NULL only when diffuse is NULL.
 * direct and diffuse_out are [n][n_channels] float, row-major.  n == 0 is a no-op; n < 2^31.
 * earhip_allo_calculate is a pure host function (a deliberate CPU computation on the calling thread, like the host forms of
 * groups K and Q).  EARHIP_INVALID_ARGUMENT, the message naming the element's index: a non-finite x, y, z or gain; a diffuse
 * that is NaN or outside [0, 1]; a mask bit at or beyond the channel count (bits of LFE channels are ignored).  The rows before
 * that index are written, its row and those after it are not.
 * earhip_allo_calculate_device takes SoA device arrays of n elements (device-reachable host memory included); it runs ONE kernel
 * on the context's stream, allocates nothing, does not synchronise and never computes on the CPU.  It cannot refuse an element:
 * an element the host form would refuse gets NaN in every column of both rows and status 1 — except that mask bits at or
 * beyond the channel count are ignored — and every other element status 0 (status_dev: int[n], may be NULL).  The kernel gives
 * a wave 64 positions, one per lane, the snapped table a by-value argument; a lane keeps its at most 8 weights in registers and
 * the wave's 64 rows leave through one LDS tile as full-width contiguous stores, first direct, then diffuse_out.  No atomics:
 * the same input gives the same bits.
 *
 * Out of scope: attaching anything to a renderer, tables for layouts outside BS.2051.  The Cartesian extent panner (width, height, depth),
 * channelLock for Cartesian blocks and Cartesian objectDivergence are group U, on this handle; the entry points of this group
 * stay point-source.
 * ---------------------------------------------------------------------- */
typedef struct earhip_allo earhip_allo;
int earhip_allo_create(const char *layout, earhip_allo **out);
int earhip_allo_create_positions(const char *layout, int n_channels, const double *x, const double *y, const double *z,
                                 earhip_allo **out);
int earhip_allo_destroy(earhip_allo *a);
int earhip_allo_num_channels(const earhip_allo *a, int *n_channels);
int earhip_allo_positions(const earhip_allo *a, double *xyz);
int earhip_allo_excluded_channels(const earhip_allo *a, int n_zones, const earhip_exclusion_zone *zones, uint32_t *mask);
int earhip_allo_calculate(const earhip_allo *a, size_t n, const double *x, const double *y, const double *z, const double *gain,
                          const double *diffuse, const uint32_t *excluded, float *direct, float *diffuse_out);
int earhip_allo_calculate_device(earhip_ctx *ctx, const earhip_allo *a, size_t n, const double *x_dev, const double *y_dev,
                                 const double *z_dev, const double *gain_dev, const double *diffuse_dev,
                                 const uint32_t *excluded_dev, float *direct_dev, float *diffuse_out_dev, int *status_dev);

/* ------------------------------------------------------------------------
 * (U) Extent, channelLock and objectDivergence for the allocentric panner, on the handle of group T: with these (and the
 * screen stage of group V in front of them) every Cartesian Objects block is rendered allocentrically, on the host or as one device launch over a resident batch.
 * libear carries only a stub here too.  THIS COMMENT IS THE SPECIFICATION.  It was written after BS.2127-0 7.3.6, 7.3.7 and
 * 7.3.11 WITHOUT A REFERENCE IMPLEMENTATION TO COMPARE AGAINST and without the Recommendation's text at hand; three sets of
 * constants are THIS PROJECT'S READING: the lock weights 1/16, 4, 32; the 20-point grid; the fall-off 10^(-5.0625 (u^4 - 1)).
 *
 * A, bracket(), the snapped table and the point-source weights w(q) of a position q are group T's.  s_c is the handle's
 * snapped position of loudspeaker c.  Per object, in this order:
 *   1. CHANNEL LOCK (channel_lock[i] non-zero).  Candidates are every loudspeaker that is not an LFE, the excluded ones too.
 *        d_c = sqrt((1/16) (x - s_c.x)^2 + 4 (y - s_c.y)^2 + 32 (z - s_c.z)^2).
 *      With a maxDistance, only loudspeakers with d_c < maxDistance + 1e-10 stay; if none is left, the position is unchanged.
 *      Among those with d_c < min d + 1e-10, the first in the lock priority order wins, and the position becomes s_c.
 *      THE LOCK PRIORITY ORDER is the indices of the loudspeakers that are not LFE, ascending by (|z|, z, -y, |x|, x) of the
 *      snapped positions; earhip_allo_lock_priority returns it, one int per loudspeaker that is not an LFE.
 *   2. DIVERGENCE v with positionRange r.  v == 0: the one position, with weight 1.  Otherwise the positions (x, y, z),
 *      (x - r, y, z) and (x + r, y, z) with the power weights (1 - v) / (1 + v), v / (1 + v) and v / (1 + v).  Nothing is
 *      clipped here; bracket() and step 3 clip.
 *   3. EXTENT of each position q, with size = (width, depth, height) on (x, y, z).
 *      Per handle: axis k is FLAT when all loudspeakers that are not LFE share its snapped coordinate.  A flat axis has one
 *      grid point, at that coordinate, with F = 1.  A non-flat axis has the grid c_j = (2 j - 19) / 19, j = 0 .. 19.
 *        s_k = min(size_k, 1) on the non-flat axes; s_eff their mean, s_max their maximum (both 0 when all axes are flat);
 *        p = 6 for s_eff <= 0.5, else 6 - 8 (s_eff - 0.5);      alpha = min(s_max / 0.2, 1).
 *      If s_max == 0 then g(q) = w(q) exactly, and nothing below is evaluated.  Otherwise, on a non-flat axis, with
 *        o_k = clamp(q_k, -1, 1),   h_k = max(size_k, 0.1),   u = max(|c - o_k|, h_k) / h_k:    F_k(c) = 10^(-5.0625 (u^4 - 1)),
 *      a plateau of half-width h_k and value 1 (the floor 0.1 keeps at least one grid point on it) and a steep fall beyond.
 *      Over every grid source s = (c_i, c_j, c_l), with w_c(s) group T's weights of s under the object's mask:
 *        G_c = (sum_s (F_x(s.x) F_y(s.y) F_z(s.z) w_c(s))^p)^(1/p),      ghat_c = G_c / sqrt(sum_c G_c^2),
 *        g_c(q) = sqrt((1 - alpha) w_c(q)^2 + alpha ghat_c^2).
 *   4. COMBINATION.  g_c = sqrt(sum_k weight_k g_c(q_k)^2) over the positions of step 2, or g = g(q) without divergence.
 *   5. OUTPUTS.  The columns of LFE channels are +0.  In float64, left to right, ONE rounding to float32:
 *        direct[i][c] = (float)(g_c * gain * sqrt(1 - diffuse)),   diffuse_out[i][c] = (float)(g_c * gain * sqrt(diffuse));
 *      a loudspeaker with g_c == 0 holds +0.
 * A row with no lock, v == 0 and s_max == 0 has the bits of earhip_allo_calculate[_device] on the same element.
 * The sum over the up to 8000 grid sources is never formed: group T's weight is a product of one function per coordinate
 * (the weight of c's plane, of c's row within the plane, of c within the row), and so is the fall-off, hence
 * G_c^p = Pz_c Py_c Px_c with Pk_c = sum_j (F_k(c_j) wk_c(c_j))^p: 60 terms per loudspeaker (csrc/allo_objects.h, the one core
 * of both forms, which also compiles without HIP).  The result is that of the triple sum up to rounding, and the bar of both
 * forms is one float32 spacing at max(|value|, 2^-20) against a float64 evaluation of the triple sum.
 *
 * ENTRY POINTS.  x, y, z and direct as in group T; every other input array may be NULL: width, height, depth 0, gain 1,
 * diffuse 0, channel_lock 0 (no lock), lock_max_distance +inf (none), divergence 0, position_range 0 (libear's
 * CartesianObjectDivergence default), excluded 0.  diffuse_out may be NULL only when diffuse is NULL.  n == 0 is a no-op;
 * n < 2^31.
 * earhip_allo_calculate_objects is a pure host function.  EARHIP_INVALID_ARGUMENT, the message naming the element's index: what
 * earhip_allo_calculate refuses; a size that is NaN, negative or infinite; a divergence that is NaN or outside [0, 1]; a
 * position_range that is NaN, negative or infinite; a lock_max_distance that is NaN or negative (each whether or not the lock
 * flag or the divergence makes use of it).  The rows before that index are written, its row and those after it are not.
 * earhip_allo_calculate_objects_device takes SoA device arrays of n elements (device-reachable host memory included); it runs
 * ONE kernel on the context's stream, allocates nothing, does not synchronise and never computes on the CPU.  An element the
 * host form would refuse gets NaN in every column of both rows and status 1 — except that mask bits at or beyond the channel
 * count are ignored — and every other element status 0 (status_dev: int[n], may be NULL).  The kernel's lanes run over
 * (object, loudspeaker): each lane finds its loudspeaker's neighbours under the object's mask in the by-value table and adds
 * its 60 terms, the normalisation is a sum in channel order through LDS, and rows leave through an LDS tile as contiguous
 * stores.  No atomics: the same input gives the same bits.
 * ---------------------------------------------------------------------- */
int earhip_allo_lock_priority(const earhip_allo *a, int *order);
int earhip_allo_calculate_objects(const earhip_allo *a, size_t n, const double *x, const double *y, const double *z,
                                  const double *width, const double *height, const double *depth, const double *gain,
                                  const double *diffuse, const unsigned char *channel_lock, const double *lock_max_distance,
                                  const double *divergence, const double *position_range, const uint32_t *excluded,
                                  float *direct, float *diffuse_out);
int earhip_allo_calculate_objects_device(earhip_ctx *ctx, const earhip_allo *a, size_t n, const double *x_dev,
                                         const double *y_dev, const double *z_dev, const double *width_dev,
                                         const double *height_dev, const double *depth_dev, const double *gain_dev,
                                         const double *diffuse_dev, const unsigned char *channel_lock_dev,
                                         const double *lock_max_distance_dev, const double *divergence_dev,
                                         const double *position_range_dev, const uint32_t *excluded_dev, float *direct_dev,
                                         float *diffuse_out_dev, int *status_dev);

/* ------------------------------------------------------------------------
 * (V) The screen of a CARTESIAN Objects block: screenRef scaling and screenEdgeLock on (x, y, z), the stage in front of groups T
 * and U that group R is in front of group I.  With it every Cartesian Objects block is rendered allocentrically: a block with
 * screenRef or a screenEdgeLock no longer has to take group K and the polar producer.  libear has no counterpart (it refuses
 * both everywhere).  THIS COMMENT IS THE SPECIFICATION, after BS.2127-0 7.3.3 and 7.3.4, which define both steps for a Cartesian
 * position as: to polar with section 10's point conversion, the polar step, back with the inverse point conversion.
 *
 * Screens, edges, the NULL rules of the three flag arrays (a NULL screen_ref means all 1, a NULL lock array all 0), the lock
 * codes, n < 2^31 and n == 0 are group R's.  Per element i:
 *   1. A NULL reproduction makes every element a bit-for-bit copy, and none is checked.
 *   2. An element with screen_ref[i] == 0 and both lock codes 0 is copied bit for bit, whatever it holds (NaN, infinity, -0.0;
 *      status 0).  Chaining groups K, R and K cannot give this: there every position takes two lossy conversions, and one that
 *      sits exactly on a loudspeaker plane of the cube (what groups T and U snap on) no longer does.
 *   3. Any other element is checked first: a non-finite coordinate or a lock code above 2 is refused.  The host form returns
 *      EARHIP_INVALID_ARGUMENT, the message naming the index; the elements before it are written, it and those after it are
 *      not.  The device form writes NaN to all three outputs and status[i] = EARHIP_INVALID_ARGUMENT (1, as group R).
 *   4. TO POLAR.  (az, el, d) = group K's point conversion of (x, y, z) (csrc/conversion.h).  A code it returns is the element's
 *      code on the host and its status, with NaN outputs, on the device, as in group K.
 *   5. SCALE AND LOCK.  Group R's steps 3 and 4 on (az, el) (csrc/screen.h); the conversion delivers az in [-180, 180] and el in
 *      [-90, 90].  d is not changed.
 *   6. BACK.  (x', y', z') = group K's point conversion of (az', el', d) to Cartesian, a code handled as in step 4.
 * Extent is not touched.  Each output may alias its own input (an element's three inputs are read before its outputs are
 * written), so the stage can run in place on the arrays groups T and U then read.  The origin stays the origin, and a position
 * on the z axis with |z| >= 1e-10 (below that the conversion calls it the origin) keeps its z and stays on the axis, unless a
 * vertical lock takes it off the pole.
 *
 * earhip_screen_apply_cartesian is a deliberate CPU computation on the calling thread, no context and no device.
 * earhip_screen_apply_cartesian_device takes the two screens in host memory and the arrays as device pointers
 * (device-reachable host memory included); it runs ONE kernel on the context's stream (one thread per element, 256 per block,
 * the six segments a by-value argument: 27 bytes read and 24 written per position, against 131 for the three launches),
 * allocates nothing, does not synchronise and never computes on the CPU.  Both forms call one core (csrc/screen_cart.h), which
 * calls the cores of groups K and R as they stand, and the library is built without contraction.  So on every element with a
 * flag set and no refusal THE HOST FORM HAS THE BITS OF earhip_conversion_to_polar, earhip_screen_apply,
 * earhip_conversion_to_cartesian CHAINED, AND THE DEVICE FORM THE BITS OF THEIR THREE DEVICE FORMS CHAINED.  Device against host
 * differs by what group K's libm calls differ on the two sides, nothing more.
 *
 * Out of scope: a screen stage for HOA, scaling of extent, fusing the stage into the kernels of groups T and
 * U, a polar-out form.
 * ---------------------------------------------------------------------- */
int earhip_screen_apply_cartesian(const earhip_screen *reference, const earhip_screen *reproduction, size_t n, const double *x,
                                  const double *y, const double *z, const unsigned char *screen_ref,
                                  const unsigned char *lock_horizontal, const unsigned char *lock_vertical, double *x_out,
                                  double *y_out, double *z_out);
int earhip_screen_apply_cartesian_device(earhip_ctx *ctx, const earhip_screen *reference, const earhip_screen *reproduction,
                                         size_t n, const double *x, const double *y, const double *z,
                                         const unsigned char *screen_ref, const unsigned char *lock_horizontal,
                                         const unsigned char *lock_vertical, double *x_out, double *y_out, double *z_out,
                                         int *status);

/* ------------------------------------------------------------------------
 * (W) The block timeline: from the timing of a track's audioBlockFormats (rtime, duration, jumpPosition, interpolationLength)
 * to the interpolation points of the renderer's curves (group F), the step between the gain producers (groups I, T, U, the
 * DirectSpeakers and HOA calculators) and earhip_render_set_object_points.  libear has no counterpart: its ObjectsTypeMetadata
 * carries no timing.  THIS COMMENT IS THE SPECIFICATION.  It follows the EBU ADM Renderer's reading of the block timing of
 * ITU-R BS.2127-0's Objects renderer; NO REFERENCE IMPLEMENTATION OF IT WAS AVAILABLE TO CHECK AGAINST, so what the tests hold
 * the code to is this comment, stated twice in exact arithmetic (tests/timeline_model.py: as a point list, and sample by sample).
 *
 * TIME.  Every time is a count of samples of the renderer's clock (earhip_render_reset).  Turning ADM time codes into samples
 * is the caller's job; take ceil(t * fs) for EVERY block boundary (a start, an end, the end of a ramp), so that a block covers
 * exactly the samples n with start <= n / fs < end, and two blocks that touch in time touch in samples.  `start` is the
 * track's offset (the audioObject's start), of any sign; s_b = start + rtime_b and e_b = s_b + duration_b are block b's first
 * sample and the first sample after it.  duration -1 is an open end (e_b is infinite), on the last block only.
 *
 * MODE.  EARHIP_TIMELINE_INTERPOLATED is the Objects rule: gains ramp from the previous block's.  EARHIP_TIMELINE_STEPPED is
 * for DirectSpeakers, HOA and any bed: no ramps, and jump_position and interpolation_length are not read at all.
 *
 * THE RULE.  A point is (time, src), src a block index — its row of gains — or -1, the all-zero row.  emit(t, src) appends a
 * point unless the last point has the same t and the same src.
 *
 *   prev = none
 *   for b in blocks, in order:
 *       if prev is none:   emit(s_b, -1); emit(s_b, b)               silence before; the first block is fixed from s_b on
 *       else:
 *           if s_b > e_prev:   emit(e_prev, -1); emit(s_b, -1)        a gap is silent
 *           if INTERPOLATED:   L = jump_position ? max(interpolation_length, 0) : duration_b
 *                              emit(s_b, prev); emit(s_b + L, b)      a ramp from the previous block's gains; L == 0 is a step
 *           else:              emit(s_b, b)                           STEPPED
 *       if duration_b != -1:   emit(e_b, b)
 *       prev = b; e_prev = e_b
 *   if the last duration != -1:   emit(e_prev, -1)                    silence after; an open end holds for ever
 *
 * The points have the semantics of GainInterpolator::interp_points (gain_interpolator.hpp:27-43): segment k covers the samples
 * [t_k-1, t_k) and runs linearly from point k-1 to point k, two points at one time are a step, the first value holds before
 * the first point and the last value after the last.  So:
 *   - block b owns the samples [s_b, e_b), and every sample no block owns is exactly +0.0 (no ramp into the first block, none
 *     out of the last, none across a gap: after a gap the ramp starts from the gains of the block before the gap);
 *   - sample n of a ramp is G_prev + (n - s_b) / L * (G_b - G_prev) in the renderer's own arithmetic, G_b is reached at s_b + L
 *     and held to e_b; without a jump the ramp takes the whole block and G_b itself is reached only at e_b, where the next
 *     block starts from it;
 *   - a list of n blocks makes at most 5 n + 1 points.
 *
 * REFUSALS, each EARHIP_INVALID_ARGUMENT with a message that names the block (the bulk setter: the track, then the block), and
 * always made on the WHOLE list, whatever the window: rtime < 0; duration == 0 or < -1; duration == -1 on a block that is not
 * the last; s_b < e_prev (blocks overlap or are out of order); an unknown mode; n_blocks < 1; a NULL blocks; and in
 * INTERPOLATED mode jump_position other than 0 or 1, with a jump an interpolation_length < -1 or an L > duration_b, and an
 * open-ended block that is not the first and has no jump (there is no duration to ramp over).  Also refused: start beyond
 * +-2^61, an rtime, duration or interpolation_length above 2^61 (no sum here leaves int64_t), and t0 >= t1.
 *
 * WINDOWS.  A curve holds at most 2^18 - 1 points, so a long programme with dense metadata is bound by time window.  For the
 * window [t0, t1) the selected blocks are [b0, b1]: b1 is the first block with e_b >= t1, or the last block if there is none;
 * b0 is the last block with s_b <= t0, or block 0 if there is none, and then one block earlier if that exists (its row is where
 * the ramp into the next block starts).  The rule runs on that sub-list as if it were the whole list; src keeps the indices
 * of the whole list.  ON EVERY SAMPLE OF [t0, t1) THE WINDOWED CURVE EQUALS THE WHOLE-LIST CURVE; outside it does not (the
 * sub-list's first block is not ramped into, and there is silence after its last).  t0 = INT64_MIN, t1 = INT64_MAX selects
 * everything.  The loop for a long programme: bind [t, t + W), commit, render the calls that fall into it, advance t by W.
 *
 * earhip_timeline_window and earhip_timeline_points are pure host functions, no context and no device.  earhip_timeline_points
 * writes at most `capacity` points and *n_points always; capacity == 0 only counts (times and source may then be NULL), any
 * other capacity below the count is EARHIP_INVALID_ARGUMENT.
 *
 * THE SETTERS bind the curves of a renderer (group F) from blocks and one row of gains per block: direct and diffuse are
 * [n_blocks][n_out] in BLOCK order, what the host form of a batch producer returns for the blocks in that order (the bulk form:
 * for the concatenated blocks of all tracks, track k's being block_offsets[k] .. block_offsets[k + 1], block_offsets[0] == 0).
 * Only rows of selected blocks are read: a caller may compute rows [first_block, last_block] of each track alone and leave
 * the rest unwritten.  diffuse is ignored (may be NULL) when n_buses == 1.  Each object's point rows — a block's row where src
 * is a block, +0.0 where it is -1 — are built in one buffer and go to the curve exactly as earhip_render_set_object_points
 * puts them there; rendering from these curves is bit for bit rendering from the same points set by hand.  The bulk form
 * checks every track before it changes any curve: a refused call leaves all curves as they were.  An object named twice gets
 * its last track.  earhip_render_commit stays the caller's call.  More than 2^18 - 1 points for one object is refused as in
 * earhip_render_set_object_points: bind a window instead.  As there, no segment may be longer than 2^31 - 1 samples: a block, a
 * ramp or a gap that long is refused.
 *
 * Out of scope: time codes and fractions of samples, clipping to the audioObject's duration, object gain, mute and
 * positionOffset (the caller scales rows), interpolating positions instead of gains, curves resident on the device.
 * ---------------------------------------------------------------------- */
typedef struct earhip_block_timing {
  int64_t rtime;                /* samples from the track's start, >= 0 */
  int64_t duration;             /* samples, >= 1; -1 = open end, allowed on the last block only */
  int64_t interpolation_length; /* samples; read only when jump_position != 0; -1 = not given (means 0) */
  int32_t jump_position;        /* 0 | 1 */
} earhip_block_timing;

enum { EARHIP_TIMELINE_INTERPOLATED = 0 /* Objects */, EARHIP_TIMELINE_STEPPED = 1 /* DirectSpeakers, HOA, any bed */ };

int earhip_timeline_window(int mode, int64_t start, int n_blocks, const earhip_block_timing *blocks,
                           int64_t t0, int64_t t1, int *first_block, int *last_block);
int earhip_timeline_points(int mode, int64_t start, int n_blocks, const earhip_block_timing *blocks, int64_t t0, int64_t t1,
                           int capacity, int64_t *times, int32_t *source, int *n_points);
int earhip_render_set_object_blocks(earhip_render *r, int object, int mode, int64_t start, int n_blocks,
                                    const earhip_block_timing *blocks, int64_t t0, int64_t t1,
                                    const float *direct, const float *diffuse);
int earhip_render_set_objects_blocks(earhip_render *r, int n_tracks, const int *objects, const int *modes, const int64_t *starts,
                                     const int64_t *block_offsets, const earhip_block_timing *blocks,
                                     int64_t t0, int64_t t1, const float *direct, const float *diffuse);

/* ------------------------------------------------------------------------
 * (X) DirectSpeakers with a CARTESIAN position or a screenEdgeLock: the two cases of ITU-R BS.2127-0 section 8 that the
 * calculator of group I (DirectSpeakers) refuses, as libear does, on that calculator's handle.  A file whose Objects are
 * Cartesian carries its bed the same way — channels with a CartesianSpeakerPosition, RC_L at (-1, 1, 0), RC_Lss at (-1, 0, 0),
 * RC_LFE with a lowPass, labels that are no BS.2051 labels — and with this group such a bed is placed by the library beside
 * the objects of groups T, U and V.  libear has no counterpart (it refuses both).  THIS COMMENT IS THE SPECIFICATION.  The lock
 * is BS.2127-0 7.3.4 as groups R and V state it.  THE CARTESIAN BOUNDS TEST AND THE FALL-THROUGH BY SECTION 10'S POINT
 * CONVERSION ARE THIS PROJECT'S READING of section 8, which words both for polar positions; no reference implementation of
 * either was available to check against, so what the tests hold the code to is this comment (tests/ds_cart_model.py).
 *
 * earhip_direct_speakers_calculate itself is unchanged: it still refuses both cases.
 *
 * INPUT.  md[i] is group I's earhip_ds_metadata.  Where md[i].cartesian is nonzero the position and its bounds are cart[i]
 * (x, y, z; a bound whose has_* flag is 0 is absent) and the polar fields of md[i] are not read; elsewhere cart[i] is not
 * read.  cart may be NULL when no md[i].cartesian is set.  In this entry point screen_edge_lock_horizontal / _vertical are
 * group R's lock CODES: horizontal 0 none, 1 left, 2 right; vertical 0 none, 1 bottom, 2 top.  reproduction is the
 * reproduction screen (group R's earhip_screen, checked as earhip_screen_edges checks it, whatever n is); NULL: no screen.
 * The reference screen of a lock is the default screen; a lock reads only the reproduction screen's edges.
 *
 * PER CHANNEL, in the order of group I.  A Cartesian element with cart == NULL is refused before anything else.
 *   1-4. Group I's steps 1 to 4 as they stand — the ADM check, the LFE decision and its two warnings, the refusal of
 *        AP_0001xxxx packs, nominal labels, the first label naming a layout channel of the same LFE type gets gain 1 — except
 *        that a Cartesian position is not refused.  A channel placed by a label never has its position, bounds or lock codes
 *        looked at.
 *   5a.  LOCK, in place of group I's refusal.  First the checks: a lock code above 2 is refused whatever the screen; a
 *        Cartesian element whose x, y or z is not finite, or which has a present bound that is not finite, is refused.  Then:
 *        - no reproduction screen: the position is unchanged;
 *        - polar: (azimuth, elevation) become what earhip_screen_apply gives for this element with screen_ref 0 and the two
 *          codes (csrc/screen.h on the map of the default screen's edges to the reproduction screen's, so the bits are group
 *          R's).  With no code set the position keeps its bits and is not checked.  With one set group R's checks apply: a
 *          non-finite azimuth or elevation, |azimuth| > 2^40 or |elevation| > 90 is refused.  The distance is untouched;
 *        - Cartesian: (x, y, z) become what earhip_screen_apply_cartesian gives for this element with screen_ref 0 and the
 *          two codes (csrc/screen_cart.h: to polar by group K's point conversion, the lock, back).  With no code set the
 *          position keeps its bits.  A code a conversion returns refuses the element.
 *        Bounds that are present stay as given; an absent bound is the position's value AFTER the lock.
 *   5b.  BOUNDS, polar: group I's step 5 on the locked position (nominal positions within the bounds, tolerance 1e-5, the pole
 *        clause; the nearest of several by the real positions).
 *        BOUNDS, Cartesian.  Loudspeaker c of the full layout stands at q_c = P(nominal azimuth, nominal elevation, 1) and
 *        its real position at r_c = P(real azimuth, real elevation, 1), P being group K's point conversion from polar to
 *        Cartesian (csrc/conversion.h; BS.2127-0 section 10).  Both tables are computed once at create, for BS.2051 layouts and
 *        defined layouts (group H) alike; no allocentric table (group T) enters, so a layout of the caller's own works.  In
 *        0+5+0 M+030 stands at (-1, 1, 0), M-030 at (1, 1, 0), M+110 at (-1, -1, 0), M-110 at (1, -1, 0), M+000 at (0, 1, 0).
 *        earhip_direct_speakers_cartesian_positions returns both tables, [n_channels][3] each.  c is a CANDIDATE when it has
 *        the channel's LFE type and
 *            q_c.x > x_min - 1e-5 && q_c.x < x_max + 1e-5,   and the same for y and z
 *        (double arithmetic as written; there is no pole clause).  One candidate gets gain 1.  Of several, with d_c the
 *        Euclidean distance sqrt((r_c.x - x)^2 + (r_c.y - y)^2 + (r_c.z - z)^2) from the locked position to r_c, the candidate
 *        of the smallest d_c gets gain 1 when |d_best - d_second| > 1e-5, d_second being the next smallest (equal to d_best
 *        when two candidates tie).  Otherwise, and with no candidate, the channel goes to step 6.
 *   6.   FALL-THROUGH.  An LFE channel goes to LFE1, or to silence in a layout without one.  Any other polar channel goes to
 *        the layout's point source panner at its locked (azimuth, elevation); any other Cartesian channel at the (azimuth,
 *        elevation) of group K's point conversion of the locked (x, y, z) to polar, which takes the origin (|x|, |y|, |z| all
 *        below 1e-10) to (0, 0, 0): panned straight ahead.  Every channel of the batch that reaches the panner, polar or
 *        Cartesian, goes to the device in the SAME single launch (real positions; LFE columns zero).
 *
 * REFUSALS.  EARHIP_INVALID_ARGUMENT, the message starting "metadata[i]: " when n > 1: cart == NULL with a Cartesian element;
 * a non-finite x, y, z or present bound; a lock code above 2; a polar position group R refuses under a lock; a conversion
 * that does not return EARHIP_OK (the message gives its code), which includes a calculator created with a loudspeaker
 * position group K's conversion refuses (|azimuth| > 2^40: every Cartesian element that reaches step 5a is then refused, and
 * so is earhip_direct_speakers_cartesian_positions; labelled and polar channels are served as ever); a Cartesian channel
 * whose conversion to polar gives an azimuth or elevation that is not finite (a guard in front of the launch: every finite
 * position tried, up to the largest double, converts to a finite direction and is panned); a handle created with ctx == NULL and a non-LFE channel that
 * reaches the panner.  EARHIP_ADM_ERROR and EARHIP_NOT_IMPLEMENTED (AP_0001xxxx) are group I's.  warnings_out is group I's:
 * [n][2], and on an error the rows up to and including the failing channel hold what was raised before it.
 *
 * PROMISES.  A batch with no Cartesian element and no lock code returns the bits of earhip_direct_speakers_calculate, gains
 * and warnings, its status and message on an error too, with or without a screen.  A batch equals its channels computed one
 * at a time.  Without a reproduction screen a lock code (0, 1 or 2) changes nothing.
 *
 * The work is host logic over a few dozen loudspeakers plus group I's panner launch: there is no new kernel, and no rate was
 * measured.  Out of scope: the common-definitions mapping rules (as in group I), a reference screen other than the default.
 * ---------------------------------------------------------------------- */
/* the Cartesian position of one channel; read only where md[i].cartesian != 0 */
typedef struct earhip_ds_cartesian {
  double x, y, z;
  int has_x_min, has_x_max, has_y_min, has_y_max, has_z_min, has_z_max;
  double x_min, x_max, y_min, y_max, z_min, z_max;
} earhip_ds_cartesian;

int earhip_direct_speakers_calculate_screen(earhip_direct_speakers *ds,
                                            const earhip_screen *reproduction, /* NULL: no screen, locks are the identity */
                                            size_t n, const earhip_ds_metadata *md,
                                            const earhip_ds_cartesian *cart,   /* [n], or NULL when no md[i].cartesian is set */
                                            float *gains, int *warnings_out);

/* the loudspeakers as the Cartesian bounds test and the nearest-candidate rule see them: [n_channels][3] each */
int earhip_direct_speakers_cartesian_positions(const earhip_direct_speakers *ds, double *nominal_xyz, double *real_xyz);

#ifdef __cplusplus
}
#endif
#endif /* EARHIP_H */
