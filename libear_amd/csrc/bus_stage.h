// bus_stage.h — what a stage of the output bus is: the base of the six opaque handles (loudness meter, FIR
// matrix, limiter, biquad matrix, sample-rate converter, delay matrix), and what their entry points share: the checks of a call
// in one order, the host form's staging, the two-halves state, destroy and reset.  Host code only.
#pragma once

#include <memory>

#include "common.h"
#include "launch_cuts.h"

namespace earhip {

// A stage's own words for the calls the shared checks refuse.
struct StageWords {
  const char *handle;                 // the handle is NULL
  const char *in_dev, *out_dev;       // device form: a NULL pointer, ...
  const char *in_stride, *out_stride; // ... a stride shorter than the call
  const char *in_rows, *out_rows;     // host form: the array of row pointers is NULL, ...
  const char *in_row, *out_row;       // ... a row that is read or written is NULL
};

struct BusStage {
  earhip_ctx *ctx = nullptr;
  int n_in = 0, n_out = 0;
  int block = 1;              // samples per unit of a call: 1, or the FIR matrix's block size
  const char *noun = "";      // "limiter", "FIR matrix": the stage in the messages of whoever holds it as a BusStage
  size_t room = 0;            // the most units one call may bring ...
  const char *room_name = ""; // ... under the name it has in the stage's config ("max_samples")
  virtual ~BusStage() = default;
  // back to the state after create (enqueues on the context's stream)
  virtual void zero() = 0;
  // throws EARHIP_INVALID_ARGUMENT when a call of `units` does not fit; consumes nothing
  virtual void check_room(size_t units) const {
    if (units > room) fail_invalid(std::string("the call would pass the ") + noun + "'s " + room_name + " (nothing was consumed)");
  }
  // the stage's kernels over planar device rows on the context's stream, the call cut into launches; the caller has checked the
  // room and the strides.  (A stage that only reads ignores out.)
  virtual void feed(size_t units, const float *in, size_t in_stride, float *out, size_t out_stride) = 0;
};

// A handle as its base, for whoever holds it opaque (the renderer's taps): a specialisation per stage that can be attached,
// declared here, in front of every use, and defined in the stage's file, where the handle is a complete type.
template <typename H>
BusStage *as_stage(H *h);
template <>
BusStage *as_stage<earhip_loudness>(earhip_loudness *h);
template <>
BusStage *as_stage<earhip_firmix>(earhip_firmix *h);
template <>
BusStage *as_stage<earhip_limiter>(earhip_limiter *h);

// Device state in two halves (launch_cuts.h): in() is read by a launch, out() written, flip() behind it.
template <typename T>
struct PingPong {
  DevBuf<T> buf;  // [2][half]
  Halves at;
  void alloc(size_t half) {
    buf.alloc(2 * half);
    at = Halves{half, 0};
  }
  void rewind() { at.par = 0; }
  void zero(hipStream_t s) {
    EARHIP_HIP(hipMemsetAsync(buf.p, 0, sizeof(T) * buf.n, s));
    rewind();
  }
  T *in() const { return buf.p + at.in(); }
  T *out() const { return buf.p + at.out(); }
  void flip() { at.flip(); }
};

// The host form's staging: the rows of a call go through one pinned buffer, one transfer each way.
struct HostRows {
  DevBuf<float> d_in, d_out;  // [rows in][the longest call], [rows out][the longest call's outputs]
  PinBuf<float> pin;
  void alloc(size_t in_elems, size_t out_elems) {
    d_in.alloc(in_elems);
    d_out.alloc(out_elems);
    pin.reserve(std::max(in_elems, out_elems));
  }
  // C rows of n samples to d_in [C][n].  A row that read(c) denies is not looked at: its staging keeps whatever it held, and no
  // kernel reads it.
  template <typename Read>
  void to_device(const float *const *rows, int C, size_t n, hipStream_t s, Read &&read) {
    for (int c = 0; c < C; c++)
      if (read(c)) std::copy(rows[c], rows[c] + n, pin.p + (size_t)c * n);
    EARHIP_HIP(hipMemcpyAsync(d_in.p, pin.p, sizeof(float) * n * (size_t)C, hipMemcpyHostToDevice, s));
  }
  // d_out [C][n] to C rows of n samples, behind everything enqueued on s (waits)
  void from_device(float *const *rows, int C, size_t n, hipStream_t s) {
    if (n > 0) EARHIP_HIP(hipMemcpyAsync(pin.p, d_out.p, sizeof(float) * n * (size_t)C, hipMemcpyDeviceToHost, s));
    EARHIP_HIP(hipStreamSynchronize(s));
    for (int c = 0; c < C; c++) std::copy(pin.p + (size_t)c * n, pin.p + (size_t)(c + 1) * n, rows[c]);
  }
};

inline bool reads_every_row(int) { return true; }

// ---- the checks of a call: handle, room, nothing to do, pointers, strides — nothing behind them refuses a call -------------

// false: the call is empty (and fits)
template <typename H>
bool stage_admits(const H *h, size_t units) {
  require(h != nullptr, H::words.handle);
  h->check_room(units);
  return units != 0;
}
// a side of 0 samples brings no pointer
inline void check_device_rows(const StageWords &w, size_t n_in, const void *in, size_t in_stride, size_t n_out, const void *out,
                              size_t out_stride) {
  require(n_in == 0 || in != nullptr, w.in_dev);
  require(n_out == 0 || out != nullptr, w.out_dev);
  require(in_stride >= n_in, w.in_stride);
  require(out_stride >= n_out, w.out_stride);
}
template <typename Read>
void check_host_rows(const StageWords &w, size_t n_in, const float *const *in, int C_in, Read &&read, size_t n_out,
                     float *const *out, int C_out) {
  require(n_in == 0 || in != nullptr, w.in_rows);
  require(n_out == 0 || out != nullptr, w.out_rows);
  for (int c = 0; n_in && c < C_in; c++) require(!read(c) || in[c] != nullptr, w.in_row);
  for (int c = 0; n_out && c < C_out; c++) require(out[c] != nullptr, w.out_row);
}

// ---- the entry points a stage has as they are ----------------------------------------------------------------------------

template <typename H>
void stage_process_device(H *h, size_t units, const float *in, size_t in_stride, float *out, size_t out_stride) {
  if (!stage_admits(h, units)) return;
  const size_t n = units * (size_t)h->block;
  check_device_rows(H::words, n, in, in_stride, n, out, out_stride);
  h->ctx->use();
  h->feed(units, in, in_stride, out, out_stride);
}

// through h->host (HostRows); read(c): input row c is read
template <typename H, typename Read>
void stage_process_host(H *h, size_t units, const float *const *in, float *const *out, Read &&read) {
  if (!stage_admits(h, units)) return;
  const size_t n = units * (size_t)h->block;
  check_host_rows(H::words, n, in, h->n_in, read, n, out, h->n_out);
  h->ctx->use();
  h->host.to_device(in, h->n_in, n, h->ctx->stream, read);
  h->feed(units, h->host.d_in.p, n, h->host.d_out.p, n);
  h->host.from_device(out, h->n_out, n, h->ctx->stream);
}

// the end of a create function: the state zeroed, the uploads and the zeroing done, the handle the caller's
template <typename H>
void stage_ready(std::unique_ptr<H> &h, H **out) {
  h->zero();
  EARHIP_HIP(hipStreamSynchronize(h->ctx->stream));
  *out = h.release();
}

template <typename H>
int stage_destroy(H *h) {
  return guarded([&] {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
  });
}

template <typename H>
int stage_reset(H *h) {
  return guarded([&] {
    require(h != nullptr, H::words.handle);
    h->ctx->use();
    h->zero();
  });
}

}  // namespace earhip
