// oracle/ref_interp_capi.cpp — C entry points over the REFERENCE's own
// include/ear/dsp/gain_interpolator.hpp (compiled in place with
// -I$(REF)/include, never copied).  Builds into oracle/_ref/libref_interp.so
// (git-ignored).  The header is header-only; its include chain ends at the
// CMake product generated/export.hpp, for which the Makefile writes a
// stand-in under oracle/_ref/include/ (EAR_EXPORT, EAR_NO_EXPORT: empty).
//
// Used only to check the oracle's GainInterpolator restatement and the HIP gain
// stage against libear, and to generate tests/golden/gain_interp_ref.npz (see
// tests/golden/make_interp_golden.py).  The interpolation is libear's; the
// objects gain stage below (one GainInterpolator<LinearInterpVector> per object,
// outputs summed into the bus in object order) is this project's composition,
// the one ear_oracle.hpp:ObjectsRenderer restates.
//
// Layouts: audio is planar, channel c at base + c * stride.  Points are dense
// [npoints][n_in][n_out] (LinearInterpMatrix's [in][out]).
#include <cstddef>
#include <cstdint>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "ear/dsp/gain_interpolator.hpp"

using ear::dsp::GainInterpolator;
using ear::dsp::LinearInterpMatrix;
using ear::dsp::LinearInterpSingle;
using ear::dsp::LinearInterpVector;
using ear::dsp::SampleIndex;

namespace {
std::string g_err;

template <typename F>
int guarded(F &&f) {
  try {
    f();
    return 0;
  } catch (const std::exception &e) {
    g_err = e.what();
    return 1;
  }
}

std::vector<const float *> chans(const float *base, size_t n, size_t stride) {
  std::vector<const float *> p(n);
  for (size_t c = 0; c < n; c++) p[c] = base + c * stride;
  return p;
}
std::vector<float *> chans(float *base, size_t n, size_t stride) {
  std::vector<float *> p(n);
  for (size_t c = 0; c < n; c++) p[c] = base + c * stride;
  return p;
}

LinearInterpVector::Point vec_point(const float *v, int n_out) {
  return LinearInterpVector::Point(v, v + n_out);
}
LinearInterpMatrix::Point mat_point(const float *v, int n_in, int n_out) {
  LinearInterpMatrix::Point p(n_in);
  for (int m = 0; m < n_in; m++) p[m].assign(v + (size_t)m * n_out, v + (size_t)(m + 1) * n_out);
  return p;
}

// kind 0: LinearInterpSingle, 1: LinearInterpVector, 2: LinearInterpMatrix
template <typename Interp>
struct PointOf;
template <>
struct PointOf<LinearInterpSingle> {
  static float make(const float *v, int, int) { return v[0]; }
};
template <>
struct PointOf<LinearInterpVector> {
  static LinearInterpVector::Point make(const float *v, int, int n_out) { return vec_point(v, n_out); }
};
template <>
struct PointOf<LinearInterpMatrix> {
  static LinearInterpMatrix::Point make(const float *v, int n_in, int n_out) { return mat_point(v, n_in, n_out); }
};

// libear reads interp_points[-1] when there are none (gain_interpolator.hpp: process); the
// oracle and the HIP path define that as an error, and so does this shim
template <typename Interp>
void require_points(const GainInterpolator<Interp> &gi) {
  if (gi.interp_points.empty()) throw std::invalid_argument("interp_points must not be empty");
}

template <typename Interp>
void set_points(GainInterpolator<Interp> &gi, int n_in, int n_out, int npoints, const int64_t *times,
                const float *values) {
  const size_t psz = (size_t)n_in * n_out;
  gi.interp_points.clear();
  for (int p = 0; p < npoints; p++)
    gi.interp_points.emplace_back((SampleIndex)times[p], PointOf<Interp>::make(values + p * psz, n_in, n_out));
}

template <typename Interp>
void policy(int interp, int n_in, int n_out, const float *in, float *out, size_t stride, int64_t r0, int64_t r1,
            int64_t block_start, int64_t start, int64_t end, const float *sp, const float *ep) {
  auto ip = chans(in, n_in, stride);
  auto op = chans(out, n_out, stride);
  if (interp)
    Interp::apply_interp(ip.data(), op.data(), r0, r1, block_start, start, end,
                         PointOf<Interp>::make(sp, n_in, n_out), PointOf<Interp>::make(ep, n_in, n_out));
  else
    Interp::apply_constant(ip.data(), op.data(), r0, r1, PointOf<Interp>::make(sp, n_in, n_out));
}

template <typename Interp>
void fresh_run(int n_in, int n_out, int npoints, const int64_t *times, const float *values, int64_t t0,
               const size_t *call_sizes, int ncalls, const float *in, float *out) {
  GainInterpolator<Interp> gi;
  set_points(gi, n_in, n_out, npoints, times, values);
  require_points(gi);
  size_t total = 0;
  for (int k = 0; k < ncalls; k++) total += call_sizes[k];
  size_t ofs = 0;
  for (int k = 0; k < ncalls; k++) {
    auto ip = chans(in + ofs, n_in, total);
    auto op = chans(out + ofs, n_out, total);
    gi.process((SampleIndex)(t0 + (int64_t)ofs), call_sizes[k], ip.data(), op.data());
    ofs += call_sizes[k];
  }
}

// the objects gain stage: one GainInterpolator<LinearInterpVector> per object
struct Objects {
  int M, N;
  std::vector<GainInterpolator<LinearInterpVector>> gi;
  std::vector<float> tmp;
};
}  // namespace

extern "C" {
const char *ref_interp_last_error() { return g_err.c_str(); }

// LinearInterp{Single,Vector,Matrix}::apply_interp (interp = 1) or ::apply_constant
// (interp = 0, point = sp): in [n_in][stride], out [n_out][stride]
int ref_interp_policy(int kind, int interp, int n_in, int n_out, const float *in, float *out, size_t stride,
                      int64_t range_start, int64_t range_end, int64_t block_start, int64_t start, int64_t end,
                      const float *sp, const float *ep) {
  return guarded([&] {
    if (kind == 0)
      policy<LinearInterpSingle>(interp, n_in, n_out, in, out, stride, range_start, range_end, block_start, start,
                                 end, sp, ep);
    else if (kind == 1)
      policy<LinearInterpVector>(interp, n_in, n_out, in, out, stride, range_start, range_end, block_start, start,
                                 end, sp, ep);
    else
      policy<LinearInterpMatrix>(interp, n_in, n_out, in, out, stride, range_start, range_end, block_start, start,
                                 end, sp, ep);
  });
}

// A fresh GainInterpolator<kind> over consecutive calls of call_sizes samples from
// sample t0 — the signature of oracle_gain_interp (oracle/oracle_capi.cpp)
int ref_gain_interp(int kind, int n_in, int n_out, int npoints, const int64_t *times, const float *values,
                    int64_t t0, const size_t *call_sizes, int ncalls, const float *in, float *out) {
  return guarded([&] {
    if (kind == 0)
      fresh_run<LinearInterpSingle>(n_in, n_out, npoints, times, values, t0, call_sizes, ncalls, in, out);
    else if (kind == 1)
      fresh_run<LinearInterpVector>(n_in, n_out, npoints, times, values, t0, call_sizes, ncalls, in, out);
    else
      fresh_run<LinearInterpMatrix>(n_in, n_out, npoints, times, values, t0, call_sizes, ncalls, in, out);
  });
}

// A GainInterpolator<LinearInterpMatrix> that lives across calls (its search
// cache included); interp_points may be replaced between calls.
void *ref_gi_create() { return new GainInterpolator<LinearInterpMatrix>(); }
void ref_gi_destroy(void *h) { delete static_cast<GainInterpolator<LinearInterpMatrix> *>(h); }
int ref_gi_set_points(void *h, int n_in, int n_out, int npoints, const int64_t *times, const float *values) {
  return guarded([&] {
    set_points(*static_cast<GainInterpolator<LinearInterpMatrix> *>(h), n_in, n_out, npoints, times, values);
  });
}
// in [n_in][in_stride], out [n_out][out_stride]
int ref_gi_process(void *h, int n_in, int n_out, int64_t block_start, size_t nsamples, const float *in,
                   size_t in_stride, float *out, size_t out_stride) {
  return guarded([&] {
    require_points(*static_cast<GainInterpolator<LinearInterpMatrix> *>(h));
    auto ip = chans(in, n_in, in_stride);
    auto op = chans(out, n_out, out_stride);
    static_cast<GainInterpolator<LinearInterpMatrix> *>(h)->process((SampleIndex)block_start, nsamples, ip.data(),
                                                                   op.data());
  });
}

// The objects gain stage (one bus): M objects -> N outputs
void *ref_objects_create(int n_objects, int n_out) {
  Objects *o = new Objects;
  o->M = n_objects, o->N = n_out;
  o->gi.resize(n_objects);
  return o;
}
void ref_objects_destroy(void *h) { delete static_cast<Objects *>(h); }
// gains [npoints][n_out]
int ref_objects_set_points(void *h, int object, int npoints, const int64_t *times, const float *gains) {
  return guarded([&] {
    Objects *o = static_cast<Objects *>(h);
    set_points(o->gi.at(object), 1, o->N, npoints, times, gains);
  });
}
// in [M][nsamples], bus [N][nsamples] (overwritten): bus = sum over objects, in object order
int ref_objects_process(void *h, int64_t block_start, size_t nsamples, const float *in, float *bus) {
  return guarded([&] {
    Objects *o = static_cast<Objects *>(h);
    for (const auto &gi : o->gi) require_points(gi);
    o->tmp.assign((size_t)o->N * nsamples, 0.0f);
    for (size_t i = 0; i < (size_t)o->N * nsamples; i++) bus[i] = 0.0f;
    auto tp = chans(o->tmp.data(), o->N, nsamples);
    for (int m = 0; m < o->M; m++) {
      const float *ip = in + (size_t)m * nsamples;
      o->gi[m].process((SampleIndex)block_start, nsamples, &ip, tp.data());
      for (size_t i = 0; i < (size_t)o->N * nsamples; i++) bus[i] += o->tmp[i];
    }
  });
}
}  // extern "C"
