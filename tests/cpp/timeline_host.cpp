// timeline_host.cpp — libear_amd/csrc/timeline.h (include/earhip.h group W) as a plain C++ program on the CPU, compiled by g++
// alone under ASan and UBSan and run directly by tests/test_timeline_host_cpu.py, which writes the cases and holds the answers
// to tests/timeline_model.py.
//
//   timeline_host points <in> <out>   cases of (mode, n_blocks, start, t0, t1, blocks): check, window, count, then the points
//                                     into arrays of exactly that size
//   timeline_host bind <in> <out>     one timeline_bind call (what earhip_render_set_objects_blocks does) against a sink that
//                                     records every set_object call
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../libear_amd/csrc/timeline.h"

using namespace earhip;

static std::vector<unsigned char> read_file(const char *path) {
  std::vector<unsigned char> data;
  FILE *f = std::fopen(path, "rb");
  if (!f) return data;
  unsigned char buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
  std::fclose(f);
  return data;
}

struct Reader {
  const std::vector<unsigned char> &data;
  size_t at = 0;
  bool bad = false;
  template <typename T>
  T one() {
    T v = T();
    many(&v, 1);
    return v;
  }
  template <typename T>
  void many(T *out, size_t n) {
    if (n > (data.size() - at) / sizeof(T)) {
      bad = true;
      return;
    }
    if (n) std::memcpy(out, data.data() + at, n * sizeof(T));
    at += n * sizeof(T);
  }
  template <typename T>
  std::vector<T> vec(size_t n) {
    std::vector<T> v(bad || n > data.size() ? 0 : n);
    many(v.data(), v.size());
    return v;
  }
};

struct Writer {
  std::vector<unsigned char> data;
  template <typename T>
  void one(T v) { many(&v, 1); }
  template <typename T>
  void many(const T *p, size_t n) {
    const unsigned char *b = reinterpret_cast<const unsigned char *>(p);
    if (n) data.insert(data.end(), b, b + n * sizeof(T));
  }
  void text(const std::string &s) {
    one<int32_t>((int32_t)s.size());
    many(s.data(), s.size());
  }
  bool save(const char *path) const {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(data.data(), 1, data.size(), f) == data.size();
    return std::fclose(f) == 0 && ok;
  }
};

static int run_points(Reader &in, Writer &out) {
  const int32_t n_cases = in.one<int32_t>();
  for (int32_t c = 0; c < n_cases && !in.bad; c++) {
    const int32_t mode = in.one<int32_t>(), n_blocks = in.one<int32_t>();
    const int64_t start = in.one<int64_t>(), t0 = in.one<int64_t>(), t1 = in.one<int64_t>();
    const std::vector<earhip_block_timing> blocks = in.vec<earhip_block_timing>(n_blocks > 0 ? n_blocks : 0);
    if (in.bad) break;
    try {
      // (an empty list still gets a non-NULL pointer: the refusal under test is n_blocks < 1)
      static const earhip_block_timing none = {0, 0, 0, 0};
      const earhip_block_timing *b = blocks.empty() ? &none : blocks.data();
      timeline_check(mode, start, n_blocks, b);
      int b0 = -1, b1 = -1;
      timeline_window(start, n_blocks, b, t0, t1, &b0, &b1);
      const int64_t n = timeline_emit(mode, start, b, b0, b1, 0, nullptr, nullptr);
      std::vector<int64_t> times((size_t)n);  // exactly n: one point too many is a heap overflow ASan reports
      std::vector<int32_t> source((size_t)n);
      if (timeline_emit(mode, start, b, b0, b1, n, times.data(), source.data()) != n) return 3;
      out.one<int32_t>(0), out.one<int32_t>(b0), out.one<int32_t>(b1), out.one<int32_t>((int32_t)n);
      out.many(times.data(), times.size()), out.many(source.data(), source.size());
    } catch (const TimelineFailure &f) {
      out.one<int32_t>(EARHIP_INVALID_ARGUMENT), out.text(f.msg);
    }
  }
  return in.bad ? 2 : 0;
}

static int run_bind(Reader &in, Writer &out) {
  const int32_t n_objects = in.one<int32_t>(), n_out = in.one<int32_t>(), n_buses = in.one<int32_t>(), max_points = in.one<int32_t>();
  const int32_t n_tracks = in.one<int32_t>();
  if (in.bad || n_tracks < 0 || n_out < 1) return 2;
  const std::vector<int32_t> objects = in.vec<int32_t>(n_tracks), modes = in.vec<int32_t>(n_tracks);
  const std::vector<int64_t> starts = in.vec<int64_t>(n_tracks), offsets = in.vec<int64_t>((size_t)n_tracks + 1);
  const int64_t t0 = in.one<int64_t>(), t1 = in.one<int64_t>();
  const int64_t total = in.one<int64_t>();  // blocks and rows given (the offsets may be wrong on purpose)
  if (in.bad || total < 0) return 2;
  const std::vector<earhip_block_timing> blocks = in.vec<earhip_block_timing>((size_t)total);
  const std::vector<float> direct = in.vec<float>((size_t)total * n_out);
  const std::vector<float> diffuse = in.vec<float>(n_buses == 2 ? (size_t)total * n_out : 0);
  if (in.bad) return 2;
  const std::vector<int> obj(objects.begin(), objects.end()), md(modes.begin(), modes.end());
  Writer calls;
  int32_t n_calls = 0;
  const size_t cols = (size_t)n_buses * n_out;
  try {
    timeline_bind(n_objects, n_out, n_buses, max_points, n_tracks, obj.data(), md.data(), starts.data(), offsets.data(), blocks.data(),
                  t0, t1, direct.data(), n_buses == 2 ? diffuse.data() : nullptr,
                  [&](int object, int npoints, const int64_t *times, const float *rows) {
                    n_calls++;
                    calls.one<int32_t>(object), calls.one<int32_t>(npoints);
                    calls.many(times, (size_t)npoints), calls.many(rows, (size_t)npoints * cols);
                  });
    out.one<int32_t>(0), out.text("");
  } catch (const TimelineFailure &f) {
    out.one<int32_t>(EARHIP_INVALID_ARGUMENT), out.text(f.msg);
  }
  out.one<int32_t>(n_calls);
  out.many(calls.data.data(), calls.data.size());
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 4) return 64;
  const std::vector<unsigned char> data = read_file(argv[2]);
  Reader in{data};
  Writer out;
  int rc = 64;
  if (std::strcmp(argv[1], "points") == 0) rc = run_points(in, out);
  if (std::strcmp(argv[1], "bind") == 0) rc = run_bind(in, out);
  if (rc != 0) return rc;
  return out.save(argv[3]) ? 0 : 5;
}
