// timeline.h — the block timeline (include/earhip.h group W, where the rule is specified): from the timing of a track's
// audioBlockFormats to the interpolation points of the renderer's curves, as plain C++ that the C ABI (api_render.hip) and a
// plain C++ program on the CPU (tests/cpp/timeline_host.cpp) both compile, as panner.h and extent.h are.  No HIP header is
// needed to include it.  Integer logic and row copies on the host: there is no device work here.
//
// Three layers, each usable alone:
//   timeline_check   every refusal of group W on a whole block list (a TimelineFailure naming the block)
//   timeline_window  the blocks [b0, b1] a window [t0, t1) needs;  timeline_emit: the rule on blocks [b0, b1]
//   timeline_bind    what earhip_render_set_object[s]_blocks do: every track checked and its points made before the first
//                    curve changes, then each object's point rows built in one buffer and handed to set_object
#pragma once
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/earhip.h"

namespace earhip {

struct TimelineFailure {
  std::string msg;
};
[[noreturn]] inline void timeline_fail(const std::string &m) { throw TimelineFailure{m}; }

// start, rtime, duration and interpolation_length stay within this, so that no sum of three of them leaves int64_t
constexpr int64_t kTimelineMaxTime = (int64_t)1 << 61;

inline bool timeline_mode_known(int mode) { return mode == EARHIP_TIMELINE_INTERPOLATED || mode == EARHIP_TIMELINE_STEPPED; }

// the ramp length of block b (INTERPOLATED, b not the first of its list)
inline int64_t timeline_ramp(const earhip_block_timing &k) {
  if (k.jump_position) return k.interpolation_length > 0 ? k.interpolation_length : 0;
  return k.duration;
}

inline void timeline_check(int mode, int64_t start, int n_blocks, const earhip_block_timing *blocks) {
  if (!timeline_mode_known(mode)) timeline_fail("unknown timeline mode " + std::to_string(mode));
  if (n_blocks < 1) timeline_fail("n_blocks must be >= 1");
  if (blocks == nullptr) timeline_fail("blocks must not be NULL");
  if (start < -kTimelineMaxTime || start > kTimelineMaxTime) timeline_fail("start must be within +-2^61 samples");
  int64_t e_prev = 0;
  for (int b = 0; b < n_blocks; b++) {
    const earhip_block_timing &k = blocks[b];
    const std::string at = "block " + std::to_string(b) + ": ";
    if (k.rtime < 0) timeline_fail(at + "rtime must be >= 0");
    if (k.duration == 0 || k.duration < -1) timeline_fail(at + "duration must be >= 1, or -1 for an open end");
    if (k.rtime > kTimelineMaxTime || k.duration > kTimelineMaxTime) timeline_fail(at + "rtime and duration must be within 2^61 samples");
    if (k.duration == -1 && b != n_blocks - 1) timeline_fail(at + "only the last block may have an open end (duration -1)");
    const int64_t s = start + k.rtime;
    if (b > 0 && s < e_prev) timeline_fail(at + "starts before the previous block ends (blocks overlap or are out of order)");
    if (mode == EARHIP_TIMELINE_INTERPOLATED) {
      if (k.jump_position != 0 && k.jump_position != 1) timeline_fail(at + "jump_position must be 0 or 1");
      if (k.jump_position) {
        if (k.interpolation_length < -1) timeline_fail(at + "interpolation_length must be >= 0, or -1 for not given");
        if (k.interpolation_length > kTimelineMaxTime) timeline_fail(at + "interpolation_length must be within 2^61 samples");
        if (k.duration != -1 && timeline_ramp(k) > k.duration) timeline_fail(at + "interpolation_length is longer than the block");
      } else if (k.duration == -1 && b > 0) {
        timeline_fail(at + "an open-ended block after another needs jump_position (there is no duration to ramp over)");
      }
    }
    e_prev = s + (k.duration == -1 ? 0 : k.duration);
  }
}

// [b0, b1] of a checked list for the window [t0, t1)
inline void timeline_window(int64_t start, int n_blocks, const earhip_block_timing *blocks, int64_t t0, int64_t t1, int *b0, int *b1) {
  if (!(t0 < t1)) timeline_fail("the window needs t0 < t1");
  int last = n_blocks - 1;
  for (int b = 0; b < n_blocks; b++) {
    const int64_t e = blocks[b].duration == -1 ? std::numeric_limits<int64_t>::max() : start + blocks[b].rtime + blocks[b].duration;
    if (e >= t1) {
      last = b;
      break;
    }
  }
  int first = 0;
  for (int b = 1; b < n_blocks && start + blocks[b].rtime <= t0; b++) first = b;
  if (first > 0) first--;  // its row is where the ramp into the next block starts
  *b0 = first, *b1 = last;
}

// The rule on blocks [b0, b1] of a checked list, as if they were the whole list; source keeps the indices of the whole
// list.  Points beyond `capacity` are counted and not written.  Returns the number of points.
inline int64_t timeline_emit(int mode, int64_t start, const earhip_block_timing *blocks, int b0, int b1, int64_t capacity,
                             int64_t *times, int32_t *source) {
  int64_t n = 0, last_t = 0;
  int32_t last_src = 0;
  auto emit = [&](int64_t t, int32_t src) {
    if (n > 0 && last_t == t && last_src == src) return;
    if (n < capacity) times[n] = t, source[n] = src;
    n++, last_t = t, last_src = src;
  };
  int64_t e_prev = 0;
  for (int b = b0; b <= b1; b++) {
    const earhip_block_timing &k = blocks[b];
    const int64_t s = start + k.rtime;
    if (b == b0) {
      emit(s, -1), emit(s, b);
    } else {
      if (s > e_prev) emit(e_prev, -1), emit(s, -1);
      if (mode == EARHIP_TIMELINE_INTERPOLATED)
        emit(s, b - 1), emit(s + timeline_ramp(k), b);
      else
        emit(s, b);
    }
    if (k.duration != -1) emit(s + k.duration, b);
    e_prev = s + k.duration;
  }
  if (blocks[b1].duration != -1) emit(e_prev, -1);
  return n;
}

// earhip_render_set_objects_blocks without the renderer: n_objects, n_out, n_buses and max_points are its, set_object(object,
// npoints, times, rows[npoints][n_buses * n_out]) is CurveSet::set_object.  Nothing is set before every track has passed
// every check, the two that set_object would make on the points included (their number, and no segment beyond 2^31 - 1
// samples).  direct / diffuse: [block_offsets[n_tracks]][n_out], of which only rows of selected blocks are read.
template <typename SetObject>
void timeline_bind(int n_objects, int n_out, int n_buses, int max_points, int n_tracks, const int *objects, const int *modes,
                   const int64_t *starts, const int64_t *block_offsets, const earhip_block_timing *blocks, int64_t t0, int64_t t1,
                   const float *direct, const float *diffuse, SetObject &&set_object) {
  if (n_tracks < 1) timeline_fail("n_tracks must be >= 1");
  if (!objects || !modes || !starts || !block_offsets || !blocks || !direct) timeline_fail("NULL argument");
  if (n_buses == 2 && !diffuse) timeline_fail("diffuse gains must not be NULL when n_buses == 2");
  std::vector<int64_t> times;
  std::vector<int32_t> source;
  std::vector<size_t> first(n_tracks + 1, 0);
  size_t most = 0;
  for (int k = 0; k < n_tracks; k++) {
    const std::string at = "track " + std::to_string(k) + ": ";
    try {
      if (objects[k] < 0 || objects[k] >= n_objects) timeline_fail("object index out of range");
      const int64_t nb = block_offsets[k + 1] - block_offsets[k];
      if (block_offsets[k] < 0 || (k == 0 && block_offsets[0] != 0) || nb > std::numeric_limits<int>::max())
        timeline_fail("block_offsets must ascend from 0 in steps of at most 2^31 - 1");
      const earhip_block_timing *tb = blocks + block_offsets[k];
      timeline_check(modes[k], starts[k], nb < 1 ? 0 : (int)nb, tb);
      int b0, b1;
      timeline_window(starts[k], (int)nb, tb, t0, t1, &b0, &b1);
      const int64_t n = timeline_emit(modes[k], starts[k], tb, b0, b1, 0, nullptr, nullptr);
      if (n > max_points) timeline_fail("too many interpolation points for one object (bind the programme by time window)");
      times.resize(first[k] + (size_t)n), source.resize(first[k] + (size_t)n);
      timeline_emit(modes[k], starts[k], tb, b0, b1, n, times.data() + first[k], source.data() + first[k]);
      for (int64_t p = 1; p < n; p++)
        if (times[first[k] + p] - times[first[k] + p - 1] > (int64_t)0x7fffffff)
          timeline_fail("block " + std::to_string(source[first[k] + p] < 0 ? source[first[k] + p - 1] : source[first[k] + p]) +
                        ": a block, a ramp or a gap longer than 2^31-1 samples is not supported");
      first[k + 1] = first[k] + (size_t)n;
      if ((size_t)n > most) most = (size_t)n;
    } catch (const TimelineFailure &f) {
      throw TimelineFailure{n_tracks > 1 ? at + f.msg : f.msg};
    }
  }
  const size_t cols = (size_t)n_buses * n_out;
  std::vector<float> rows(most * cols);
  for (int k = 0; k < n_tracks; k++) {
    const size_t n = first[k + 1] - first[k];
    for (size_t p = 0; p < n; p++) {
      float *row = rows.data() + p * cols;
      const int32_t src = source[first[k] + p];
      if (src < 0) {
        std::memset(row, 0, sizeof(float) * cols);
        continue;
      }
      const size_t at = ((size_t)block_offsets[k] + (size_t)src) * n_out;
      std::memcpy(row, direct + at, sizeof(float) * n_out);
      if (n_buses == 2) std::memcpy(row + n_out, diffuse + at, sizeof(float) * n_out);
    }
    set_object(objects[k], (int)n, times.data() + first[k], rows.data());
  }
}

}  // namespace earhip
