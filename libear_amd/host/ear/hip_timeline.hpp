// ear/hip_timeline.hpp — the block timeline: the C++ face of group W of the C ABI (include/earhip.h, where the rule is
// specified).  From the timing of a track's audioBlockFormats — rtime, duration, jumpPosition, interpolationLength, in samples —
// to the interpolation points of ear::dsp::ObjectsRenderer's curves.  libear's ObjectsTypeMetadata carries no timing, so there
// is no libear class any of this mirrors; it follows the conventions of the mirror classes (exceptions for status codes, a
// context argument that defaults to the process-wide one), as hip_objects.hpp and hip_screen.hpp do.
//
//   BlockTiming, TimelineMode        one block's timing; Objects ramp (Interpolated), beds and HOA do not (Stepped)
//   timelinePoints, timelineWindow   the rule itself and the blocks a time window needs: pure host functions
//   ObjectsProgramme                 tracks of (timing, metadata) blocks -> gains -> curves: bind(renderer, t0, t1) sends every
//                                    selected block of every track through ONE call of each gain calculator (Objects polar
//                                    and Cartesian, DirectSpeakers) and makes ONE
//                                    ObjectsRenderer::set_objects_blocks call
//
// A long programme is bound window by window: for (t = 0; t < end; t += W) { programme.bind(renderer, t, t + W); render the
// calls that fall into [t, t + W); } — inside its window each curve is the curve of the whole programme.
#pragma once
#include <cstdint>
#include <limits>
#include <memory>
#include <utility>
#include <vector>

#include "hip_allo_objects.hpp"
#include "hip_direct_speakers.hpp"
#include "hip_objects.hpp"
#include "hip_screen.hpp"

namespace ear {
  namespace hip {
    /// all times are samples of the renderer's clock; take ceil(t * fs) for every block boundary
    struct BlockTiming {
      BlockTiming() {}
      BlockTiming(int64_t rtime_, int64_t duration_, bool jumpPosition_ = false, int64_t interpolationLength_ = -1)
          : rtime(rtime_), duration(duration_), jumpPosition(jumpPosition_), interpolationLength(interpolationLength_) {}
      int64_t rtime = 0;                 ///< from the track's start, >= 0
      int64_t duration = -1;             ///< >= 1; -1: an open end, on the last block only
      bool jumpPosition = false;
      int64_t interpolationLength = -1;  ///< read only with jumpPosition; -1: not given (means 0)
    };

    enum class TimelineMode { Interpolated = EARHIP_TIMELINE_INTERPOLATED, Stepped = EARHIP_TIMELINE_STEPPED };

    /// point k of a curve is at times[k] and takes the row of gains of block source[k], or zeros where source[k] == -1
    struct TimelinePoints {
      std::vector<int64_t> times;
      std::vector<int32_t> source;
    };

    const int64_t kTimelineBegin = std::numeric_limits<int64_t>::min(), kTimelineEnd = std::numeric_limits<int64_t>::max();

    namespace detail {
      inline std::vector<earhip_block_timing> to_c(const std::vector<BlockTiming> &blocks) {
        std::vector<earhip_block_timing> c(blocks.size());
        for (size_t i = 0; i < blocks.size(); i++) {
          c[i] = earhip_block_timing();
          c[i].rtime = blocks[i].rtime, c[i].duration = blocks[i].duration;
          c[i].interpolation_length = blocks[i].interpolationLength, c[i].jump_position = blocks[i].jumpPosition ? 1 : 0;
        }
        return c;
      }
    }  // namespace detail

    /// the points of one track for the window [t0, t1); throws ear::invalid_argument for what group W refuses, naming the block
    inline TimelinePoints timelinePoints(TimelineMode mode, int64_t start, const std::vector<BlockTiming> &blocks,
                                         int64_t t0 = kTimelineBegin, int64_t t1 = kTimelineEnd) {
      const std::vector<earhip_block_timing> c = detail::to_c(blocks);
      int n = 0;
      check(earhip_timeline_points((int)mode, start, (int)c.size(), c.data(), t0, t1, 0, nullptr, nullptr, &n));
      TimelinePoints p;
      p.times.resize(n), p.source.resize(n);
      check(earhip_timeline_points((int)mode, start, (int)c.size(), c.data(), t0, t1, n, p.times.data(), p.source.data(), &n));
      return p;
    }

    /// (first, last) block whose rows the curve of the window [t0, t1) uses
    inline std::pair<int, int> timelineWindow(TimelineMode mode, int64_t start, const std::vector<BlockTiming> &blocks,
                                              int64_t t0 = kTimelineBegin, int64_t t1 = kTimelineEnd) {
      const std::vector<earhip_block_timing> c = detail::to_c(blocks);
      std::pair<int, int> w(0, 0);
      check(earhip_timeline_window((int)mode, start, (int)c.size(), c.data(), t0, t1, &w.first, &w.second));
      return w;
    }

    /// one track of ObjectsRenderer::set_objects_blocks
    struct TimelineTrack {
      size_t object = 0;
      TimelineMode mode = TimelineMode::Interpolated;
      int64_t start = 0;
      std::vector<BlockTiming> blocks;
    };

    /// The tracks of a programme with what each block renders: Objects tracks with one ObjectsTypeMetadata per block, polar or
    /// Cartesian block by block, and stepped tracks (beds, HOA channels) whose constant rows came from the DirectSpeakers or
    /// the HOA calculator, or whose DirectSpeakersTypeMetadata bind() sends through ear::hip::DirectSpeakersGainCalculator
    /// itself (a bed with Cartesian positions or screenEdgeLocks included).  bind() turns a time window of it into the curves of
    /// a renderer.
    class ObjectsProgramme {
     public:
      /// layout: what the renderer renders to (its channel count is the renderer's n_out); a layout of the caller's own has
      /// no allocentric table, and a Cartesian block then throws not_implemented at bind
      explicit ObjectsProgramme(const Layout &layout, Context &ctx = default_context()) : layout_(layout), ctx_(ctx) {}
      /// with a reproduction screen: blocks with screenRef or a screenEdgeLock go through ScreenHandler first
      ObjectsProgramme(const Layout &layout, const Screen &reproduction, Context &ctx = default_context())
          : layout_(layout), ctx_(ctx), screen_(new ScreenHandler(reproduction)) {}

      /// an Objects track (gains ramp from block to block).  locks: empty, or one per block
      void add_object(size_t object, int64_t start, const std::vector<std::pair<BlockTiming, ObjectsTypeMetadata>> &blocks,
                      const std::vector<ScreenEdgeLock> &locks = std::vector<ScreenEdgeLock>()) {
        if (!locks.empty() && locks.size() != blocks.size()) throw invalid_argument("locks must be empty or one per block");
        Track t;
        t.timing.object = object, t.timing.mode = TimelineMode::Interpolated, t.timing.start = start;
        for (auto &b : blocks) t.timing.blocks.push_back(b.first), t.metadata.push_back(b.second);
        t.locks = locks;
        tracks_.push_back(t);
      }
      /// a stepped track: rows[block][channel of the layout] on the direct bus, nothing on the diffuse bus
      void add_stepped(size_t object, int64_t start, const std::vector<BlockTiming> &timings,
                       const std::vector<std::vector<float>> &rows) {
        if (rows.size() != timings.size()) throw invalid_argument("one row of gains per block");
        Track t;
        t.timing.object = object, t.timing.mode = TimelineMode::Stepped, t.timing.start = start;
        t.timing.blocks = timings;
        t.rows = rows;
        tracks_.push_back(t);
      }
      /// a DirectSpeakers channel: a stepped track whose rows bind() computes, one DirectSpeakersTypeMetadata per block, polar
      /// or Cartesian, with or without a screenEdgeLock (locked to the programme's reproduction screen when it has one)
      void add_direct_speakers(size_t object, int64_t start, const std::vector<BlockTiming> &timings,
                               const std::vector<DirectSpeakersTypeMetadata> &metadata) {
        if (metadata.size() != timings.size()) throw invalid_argument("one DirectSpeakersTypeMetadata per block");
        Track t;
        t.timing.object = object, t.timing.mode = TimelineMode::Stepped, t.timing.start = start;
        t.timing.blocks = timings;
        t.bed = metadata;
        tracks_.push_back(t);
      }
      size_t size() const { return tracks_.size(); }

      /// Bind the window [t0, t1) of every track to `renderer` (ear::dsp::ObjectsRenderer), whose commit stays the caller's.
      /// Whatever throws — a block list group W refuses, a block a calculator refuses — throws before any curve has changed.
      /// warning_cb receives the warnings of the DirectSpeakers tracks' selected blocks (e.g. a lowPass on a label that is no
      /// LFE label), in track order, at every bind.
      template <typename Renderer>
      void bind(Renderer &renderer, int64_t t0 = kTimelineBegin, int64_t t1 = kTimelineEnd,
                const WarningCB &warning_cb = default_warning_cb) {
        const size_t n_out = layout_.channels().size();
        if (renderer.n_out() != n_out) throw invalid_argument("the renderer's outputs are not the programme's layout");
        // 1. the blocks each track needs
        std::vector<TimelineTrack> tracks;
        std::vector<size_t> first_row;
        size_t total = 0;
        std::vector<ObjectsTypeMetadata> polar, cartesian;
        std::vector<ScreenEdgeLock> polar_locks, cartesian_locks;
        std::vector<size_t> polar_row, cartesian_row;
        bool polar_screen = false, cartesian_screen = false;
        std::vector<DirectSpeakersTypeMetadata> bed;
        std::vector<size_t> bed_row;
        for (const Track &t : tracks_) {
          const std::pair<int, int> w = timelineWindow(t.timing.mode, t.timing.start, t.timing.blocks, t0, t1);
          tracks.push_back(t.timing);
          first_row.push_back(total);
          for (int b = w.first; b <= w.second && !t.metadata.empty(); b++) {
            const ObjectsTypeMetadata &m = t.metadata[b];
            const ScreenEdgeLock lock = t.locks.empty() ? ScreenEdgeLock() : t.locks[b];
            const bool on_screen = m.screenRef || lock.horizontal || lock.vertical;
            if (m.cartesian) {
              cartesian.push_back(m), cartesian_locks.push_back(lock), cartesian_row.push_back(total + b);
              cartesian_screen = cartesian_screen || on_screen;
            } else {
              polar.push_back(m), polar_locks.push_back(lock), polar_row.push_back(total + b);
              polar_screen = polar_screen || on_screen;
            }
          }
          for (int b = w.first; b <= w.second && !t.bed.empty(); b++) bed.push_back(t.bed[b]), bed_row.push_back(total + b);
          total += t.timing.blocks.size();
        }
        // 2. every selected block through one call of its calculator, behind the screen stage where a block asks for it
        std::vector<float> direct(total * n_out, 0.0f), diffuse(total * n_out, 0.0f);
        std::vector<std::vector<float>> d, f;
        if (!polar.empty()) {
          if (screen_ && polar_screen) screen_->apply(polar, polar_locks, ctx_);
          if (!polar_calc_) polar_calc_.reset(new ObjectsGainCalculator(layout_, ctx_));
          polar_calc_->calculate(polar, d, f);
          put(d, polar_row, n_out, direct), put(f, polar_row, n_out, diffuse);
        }
        if (!cartesian.empty()) {
          if (screen_ && cartesian_screen) screen_->apply_cartesian(cartesian, cartesian_locks, ctx_);
          if (!cartesian_calc_) cartesian_calc_.reset(new AllocentricObjectsGainCalculator(layout_));
          cartesian_calc_->calculate(cartesian, d, f);
          put(d, cartesian_row, n_out, direct), put(f, cartesian_row, n_out, diffuse);
        }
        if (!bed.empty()) {
          if (!bed_calc_)
            bed_calc_.reset(screen_ ? new DirectSpeakersGainCalculator(layout_, *screen_, {}, ctx_)
                                          : new DirectSpeakersGainCalculator(layout_, {}, ctx_));
          bed_calc_->calculate(bed, d, warning_cb);
          put(d, bed_row, n_out, direct);
        }
        for (size_t k = 0; k < tracks_.size(); k++)
          for (size_t b = 0; b < tracks_[k].rows.size(); b++) {
            if (tracks_[k].rows[b].size() != n_out) throw invalid_argument("gain vector length != number of outputs");
            for (size_t c = 0; c < n_out; c++) direct[(first_row[k] + b) * n_out + c] = tracks_[k].rows[b][c];
          }
        // 3. one call for all curves
        renderer.set_objects_blocks(tracks, direct, diffuse, t0, t1);
      }

     private:
      struct Track {
        TimelineTrack timing;
        std::vector<ObjectsTypeMetadata> metadata;  // Objects tracks
        std::vector<ScreenEdgeLock> locks;
        std::vector<std::vector<float>> rows;  // stepped tracks
        std::vector<DirectSpeakersTypeMetadata> bed;  // DirectSpeakers tracks
      };
      static void put(const std::vector<std::vector<float>> &rows, const std::vector<size_t> &at, size_t n_out,
                      std::vector<float> &flat) {
        for (size_t i = 0; i < rows.size(); i++)
          for (size_t c = 0; c < n_out; c++) flat[at[i] * n_out + c] = rows[i][c];
      }

      const Layout layout_;
      Context &ctx_;
      std::unique_ptr<ScreenHandler> screen_;
      std::unique_ptr<ObjectsGainCalculator> polar_calc_;
      std::unique_ptr<AllocentricObjectsGainCalculator> cartesian_calc_;
      std::unique_ptr<DirectSpeakersGainCalculator> bed_calc_;
      std::vector<Track> tracks_;
    };
  }  // namespace hip
}  // namespace ear

#include "dsp/objects_renderer.hpp"
