// ear/hip_batch.hpp — what the mirror's gain calculators and device batches share, each piece once: the native layout behind
// a caller's Layout and the scatter of its rows (LayoutBinding), the single-block calculate, the polar and the Cartesian
// Objects rows, the DirectSpeakers rows, the allocentric handle, the zone conversion, and the device batch: a block of host memory the device
// reaches, carved into typed arrays (Carver, DeviceBatch), and the step after the device call (finish).
#pragma once
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "hip.hpp"
#include "metadata.hpp"
#include "warnings.hpp"

namespace ear {
  namespace detail {
    /// 64-bit FNV-1a
    inline void fnv1a(uint64_t &h, const void *data, size_t n) {
      const unsigned char *p = static_cast<const unsigned char *>(data);
      for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    }

    /// A layout that is not one of BS.2051 — libear's Layout(name, channels) is a public constructor — is defined in the
    /// native registry (earhip_layout_define, group H) under "ear:" + 16 hex digits of a hash over each channel's name,
    /// the bits of its nominal azimuth and elevation, its LFE flag and the ranges it was given, if any.  The layout's own
    /// name is not part of it: an empty name, or one name for two layouts, works.  Returns the registry name.
    inline std::string define_layout(const Layout &layout) {
      const std::vector<Channel> &ch = layout.channels();
      std::vector<earhip_layout_channel_def> defs(ch.size());
      uint64_t h = 0xcbf29ce484222325ull;
      for (size_t i = 0; i < ch.size(); i++) {
        earhip_layout_channel_def &d = defs[i];
        d = earhip_layout_channel_def();
        d.name = ch[i].name().c_str();
        d.azimuth = ch[i].polarPositionNominal().azimuth;
        d.elevation = ch[i].polarPositionNominal().elevation;
        d.is_lfe = ch[i].isLfe() ? 1 : 0;
        // (a range that was never set reads as the REAL position, which is no part of a definition: the nominal one)
        d.has_ranges = ch[i].hasAzimuthRange() || ch[i].hasElevationRange();
        d.azimuth_range[0] = d.azimuth_range[1] = d.azimuth;
        d.elevation_range[0] = d.elevation_range[1] = d.elevation;
        if (ch[i].hasAzimuthRange()) d.azimuth_range[0] = ch[i].azimuthRange().first, d.azimuth_range[1] = ch[i].azimuthRange().second;
        if (ch[i].hasElevationRange())
          d.elevation_range[0] = ch[i].elevationRange().first, d.elevation_range[1] = ch[i].elevationRange().second;
        const unsigned char flags[2] = {(unsigned char)d.is_lfe, (unsigned char)d.has_ranges};
        fnv1a(h, ch[i].name().c_str(), ch[i].name().size() + 1);
        fnv1a(h, &d.azimuth, sizeof(double));
        fnv1a(h, &d.elevation, sizeof(double));
        fnv1a(h, flags, sizeof(flags));
        if (d.has_ranges) fnv1a(h, d.azimuth_range, sizeof(d.azimuth_range)), fnv1a(h, d.elevation_range, sizeof(d.elevation_range));
      }
      char name[32];
      std::snprintf(name, sizeof(name), "ear:%016llx", (unsigned long long)h);
      hip::check(earhip_layout_define(name, (int)defs.size(), defs.data()));
      return name;
    }

    /// The native layout behind the caller's: `name` is what the native entry points take, az / el (empty on entry) the real
    /// positions of all of ITS channels, and the result says which of them the caller's layout keeps, in the caller's order.
    /// A BS.2051 name stands for that layout, of which the caller's may be a part (Layout::withoutLfe drops the LFEs; a
    /// channel that is no part of it is refused); any other layout is defined as it is (define_layout).
    inline std::vector<int> match_layout(const Layout &layout, std::string &name, std::vector<double> &az, std::vector<double> &el) {
      int kind = 0;
      hip::check(earhip_layout_kind(layout.name().c_str(), &kind));
      name = kind == 1 ? layout.name() : define_layout(layout);
      const Layout full = kind == 1 ? getLayout(layout.name()) : layout;
      for (auto &c : full.channels()) az.push_back(c.polarPosition().azimuth), el.push_back(c.polarPosition().elevation);
      std::vector<int> keep;
      for (auto &c : layout.channels()) {
        const int i = kind == 1 ? full.indexForName(c.name()) : (int)keep.size();
        if (i < 0) throw invalid_argument("channel " + c.name() + " is not part of layout " + layout.name());
        az[i] = c.polarPosition().azimuth, el[i] = c.polarPosition().elevation;
        keep.push_back(i);
      }
      return keep;
    }

    /// What match_layout returns, held by a calculator: the entry points work on the n_full channels of `name`
    struct LayoutBinding {
      LayoutBinding() {}
      explicit LayoutBinding(const Layout &layout) : keep(match_layout(layout, name, az, el)), n_full(az.size()) {}

      void check_size(size_t direct, size_t diffuse) const {
        if (direct != keep.size() || diffuse != keep.size()) throw invalid_argument("incorrect size for output vector");
      }
      /// rows [n][n_full] of the native layout -> n vectors of the caller's channels
      template <typename T>
      void scatter(size_t n, const float *rows, std::vector<std::vector<T>> &out) const {
        out.assign(n, std::vector<T>(keep.size()));
        for (size_t i = 0; i < n; i++)
          for (size_t c = 0; c < keep.size(); c++) out[i][c] = (T)rows[i * n_full + keep[c]];
      }

      std::string name;
      std::vector<double> az, el;  // real loudspeaker positions, full layout
      std::vector<int> keep;
      size_t n_full = 0;
    };

    /// one metadata block through a calculator's batch form (libear: include/ear/helpers/output_gains.hpp:40-43)
    template <typename Calculator, typename T>
    void calculate_one(Calculator &calc, const LayoutBinding &layout, const ObjectsTypeMetadata &metadata,
                       std::vector<T> &directGains, std::vector<T> &diffuseGains) {
      layout.check_size(directGains.size(), diffuseGains.size());
      std::vector<std::vector<T>> d, f;
      calc.calculate(std::vector<ObjectsTypeMetadata>(1, metadata), d, f);
      directGains = d[0];
      diffuseGains = f[0];
    }

    inline earhip_exclusion_zone to_c(const ExclusionZone &z) {
      earhip_exclusion_zone c = earhip_exclusion_zone();
      c.cartesian = z.isCartesian;
      c.min_azimuth = z.polar.minAzimuth, c.max_azimuth = z.polar.maxAzimuth;
      c.min_elevation = z.polar.minElevation, c.max_elevation = z.polar.maxElevation;
      c.min_x = z.cartesian.minX, c.max_x = z.cartesian.maxX;
      c.min_y = z.cartesian.minY, c.max_y = z.cartesian.maxY;
      c.min_z = z.cartesian.minZ, c.max_z = z.cartesian.maxZ;
      return c;
    }

    /// the rows of a polar Objects batch the panner's entry points share; the caller refuses what it does not render first
    struct PolarRows {
      explicit PolarRows(size_t n) : az(n), el(n), dist(n), width(n), height(n), depth(n), gain(n), diffuse(n) {}
      void set(size_t i, const ObjectsTypeMetadata &m) {
        az[i] = m.position.polar.azimuth, el[i] = m.position.polar.elevation, dist[i] = m.position.polar.distance;
        width[i] = m.width, height[i] = m.height, depth[i] = m.depth;
        gain[i] = m.gain, diffuse[i] = m.diffuse;
      }
      std::vector<double> az, el, dist, width, height, depth, gain, diffuse;
    };

    /// The rows of a DirectSpeakers batch as group I takes them, with the label pointers they refer to (`metadata` must
    /// outlive them).  The polar position and its bounds are filled in whatever the position is; the two screenEdgeLock
    /// fields say whether a lock is set.
    struct DirectSpeakersRows {
      explicit DirectSpeakersRows(const std::vector<DirectSpeakersTypeMetadata> &metadata)
          : md(metadata.size()), labels(metadata.size()) {
        for (size_t i = 0; i < metadata.size(); i++) {
          const DirectSpeakersTypeMetadata &m = metadata[i];
          earhip_ds_metadata &c = md[i];
          c = earhip_ds_metadata();
          for (auto &l : m.speakerLabels) labels[i].push_back(l.c_str());
          c.n_labels = (int)labels[i].size();
          c.labels = labels[i].data();
          c.cartesian = m.position.isCartesian;
          const PolarSpeakerPosition &p = m.position.polar;
          c.azimuth = p.azimuth, c.elevation = p.elevation, c.distance = p.distance;
          c.has_azimuth_min = (bool)p.azimuthMin, c.azimuth_min = p.azimuthMin.value_or(0.0);
          c.has_azimuth_max = (bool)p.azimuthMax, c.azimuth_max = p.azimuthMax.value_or(0.0);
          c.has_elevation_min = (bool)p.elevationMin, c.elevation_min = p.elevationMin.value_or(0.0);
          c.has_elevation_max = (bool)p.elevationMax, c.elevation_max = p.elevationMax.value_or(0.0);
          c.has_distance_min = (bool)p.distanceMin, c.distance_min = p.distanceMin.value_or(0.0);
          c.has_distance_max = (bool)p.distanceMax, c.distance_max = p.distanceMax.value_or(0.0);
          c.screen_edge_lock_horizontal = (bool)p.screenEdgeLock.horizontal;
          c.screen_edge_lock_vertical = (bool)p.screenEdgeLock.vertical;
          c.has_low_pass = (bool)m.channelFrequency.lowPass, c.low_pass = m.channelFrequency.lowPass.value_or(0.0);
          c.has_high_pass = (bool)m.channelFrequency.highPass, c.high_pass = m.channelFrequency.highPass.value_or(0.0);
          c.audio_pack_format_id = m.audioPackFormatID ? m.audioPackFormatID.get().c_str() : nullptr;
        }
      }
      /// After the call (status: what it returned; warnings: its warnings_out): every warning to warning_cb in order, then
      /// the throw for a failed call
      static void finish(int status, const std::vector<int> &warnings, const WarningCB &warning_cb) {
        const std::string error = status == EARHIP_OK ? std::string() : std::string(earhip_last_error());
        for (int w : warnings) {
          // (libear's messages: src/direct_speakers/gain_calculator_direct_speakers.cpp:118-120, :132-134)
          if (w == (int)Warning::Code::FREQ_NOT_LFE)
            warning_cb({Warning::Code::FREQ_NOT_LFE, "frequency indication present but does not indicate an LFE channel"});
          else if (w == (int)Warning::Code::FREQ_SPEAKERLABEL_LFE_MISMATCH)
            warning_cb({Warning::Code::FREQ_SPEAKERLABEL_LFE_MISMATCH,
                        "LFE indication from frequency element does not match speakerLabel"});
        }
        hip::check(status, error);
      }

      std::vector<earhip_ds_metadata> md;
      std::vector<std::vector<const char *>> labels;
    };

    /// Owner of an earhip_allo with the layout it was made for: what the two allocentric calculators are made of.
    class AlloHandle {
     public:
      /// the built-in table of group T; a layout of the caller's own has none: not_implemented
      explicit AlloHandle(const Layout &l) : layout(l) { hip::check(earhip_allo_create(layout.name.c_str(), &h_)); }
      /// one position per channel of `l`, in its order
      AlloHandle(const Layout &l, const std::vector<CartesianPosition> &positions) : layout(l) {
        const std::vector<int> &keep = layout.keep;
        if (positions.size() != keep.size()) throw invalid_argument("one position per channel of the layout");
        // (a BS.2051 layout given without its LFE channels: the native creator ignores those rows, and refuses the NaN of
        // any other channel that is missing)
        const double none = std::numeric_limits<double>::quiet_NaN();
        std::vector<double> x(layout.n_full, none), y(layout.n_full, none), z(layout.n_full, none);
        for (size_t c = 0; c < keep.size(); c++) x[keep[c]] = positions[c].X, y[keep[c]] = positions[c].Y, z[keep[c]] = positions[c].Z;
        hip::check(earhip_allo_create_positions(layout.name.c_str(), (int)layout.n_full, x.data(), y.data(), z.data(), &h_));
      }
      ~AlloHandle() { earhip_allo_destroy(h_); }
      AlloHandle(const AlloHandle &) = delete;
      AlloHandle &operator=(const AlloHandle &) = delete;
      earhip_allo *get() const { return h_; }

      /// the rows of a Cartesian Objects batch.  v: the double arrays of the C ABI, in its order
      struct Rows {
        enum { X, Y, Z, WIDTH, HEIGHT, DEPTH, GAIN, DIFFUSE, LOCK_MAX, DIVERGENCE, RANGE, kDoubles };
        std::vector<double> v[kDoubles];
        std::vector<unsigned char> lock;
        std::vector<uint32_t> excluded;
      };
      /// refuse(block) throws for what the calling class does not render; a polar zone is refused for all, after it
      Rows gather(const std::vector<ObjectsTypeMetadata> &metadata, void (*refuse)(const ObjectsTypeMetadata &)) const {
        const size_t n = metadata.size();
        Rows b;
        for (std::vector<double> &a : b.v) a.resize(n);
        b.lock.assign(n, 0), b.excluded.assign(n, 0);
        for (size_t i = 0; i < n; i++) {
          const ObjectsTypeMetadata &m = metadata[i];
          refuse(m);
          b.v[Rows::X][i] = m.position.cartesian.X, b.v[Rows::Y][i] = m.position.cartesian.Y, b.v[Rows::Z][i] = m.position.cartesian.Z;
          b.v[Rows::WIDTH][i] = m.width, b.v[Rows::HEIGHT][i] = m.height, b.v[Rows::DEPTH][i] = m.depth;
          b.v[Rows::GAIN][i] = m.gain, b.v[Rows::DIFFUSE][i] = m.diffuse;
          b.lock[i] = m.channelLock.flag ? 1 : 0;
          b.v[Rows::LOCK_MAX][i] = m.channelLock.hasMaxDistance ? m.channelLock.maxDistance : std::numeric_limits<double>::infinity();
          b.v[Rows::DIVERGENCE][i] = m.objectDivergence.divergence;
          b.v[Rows::RANGE][i] = m.objectDivergence.isCartesian ? m.objectDivergence.range : 0.0;
          if (!m.zoneExclusion.zones.empty()) {
            std::vector<earhip_exclusion_zone> zones;
            for (const ExclusionZone &zn : m.zoneExclusion.zones) {
              if (!zn.isCartesian) throw not_implemented("zoneExclusion: polar zone");
              zones.push_back(to_c(zn));
            }
            hip::check(earhip_allo_excluded_channels(h_, (int)zones.size(), zones.data(), &b.excluded[i]));
          }
        }
        return b;
      }

      const LayoutBinding layout;

     private:
      earhip_allo *h_ = nullptr;
    };

    /// Hands out a block of memory as typed arrays, one after the other.  Knows nothing of HIP.  Without a block (base ==
    /// nullptr) it only counts, which is how bytes_for sizes a block by the takes that will carve it.
    class Carver {
     public:
      Carver(void *base, size_t bytes) : base_(static_cast<unsigned char *>(base)), bytes_(bytes) {}
      /// the next `count` elements of T; one that would start misaligned or end outside the block is the caller's bug
      template <typename T>
      T *take(size_t count) {
        if (used_ % alignof(T) != 0 || (base_ && reinterpret_cast<uintptr_t>(base_) % alignof(T) != 0) ||
            count > (bytes_ - used_) / sizeof(T))
          throw internal_error("device batch: an array misaligned or outside its block at offset " + std::to_string(used_));
        T *p = base_ ? static_cast<T *>(static_cast<void *>(base_ + used_)) : nullptr;
        used_ += count * sizeof(T);
        return p;
      }
      size_t used() const { return used_; }
      /// the bytes that Arrays(carver, sizes...) takes
      template <typename Arrays, typename... Sizes>
      static size_t bytes_for(Sizes... sizes) {
        Carver count(nullptr, std::numeric_limits<size_t>::max());
        (void)Arrays(count, sizes...);
        return count.used();
      }

     private:
      unsigned char *base_;
      size_t bytes_, used_ = 0;
    };

    /// One block of host memory the device reaches (earhip_host_alloc), released on every path, carved into `Arrays`: a
    /// struct whose constructor (Carver &, sizes...) takes its members in order.
    template <typename Arrays>
    class DeviceBatch {
     public:
      template <typename... Sizes>
      explicit DeviceBatch(hip::Context &ctx, Sizes... sizes)
          : mem_(ctx.get(), Carver::bytes_for<Arrays>(sizes...)), carver_(mem_.p, mem_.bytes), arrays(carver_, sizes...) {}
      DeviceBatch(const DeviceBatch &) = delete;
      DeviceBatch &operator=(const DeviceBatch &) = delete;

      /// After the device call (st: its status): waits for the stream, then throws for a failed call — with its message,
      /// read at once — or for the first element k < n whose status[k] is not 0, with the (status code, message) that
      /// describe(k) returns.  The caller writes back after it returns.
      template <typename Describe>
      void finish(int st, const int *status, size_t n, Describe describe) const {
        if (st == EARHIP_OK) st = earhip_ctx_synchronize(mem_.ctx);
        std::string msg = st == EARHIP_OK ? std::string() : std::string(earhip_last_error());
        for (size_t k = 0; k < n && st == EARHIP_OK; k++)
          if (status[k] != 0) {
            const std::pair<int, std::string> r = describe(k);
            st = r.first, msg = r.second;
          }
        hip::check(st, msg);
      }

     private:
      struct Mem {
        Mem(earhip_ctx *c, size_t b) : ctx(c), bytes(b) { hip::check(earhip_host_alloc(ctx, bytes, &p)); }
        ~Mem() { earhip_host_release(ctx, p); }
        earhip_ctx *ctx;
        size_t bytes;
        void *p = nullptr;
      };
      Mem mem_;
      Carver carver_;

     public:
      const Arrays arrays;
    };

    /// what a batch makes of block i that the device refused: (code, "metadata block i: what")
    inline std::pair<int, std::string> bad_block(size_t i, const char *what, int code = EARHIP_INVALID_ARGUMENT) {
      return {code, "metadata block " + std::to_string(i) + ": " + what};
    }
  }  // namespace detail
}  // namespace ear
