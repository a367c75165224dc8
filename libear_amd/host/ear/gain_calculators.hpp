// ear/gain_calculators.hpp — GainCalculatorObjects with libear's interface
// (include/ear/gain_calculators.hpp:45-56) over the device batch panner (earhip group I), plus the batched
// call a renderer wants: all metadata blocks of all objects in one launch; GainCalculatorHOA and
// GainCalculatorDirectSpeakers over the same panner.
#pragma once
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
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

    /// The native layout behind the caller's: `name` is what the native entry points take, az / el the real positions of
    /// all of ITS channels, and the result says which of them the caller's layout keeps, in the caller's order.  A
    /// BS.2051 name stands for that layout, of which the caller's may be a part (Layout::withoutLfe drops the LFEs; a
    /// channel that is no part of it is refused); any other layout is defined as it is (define_layout).
    inline std::vector<int> match_layout(const Layout &layout, std::string &name, std::vector<double> &az, std::vector<double> &el) {
      int kind = 0;
      hip::check(earhip_layout_kind(layout.name().c_str(), &kind));
      std::vector<int> keep;
      if (kind != 1) {
        name = define_layout(layout);
        for (auto &c : layout.channels()) {
          az.push_back(c.polarPosition().azimuth);
          el.push_back(c.polarPosition().elevation);
          keep.push_back((int)keep.size());
        }
        return keep;
      }
      name = layout.name();
      const Layout full = getLayout(layout.name());
      for (auto &c : full.channels()) {
        az.push_back(c.polarPosition().azimuth);
        el.push_back(c.polarPosition().elevation);
      }
      for (auto &c : layout.channels()) {
        const int i = full.indexForName(c.name());
        if (i < 0) throw invalid_argument("channel " + c.name() + " is not part of layout " + layout.name());
        az[i] = c.polarPosition().azimuth;
        el[i] = c.polarPosition().elevation;
        keep.push_back(i);
      }
      return keep;
    }
  }  // namespace detail

  class GainCalculatorObjects {
   public:
    /// layout: an ITU-R BS.2051 layout (getLayout), with or without its LFE channels, or a layout of the caller's own
    explicit GainCalculatorObjects(const Layout &layout, hip::Context &ctx = hip::default_context()) {
      std::vector<double> az, el;
      std::string name;
      keep_ = detail::match_layout(layout, name, az, el);
      n_full_ = az.size();
      // the loudspeakers' real positions (Channel::polarPosition) shape the panner, the nominal ones its layers
      hip::check(earhip_panner_create_positions(ctx.get(), name.c_str(), (int)n_full_, az.data(), el.data(), &h_));
    }
    ~GainCalculatorObjects() { earhip_panner_destroy(h_); }
    GainCalculatorObjects(const GainCalculatorObjects &) = delete;
    GainCalculatorObjects &operator=(const GainCalculatorObjects &) = delete;

    /// one metadata block -> direct and diffuse gain vectors, which must have the layout's channel count
    /// (libear: OutputGainsT::check_size, include/ear/helpers/output_gains.hpp:40-43)
    template <typename T>
    void calculate(const ObjectsTypeMetadata &metadata, std::vector<T> &directGains, std::vector<T> &diffuseGains,
                   const WarningCB & = default_warning_cb) {  // (libear's Objects calculator emits no warnings either)
      if (directGains.size() != keep_.size() || diffuseGains.size() != keep_.size())
        throw invalid_argument("incorrect size for output vector");
      std::vector<std::vector<T>> d, f;
      calculate(std::vector<ObjectsTypeMetadata>(1, metadata), d, f);
      directGains = d[0];
      diffuseGains = f[0];
    }
    /// a batch of metadata blocks in one device launch
    template <typename T>
    void calculate(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                   std::vector<std::vector<T>> &diffuseGains) {
      const size_t n = metadata.size();
      std::vector<double> az(n), el(n), dist(n), gain(n), diffuse(n), width(n), height(n), depth(n);
      bool extent = false;
      for (size_t i = 0; i < n; i++) {
        const ObjectsTypeMetadata &m = metadata[i];
        // libear's own refusals (src/object_based/gain_calculator_objects.cpp:37-44) ...
        if (m.cartesian || m.position.isCartesian) throw not_implemented("cartesian");
        if (m.objectDivergence.divergence != 0.0) throw not_implemented("divergence");
        if (m.channelLock.flag) throw not_implemented("channelLock");
        if (m.zoneExclusion.zones.size()) throw not_implemented("zoneExclusion");
        if (m.screenRef) throw not_implemented("screenRef");
        // width / height / depth: the polar extent panner (src/object_based/polar_extent.cpp:290-302)
        extent = extent || m.width != 0.0 || m.height != 0.0 || m.depth != 0.0;
        width[i] = m.width;
        height[i] = m.height;
        depth[i] = m.depth;
        az[i] = m.position.polar.azimuth;
        el[i] = m.position.polar.elevation;
        dist[i] = m.position.polar.distance;
        gain[i] = m.gain;
        diffuse[i] = m.diffuse;
      }
      std::vector<float> d(n * n_full_), f(n * n_full_);
      if (extent)
        hip::check(earhip_panner_calculate_extent(h_, n, az.data(), el.data(), dist.data(), width.data(), height.data(),
                                                  depth.data(), gain.data(), diffuse.data(), d.data(), f.data()));
      else
        hip::check(earhip_panner_calculate(h_, n, az.data(), el.data(), dist.data(), gain.data(), diffuse.data(), d.data(),
                                           f.data()));
      directGains.assign(n, std::vector<T>(keep_.size()));
      diffuseGains.assign(n, std::vector<T>(keep_.size()));
      for (size_t i = 0; i < n; i++)
        for (size_t c = 0; c < keep_.size(); c++) {
          directGains[i][c] = (T)d[i * n_full_ + keep_[c]];
          diffuseGains[i][c] = (T)f[i * n_full_ + keep_[c]];
        }
    }

   private:
    earhip_panner *h_ = nullptr;
    std::vector<int> keep_;
    size_t n_full_ = 0;
  };

  /// libear: include/ear/gain_calculators.hpp:18-35 (earhip group I, DirectSpeakers).  One difference: the ITU-R
  /// BS.2127 mapping rules of the common-definitions packs are not carried, and a channel of such a pack
  /// (audioPackFormatID AP_0001xxxx) throws not_implemented.
  class GainCalculatorDirectSpeakers {
   public:
    /// layout: an ITU-R BS.2051 layout (getLayout), with or without its LFE channels, or a layout of the caller's own; additionalSubstitutions:
    /// speakerLabel -> nominal label, on top of (never instead of) LFE -> LFE1, LFEL -> LFE1, LFER -> LFE2
    explicit GainCalculatorDirectSpeakers(const Layout &layout,
                                          std::map<std::string, std::string> additionalSubstitutions = {},
                                          hip::Context &ctx = hip::default_context()) {
      std::vector<double> az, el;
      std::string name;
      keep_ = detail::match_layout(layout, name, az, el);
      n_full_ = az.size();
      std::vector<const char *> from, to;
      for (auto &kv : additionalSubstitutions) from.push_back(kv.first.c_str()), to.push_back(kv.second.c_str());
      hip::check(earhip_direct_speakers_create_positions(ctx.get(), name.c_str(), (int)n_full_, az.data(),
                                                         el.data(), (int)from.size(), from.data(), to.data(), &h_));
    }
    ~GainCalculatorDirectSpeakers() { earhip_direct_speakers_destroy(h_); }
    GainCalculatorDirectSpeakers(const GainCalculatorDirectSpeakers &) = delete;
    GainCalculatorDirectSpeakers &operator=(const GainCalculatorDirectSpeakers &) = delete;

    /// one channel's metadata -> its gains, which must have the layout's channel count (after the ADM check, as
    /// in libear: src/direct_speakers/gain_calculator_direct_speakers.cpp:247-251)
    template <typename T>
    void calculate(const DirectSpeakersTypeMetadata &metadata, std::vector<T> &gains,
                   const WarningCB &warning_cb = default_warning_cb) {
      const bool adm_error_first = metadata.audioPackFormatID && metadata.speakerLabels.empty();
      if (gains.size() != keep_.size() && !adm_error_first) throw invalid_argument("incorrect size for output vector");
      std::vector<std::vector<T>> g;
      calculate(std::vector<DirectSpeakersTypeMetadata>(1, metadata), g, warning_cb);
      gains = g[0];
    }
    /// a batch of channels; the ones that need the point source panner go to the device in one launch.  The
    /// warnings of each channel reach warning_cb in order (on an error: those raised up to it, then the throw).
    template <typename T>
    void calculate(const std::vector<DirectSpeakersTypeMetadata> &metadata, std::vector<std::vector<T>> &gains,
                   const WarningCB &warning_cb = default_warning_cb) {
      const size_t n = metadata.size();
      std::vector<earhip_ds_metadata> md(n);
      std::vector<std::vector<const char *>> labels(n);
      for (size_t i = 0; i < n; i++) {
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
      std::vector<float> g(n * n_full_);
      std::vector<int> warnings(2 * n, 0);
      const int status = earhip_direct_speakers_calculate(h_, n, md.data(), g.data(), warnings.data());
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
      gains.assign(n, std::vector<T>(keep_.size()));
      for (size_t i = 0; i < n; i++)
        for (size_t c = 0; c < keep_.size(); c++) gains[i][c] = (T)g[i * n_full_ + keep_[c]];
    }

   private:
    earhip_direct_speakers *h_ = nullptr;
    std::vector<int> keep_;
    size_t n_full_ = 0;
  };

  /// libear: include/ear/gain_calculators.hpp:58-70
  class GainCalculatorHOA {
   public:
    explicit GainCalculatorHOA(const Layout &layout, hip::Context &ctx = hip::default_context())
        : ctx_(ctx) {
      keep_ = detail::match_layout(layout, name_, az_, el_);
      n_full_ = az_.size();
    }
    /// gains[coefficient][loudspeaker] (libear's column-major vector of vectors): must have that shape
    template <typename T>
    void calculate(const HOATypeMetadata &metadata, std::vector<std::vector<T>> &gains,
                   const WarningCB &warning_cb = default_warning_cb) {
      if (metadata.orders.size() != metadata.degrees.size())
        throw invalid_argument("orders and degrees must be the same size");
      const size_t C = metadata.orders.size();
      if (gains.size() != C) throw invalid_argument("incorrect number of cols in output matrix");
      for (auto &col : gains)
        if (col.size() != keep_.size()) throw invalid_argument("incorrect number of rows in output matrix column");
      std::vector<float> D(n_full_ * (C ? C : 1));
      // (an unknown normalization is refused by the C ABI before anything is ignored, as in libear:
      // src/hoa/gain_calculator_hoa.cpp:36-48)
      if (metadata.normalization == "N3D" || metadata.normalization == "SN3D" || metadata.normalization == "FuMa") {
        if (metadata.screenRef)
          warning_cb({Warning::Code::HOA_SCREENREF_NOT_IMPLEMENTED, "screenRef for HOA is not implemented; ignoring"});
        if (metadata.nfcRefDist != 0.0)
          warning_cb({Warning::Code::HOA_NFCREFDIST_NOT_IMPLEMENTED, "nfcRefDist is not implemented; ignoring"});
      }
      hip::check(earhip_hoa_decode_matrix_positions(ctx_.get(), name_.c_str(), (int)n_full_, az_.data(), el_.data(), (int)C,
                                                    metadata.orders.data(), metadata.degrees.data(),
                                                    metadata.normalization.c_str(), D.data()));
      for (size_t c = 0; c < C; c++)
        for (size_t r = 0; r < keep_.size(); r++) gains[c][r] = (T)D[(size_t)keep_[r] * C + c];
    }

   private:
    std::string name_;
    hip::Context &ctx_;
    std::vector<int> keep_;
    std::vector<double> az_, el_;  // real loudspeaker positions, full layout
    size_t n_full_ = 0;
  };
}  // namespace ear
