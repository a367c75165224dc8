// ear/gain_calculators.hpp — GainCalculatorObjects with libear's interface
// (include/ear/gain_calculators.hpp:45-56) over the device batch panner (earhip group I), plus the batched
// call a renderer wants: all metadata blocks of all objects in one launch; GainCalculatorHOA and
// GainCalculatorDirectSpeakers over the same panner.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "hip_batch.hpp"
#include "warnings.hpp"

namespace ear {
  class GainCalculatorObjects {
   public:
    /// layout: an ITU-R BS.2051 layout (getLayout), with or without its LFE channels, or a layout of the caller's own
    explicit GainCalculatorObjects(const Layout &layout, hip::Context &ctx = hip::default_context()) : layout_(layout) {
      // the loudspeakers' real positions (Channel::polarPosition) shape the panner, the nominal ones its layers
      hip::check(earhip_panner_create_positions(ctx.get(), layout_.name.c_str(), (int)layout_.n_full, layout_.az.data(),
                                                layout_.el.data(), &h_));
    }
    ~GainCalculatorObjects() { earhip_panner_destroy(h_); }
    GainCalculatorObjects(const GainCalculatorObjects &) = delete;
    GainCalculatorObjects &operator=(const GainCalculatorObjects &) = delete;

    /// one metadata block -> direct and diffuse gain vectors, which must have the layout's channel count
    /// (libear: OutputGainsT::check_size, include/ear/helpers/output_gains.hpp:40-43)
    template <typename T>
    void calculate(const ObjectsTypeMetadata &metadata, std::vector<T> &directGains, std::vector<T> &diffuseGains,
                   const WarningCB & = default_warning_cb) {  // (libear's Objects calculator emits no warnings either)
      detail::calculate_one(*this, layout_, metadata, directGains, diffuseGains);
    }
    /// a batch of metadata blocks in one device launch
    template <typename T>
    void calculate(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                   std::vector<std::vector<T>> &diffuseGains) {
      const size_t n = metadata.size();
      detail::PolarRows r(n);
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
        r.set(i, m);
      }
      std::vector<float> d(n * layout_.n_full), f(n * layout_.n_full);
      if (extent)
        hip::check(earhip_panner_calculate_extent(h_, n, r.az.data(), r.el.data(), r.dist.data(), r.width.data(), r.height.data(),
                                                  r.depth.data(), r.gain.data(), r.diffuse.data(), d.data(), f.data()));
      else
        hip::check(earhip_panner_calculate(h_, n, r.az.data(), r.el.data(), r.dist.data(), r.gain.data(), r.diffuse.data(),
                                           d.data(), f.data()));
      layout_.scatter(n, d.data(), directGains);
      layout_.scatter(n, f.data(), diffuseGains);
    }

   private:
    const detail::LayoutBinding layout_;
    earhip_panner *h_ = nullptr;
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
                                          hip::Context &ctx = hip::default_context())
        : layout_(layout) {
      std::vector<const char *> from, to;
      for (auto &kv : additionalSubstitutions) from.push_back(kv.first.c_str()), to.push_back(kv.second.c_str());
      hip::check(earhip_direct_speakers_create_positions(ctx.get(), layout_.name.c_str(), (int)layout_.n_full, layout_.az.data(),
                                                         layout_.el.data(), (int)from.size(), from.data(), to.data(), &h_));
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
      if (!adm_error_first) layout_.check_size(gains.size(), gains.size());
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
      const detail::DirectSpeakersRows rows(metadata);
      std::vector<float> g(n * layout_.n_full);
      std::vector<int> warnings(2 * n, 0);
      const int status = earhip_direct_speakers_calculate(h_, n, rows.md.data(), g.data(), warnings.data());
      detail::DirectSpeakersRows::finish(status, warnings, warning_cb);
      layout_.scatter(n, g.data(), gains);
    }

   private:
    const detail::LayoutBinding layout_;
    earhip_direct_speakers *h_ = nullptr;
  };

  /// libear: include/ear/gain_calculators.hpp:58-70
  class GainCalculatorHOA {
   public:
    explicit GainCalculatorHOA(const Layout &layout, hip::Context &ctx = hip::default_context())
        : layout_(layout), ctx_(ctx) {}
    /// gains[coefficient][loudspeaker] (libear's column-major vector of vectors): must have that shape
    template <typename T>
    void calculate(const HOATypeMetadata &metadata, std::vector<std::vector<T>> &gains,
                   const WarningCB &warning_cb = default_warning_cb) {
      if (metadata.orders.size() != metadata.degrees.size())
        throw invalid_argument("orders and degrees must be the same size");
      const size_t C = metadata.orders.size(), n_full = layout_.n_full;
      if (gains.size() != C) throw invalid_argument("incorrect number of cols in output matrix");
      for (auto &col : gains)
        if (col.size() != layout_.keep.size()) throw invalid_argument("incorrect number of rows in output matrix column");
      std::vector<float> D(n_full * (C ? C : 1));
      // (an unknown normalization is refused by the C ABI before anything is ignored, as in libear:
      // src/hoa/gain_calculator_hoa.cpp:36-48)
      if (metadata.normalization == "N3D" || metadata.normalization == "SN3D" || metadata.normalization == "FuMa") {
        if (metadata.screenRef)
          warning_cb({Warning::Code::HOA_SCREENREF_NOT_IMPLEMENTED, "screenRef for HOA is not implemented; ignoring"});
        if (metadata.nfcRefDist != 0.0)
          warning_cb({Warning::Code::HOA_NFCREFDIST_NOT_IMPLEMENTED, "nfcRefDist is not implemented; ignoring"});
      }
      hip::check(earhip_hoa_decode_matrix_positions(ctx_.get(), layout_.name.c_str(), (int)n_full, layout_.az.data(),
                                                    layout_.el.data(), (int)C,
                                                    metadata.orders.data(), metadata.degrees.data(),
                                                    metadata.normalization.c_str(), D.data()));
      for (size_t c = 0; c < C; c++)
        for (size_t r = 0; r < layout_.keep.size(); r++) gains[c][r] = (T)D[(size_t)layout_.keep[r] * C + c];
    }

   private:
    const detail::LayoutBinding layout_;
    hip::Context &ctx_;
  };
}  // namespace ear
