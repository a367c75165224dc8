// ear/hip_objects.hpp — an Objects gain calculator that carries channelLock, polar objectDivergence and zoneExclusion: the
// C++ face of the _objects forms of group I of the C ABI (include/earhip.h, where the three are specified).  libear refuses
// these fields (src/object_based/gain_calculator_objects.cpp:37-44) and ear::GainCalculatorObjects keeps refusing them, so
// there is no libear class this one mirrors; it has that class's constructor and calculate overloads and follows the
// conventions of the mirror classes (exceptions for status codes, a context argument that defaults to the process-wide one),
// as hip_iir.hpp and hip_src.hpp do.
#pragma once
#include <cstdint>
#include <limits>
#include <vector>

#include "gain_calculators.hpp"

namespace ear {
  namespace hip {
    class ObjectsGainCalculator {
     public:
      /// layout: an ITU-R BS.2051 layout (getLayout), with or without its LFE channels, or a layout of the caller's own
      explicit ObjectsGainCalculator(const Layout &layout, Context &ctx = default_context()) : layout_(layout) {
        check(earhip_panner_create_positions(ctx.get(), layout_.name.c_str(), (int)layout_.n_full, layout_.az.data(),
                                             layout_.el.data(), &h_));
      }
      ~ObjectsGainCalculator() { earhip_panner_destroy(h_); }
      ObjectsGainCalculator(const ObjectsGainCalculator &) = delete;
      ObjectsGainCalculator &operator=(const ObjectsGainCalculator &) = delete;

      /// one metadata block -> direct and diffuse gain vectors, which must have the layout's channel count
      template <typename T>
      void calculate(const ObjectsTypeMetadata &metadata, std::vector<T> &directGains, std::vector<T> &diffuseGains,
                     const WarningCB & = default_warning_cb) {
        ear::detail::calculate_one(*this, layout_, metadata, directGains, diffuseGains);
      }
      /// a batch of metadata blocks in one device call.  Still refused, with libear's messages: Cartesian positions and
      /// `cartesian`, a non-zero CartesianObjectDivergence, screenRef.
      template <typename T>
      void calculate(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                     std::vector<std::vector<T>> &diffuseGains) {
        const size_t n = metadata.size();
        ear::detail::PolarRows r(n);
        std::vector<double> lock_max(n), div(n), range(n);
        std::vector<unsigned char> lock(n);
        std::vector<uint32_t> excluded(n, 0);
        for (size_t i = 0; i < n; i++) {
          const ObjectsTypeMetadata &m = metadata[i];
          if (m.cartesian || m.position.isCartesian) throw not_implemented("cartesian");
          if (m.objectDivergence.isCartesian && m.objectDivergence.divergence != 0.0) throw not_implemented("divergence");
          if (m.screenRef) throw not_implemented("screenRef");
          r.set(i, m);
          lock[i] = m.channelLock.flag ? 1 : 0;
          lock_max[i] = m.channelLock.hasMaxDistance ? m.channelLock.maxDistance : std::numeric_limits<double>::infinity();
          div[i] = m.objectDivergence.divergence;
          range[i] = m.objectDivergence.isCartesian ? 45.0 : m.objectDivergence.range;
          if (!m.zoneExclusion.zones.empty()) {
            std::vector<earhip_exclusion_zone> zones;
            for (const ExclusionZone &z : m.zoneExclusion.zones) zones.push_back(ear::detail::to_c(z));
            check(earhip_objects_excluded_channels(layout_.name.c_str(), (int)zones.size(), zones.data(), &excluded[i]));
          }
        }
        std::vector<float> d(n * layout_.n_full), f(n * layout_.n_full);
        check(earhip_panner_calculate_objects(h_, n, r.az.data(), r.el.data(), r.dist.data(), r.width.data(), r.height.data(),
                                              r.depth.data(), r.gain.data(), r.diffuse.data(), lock.data(), lock_max.data(),
                                              div.data(), range.data(), excluded.data(), d.data(), f.data()));
        layout_.scatter(n, d.data(), directGains);
        layout_.scatter(n, f.data(), diffuseGains);
      }

     private:
      const ear::detail::LayoutBinding layout_;
      earhip_panner *h_ = nullptr;
    };
  }  // namespace hip
}  // namespace ear
