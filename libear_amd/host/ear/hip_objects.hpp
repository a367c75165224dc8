// ear/hip_objects.hpp — an Objects gain calculator that carries channelLock, polar objectDivergence and zoneExclusion: the
// C++ face of the _objects forms of group I of the C ABI (include/earhip.h, where the three are specified).  libear refuses
// these fields (src/object_based/gain_calculator_objects.cpp:37-44) and ear::GainCalculatorObjects keeps refusing them, so
// there is no libear class this one mirrors; it has that class's constructor and calculate overloads and follows the
// conventions of the mirror classes (exceptions for status codes, a context argument that defaults to the process-wide one),
// as hip_iir.hpp and hip_src.hpp do.
#pragma once
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "gain_calculators.hpp"

namespace ear {
  namespace hip {
    class ObjectsGainCalculator {
     public:
      /// layout: an ITU-R BS.2051 layout (getLayout), with or without its LFE channels, or a layout of the caller's own
      explicit ObjectsGainCalculator(const Layout &layout, Context &ctx = default_context()) {
        std::vector<double> az, el;
        keep_ = ear::detail::match_layout(layout, name_, az, el);
        n_full_ = az.size();
        check(earhip_panner_create_positions(ctx.get(), name_.c_str(), (int)n_full_, az.data(), el.data(), &h_));
      }
      ~ObjectsGainCalculator() { earhip_panner_destroy(h_); }
      ObjectsGainCalculator(const ObjectsGainCalculator &) = delete;
      ObjectsGainCalculator &operator=(const ObjectsGainCalculator &) = delete;

      /// one metadata block -> direct and diffuse gain vectors, which must have the layout's channel count
      template <typename T>
      void calculate(const ObjectsTypeMetadata &metadata, std::vector<T> &directGains, std::vector<T> &diffuseGains,
                     const WarningCB & = default_warning_cb) {
        if (directGains.size() != keep_.size() || diffuseGains.size() != keep_.size())
          throw invalid_argument("incorrect size for output vector");
        std::vector<std::vector<T>> d, f;
        calculate(std::vector<ObjectsTypeMetadata>(1, metadata), d, f);
        directGains = d[0];
        diffuseGains = f[0];
      }
      /// a batch of metadata blocks in one device call.  Still refused, with libear's messages: Cartesian positions and
      /// `cartesian`, a non-zero CartesianObjectDivergence, screenRef.
      template <typename T>
      void calculate(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                     std::vector<std::vector<T>> &diffuseGains) {
        const size_t n = metadata.size();
        std::vector<double> az(n), el(n), dist(n), gain(n), diffuse(n), width(n), height(n), depth(n), lock_max(n), div(n),
            range(n);
        std::vector<unsigned char> lock(n);
        std::vector<uint32_t> excluded(n, 0);
        for (size_t i = 0; i < n; i++) {
          const ObjectsTypeMetadata &m = metadata[i];
          if (m.cartesian || m.position.isCartesian) throw not_implemented("cartesian");
          if (m.objectDivergence.isCartesian && m.objectDivergence.divergence != 0.0) throw not_implemented("divergence");
          if (m.screenRef) throw not_implemented("screenRef");
          az[i] = m.position.polar.azimuth, el[i] = m.position.polar.elevation, dist[i] = m.position.polar.distance;
          width[i] = m.width, height[i] = m.height, depth[i] = m.depth;
          gain[i] = m.gain, diffuse[i] = m.diffuse;
          lock[i] = m.channelLock.flag ? 1 : 0;
          lock_max[i] = m.channelLock.hasMaxDistance ? m.channelLock.maxDistance : std::numeric_limits<double>::infinity();
          div[i] = m.objectDivergence.divergence;
          range[i] = m.objectDivergence.isCartesian ? 45.0 : m.objectDivergence.range;
          if (!m.zoneExclusion.zones.empty()) {
            std::vector<earhip_exclusion_zone> zones;
            for (const ExclusionZone &z : m.zoneExclusion.zones) {
              earhip_exclusion_zone c = earhip_exclusion_zone();
              c.cartesian = z.isCartesian;
              c.min_azimuth = z.polar.minAzimuth, c.max_azimuth = z.polar.maxAzimuth;
              c.min_elevation = z.polar.minElevation, c.max_elevation = z.polar.maxElevation;
              c.min_x = z.cartesian.minX, c.max_x = z.cartesian.maxX;
              c.min_y = z.cartesian.minY, c.max_y = z.cartesian.maxY;
              c.min_z = z.cartesian.minZ, c.max_z = z.cartesian.maxZ;
              zones.push_back(c);
            }
            check(earhip_objects_excluded_channels(name_.c_str(), (int)zones.size(), zones.data(), &excluded[i]));
          }
        }
        std::vector<float> d(n * n_full_), f(n * n_full_);
        check(earhip_panner_calculate_objects(h_, n, az.data(), el.data(), dist.data(), width.data(), height.data(), depth.data(),
                                              gain.data(), diffuse.data(), lock.data(), lock_max.data(), div.data(), range.data(),
                                              excluded.data(), d.data(), f.data()));
        directGains.assign(n, std::vector<T>(keep_.size()));
        diffuseGains.assign(n, std::vector<T>(keep_.size()));
        for (size_t i = 0; i < n; i++)
          for (size_t c = 0; c < keep_.size(); c++) {
            directGains[i][c] = (T)d[i * n_full_ + keep_[c]];
            diffuseGains[i][c] = (T)f[i * n_full_ + keep_[c]];
          }
      }

     private:
      std::string name_;
      earhip_panner *h_ = nullptr;
      std::vector<int> keep_;
      size_t n_full_ = 0;
    };
  }  // namespace hip
}  // namespace ear
