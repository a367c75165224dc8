// ear/hip_allo_objects.hpp — the gain calculator for every Objects block with Cartesian positions (cartesian == 1) but
// screenRef: the C++ face of group U of the C ABI (include/earhip.h, where the gains are specified, after ITU-R BS.2127-0
// 7.3.6, 7.3.7, 7.3.10 and 7.3.11).  Beyond AllocentricGainCalculator (hip_allo.hpp), whose constructors and calculate /
// calculate_device overloads it has, it takes width, height and depth, channelLock (flag and maxDistance) and
// CartesianObjectDivergence.  libear carries only a stub of this panner, so there is no libear class this one mirrors.  It is
// pure host: only calculate_device, the batch form that runs one device launch, takes a Context.
#pragma once
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "gain_calculators.hpp"

namespace ear {
  namespace hip {
    class AllocentricObjectsGainCalculator {
     public:
      /// layout: an ITU-R BS.2051 layout (getLayout), with or without its LFE channels; its loudspeakers stand where the
      /// built-in table of group T puts them.  A layout of the caller's own has no table: not_implemented.
      explicit AllocentricObjectsGainCalculator(const Layout &layout) {
        std::vector<double> az, el;
        keep_ = ear::detail::match_layout(layout, name_, az, el);
        n_full_ = az.size();
        check(earhip_allo_create(name_.c_str(), &h_));
      }
      /// any layout, with the loudspeakers where the caller says: one position per channel of `layout`, in its order (those
      /// of LFE channels are ignored)
      AllocentricObjectsGainCalculator(const Layout &layout, const std::vector<CartesianPosition> &positions) {
        std::vector<double> az, el;
        keep_ = ear::detail::match_layout(layout, name_, az, el);
        n_full_ = az.size();
        if (positions.size() != keep_.size()) throw invalid_argument("one position per channel of the layout");
        const double none = std::numeric_limits<double>::quiet_NaN();
        std::vector<double> x(n_full_, none), y(n_full_, none), z(n_full_, none);
        for (size_t c = 0; c < keep_.size(); c++) x[keep_[c]] = positions[c].X, y[keep_[c]] = positions[c].Y, z[keep_[c]] = positions[c].Z;
        check(earhip_allo_create_positions(name_.c_str(), (int)n_full_, x.data(), y.data(), z.data(), &h_));
      }
      ~AllocentricObjectsGainCalculator() { earhip_allo_destroy(h_); }
      AllocentricObjectsGainCalculator(const AllocentricObjectsGainCalculator &) = delete;
      AllocentricObjectsGainCalculator &operator=(const AllocentricObjectsGainCalculator &) = delete;

      /// one metadata block -> direct and diffuse gain vectors, which must have the layout's channel count
      template <typename T>
      void calculate(const ObjectsTypeMetadata &metadata, std::vector<T> &directGains, std::vector<T> &diffuseGains,
                     const WarningCB & = default_warning_cb) const {
        if (directGains.size() != keep_.size() || diffuseGains.size() != keep_.size())
          throw invalid_argument("incorrect size for output vector");
        std::vector<std::vector<T>> d, f;
        calculate(std::vector<ObjectsTypeMetadata>(1, metadata), d, f);
        directGains = d[0];
        diffuseGains = f[0];
      }
      /// a batch of metadata blocks, on the calling thread.  Refused with not_implemented, the message naming the field: a
      /// polar position or `cartesian == false`, a non-zero PolarObjectDivergence, screenRef (such a block still takes
      /// ear::conversion and the polar calculators), a polar exclusion zone.
      template <typename T>
      void calculate(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                     std::vector<std::vector<T>> &diffuseGains) const {
        Batch b = gather(metadata);
        const size_t n = metadata.size();
        std::vector<float> d(n * n_full_), f(n * n_full_);
        check(earhip_allo_calculate_objects(h_, n, b.v[0].data(), b.v[1].data(), b.v[2].data(), b.v[3].data(), b.v[4].data(),
                                            b.v[5].data(), b.v[6].data(), b.v[7].data(), b.lock.data(), b.v[8].data(),
                                            b.v[9].data(), b.v[10].data(), b.excluded.data(), d.data(), f.data()));
        scatter(n, d.data(), f.data(), directGains, diffuseGains);
      }
      /// the same batch in one device launch, through buffers in host memory the device reaches.  A block the host form
      /// refuses throws here too, before anything is written.
      template <typename T>
      void calculate_device(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                            std::vector<std::vector<T>> &diffuseGains, Context &ctx = default_context()) const {
        const Batch b = gather(metadata);
        const size_t n = metadata.size();
        if (n == 0) {
          directGains.clear(), diffuseGains.clear();
          return;
        }
        void *mem = nullptr;
        check(earhip_host_alloc(ctx.get(), n * (kDoubles * sizeof(double) + sizeof(uint32_t) + sizeof(int) +
                                                2 * n_full_ * sizeof(float) + 1), &mem));
        double *v[kDoubles];
        for (int k = 0; k < kDoubles; k++) {
          v[k] = static_cast<double *>(mem) + k * n;
          for (size_t i = 0; i < n; i++) v[k][i] = b.v[k][i];
        }
        uint32_t *excluded = reinterpret_cast<uint32_t *>(v[kDoubles - 1] + n);
        int *status = reinterpret_cast<int *>(excluded + n);
        float *d = reinterpret_cast<float *>(status + n), *f = d + n * n_full_;
        unsigned char *lock = reinterpret_cast<unsigned char *>(f + n * n_full_);
        for (size_t i = 0; i < n; i++) excluded[i] = b.excluded[i], lock[i] = b.lock[i];
        int st = earhip_allo_calculate_objects_device(ctx.get(), h_, n, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], lock, v[8],
                                                      v[9], v[10], excluded, d, f, status);
        if (st == EARHIP_OK) st = earhip_ctx_synchronize(ctx.get());
        std::string msg = st == EARHIP_OK ? std::string() : std::string(earhip_last_error());
        for (size_t i = 0; i < n && st == EARHIP_OK; i++)
          if (status[i] != 0) {
            st = EARHIP_INVALID_ARGUMENT;
            msg = "metadata block " + std::to_string(i) + ": the position and the gain must be finite, the sizes, the "
                  "positionRange and the maxDistance not negative, the diffuse and the divergence within [0, 1]";
          }
        if (st == EARHIP_OK) scatter(n, d, f, directGains, diffuseGains);
        earhip_host_release(ctx.get(), mem);
        check(st, msg);
      }

     private:
      // the double arrays of the C ABI, in its order: x, y, z, width, height, depth, gain, diffuse, lock_max_distance,
      // divergence, position_range
      enum { kDoubles = 11 };
      struct Batch {
        std::vector<double> v[kDoubles];
        std::vector<unsigned char> lock;
        std::vector<uint32_t> excluded;
      };
      Batch gather(const std::vector<ObjectsTypeMetadata> &metadata) const {
        const size_t n = metadata.size();
        Batch b;
        for (std::vector<double> &a : b.v) a.resize(n);
        b.lock.assign(n, 0), b.excluded.assign(n, 0);
        for (size_t i = 0; i < n; i++) {
          const ObjectsTypeMetadata &m = metadata[i];
          if (!m.position.isCartesian) throw not_implemented("position: polar");
          if (!m.cartesian) throw not_implemented("cartesian == false");
          if (!m.objectDivergence.isCartesian && m.objectDivergence.divergence != 0.0)
            throw not_implemented("objectDivergence: polar");
          if (m.screenRef) throw not_implemented("screenRef");
          b.v[0][i] = m.position.cartesian.X, b.v[1][i] = m.position.cartesian.Y, b.v[2][i] = m.position.cartesian.Z;
          b.v[3][i] = m.width, b.v[4][i] = m.height, b.v[5][i] = m.depth;
          b.v[6][i] = m.gain, b.v[7][i] = m.diffuse;
          b.lock[i] = m.channelLock.flag ? 1 : 0;
          b.v[8][i] = m.channelLock.hasMaxDistance ? m.channelLock.maxDistance : std::numeric_limits<double>::infinity();
          b.v[9][i] = m.objectDivergence.divergence;
          b.v[10][i] = m.objectDivergence.isCartesian ? m.objectDivergence.range : 0.0;
          if (!m.zoneExclusion.zones.empty()) {
            std::vector<earhip_exclusion_zone> zones;
            for (const ExclusionZone &zn : m.zoneExclusion.zones) {
              if (!zn.isCartesian) throw not_implemented("zoneExclusion: polar zone");
              earhip_exclusion_zone c = earhip_exclusion_zone();
              c.cartesian = 1;
              c.min_x = zn.cartesian.minX, c.max_x = zn.cartesian.maxX;
              c.min_y = zn.cartesian.minY, c.max_y = zn.cartesian.maxY;
              c.min_z = zn.cartesian.minZ, c.max_z = zn.cartesian.maxZ;
              zones.push_back(c);
            }
            check(earhip_allo_excluded_channels(h_, (int)zones.size(), zones.data(), &b.excluded[i]));
          }
        }
        return b;
      }
      template <typename T>
      void scatter(size_t n, const float *d, const float *f, std::vector<std::vector<T>> &directGains,
                   std::vector<std::vector<T>> &diffuseGains) const {
        directGains.assign(n, std::vector<T>(keep_.size()));
        diffuseGains.assign(n, std::vector<T>(keep_.size()));
        for (size_t i = 0; i < n; i++)
          for (size_t c = 0; c < keep_.size(); c++) {
            directGains[i][c] = (T)d[i * n_full_ + keep_[c]];
            diffuseGains[i][c] = (T)f[i * n_full_ + keep_[c]];
          }
      }

      std::string name_;
      earhip_allo *h_ = nullptr;
      std::vector<int> keep_;
      size_t n_full_ = 0;
    };
  }  // namespace hip
}  // namespace ear
