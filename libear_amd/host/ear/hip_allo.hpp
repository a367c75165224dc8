// ear/hip_allo.hpp — a gain calculator for Objects blocks with Cartesian positions (cartesian == 1): the C++ face of group T
// of the C ABI (include/earhip.h, where the allocentric panner's gains are specified, after ITU-R BS.2127-0 7.3.10).  libear
// carries only a stub of this panner, and ear::GainCalculatorObjects and ear::hip::ObjectsGainCalculator keep refusing
// Cartesian blocks, so there is no libear class this one mirrors; it has the constructor and calculate overloads of
// ObjectsGainCalculator (hip_objects.hpp) and follows the conventions of the mirror classes (exceptions for status codes).
// It is pure host: only calculate_device, the batch form that runs one device launch, takes a Context.
#pragma once
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "gain_calculators.hpp"

namespace ear {
  namespace hip {
    class AllocentricGainCalculator {
     public:
      /// layout: an ITU-R BS.2051 layout (getLayout), with or without its LFE channels; its loudspeakers stand where the
      /// built-in table of group T puts them.  A layout of the caller's own has no table: not_implemented.
      explicit AllocentricGainCalculator(const Layout &layout) {
        std::vector<double> az, el;
        keep_ = ear::detail::match_layout(layout, name_, az, el);
        n_full_ = az.size();
        check(earhip_allo_create(name_.c_str(), &h_));
      }
      /// any layout, with the loudspeakers where the caller says: one position per channel of `layout`, in its order (those
      /// of LFE channels are ignored)
      AllocentricGainCalculator(const Layout &layout, const std::vector<CartesianPosition> &positions) {
        std::vector<double> az, el;
        keep_ = ear::detail::match_layout(layout, name_, az, el);
        n_full_ = az.size();
        if (positions.size() != keep_.size()) throw invalid_argument("one position per channel of the layout");
        // (a BS.2051 layout given without its LFE channels: the native creator ignores those rows, and refuses the NaN of
        // any other channel that is missing)
        const double none = std::numeric_limits<double>::quiet_NaN();
        std::vector<double> x(n_full_, none), y(n_full_, none), z(n_full_, none);
        for (size_t c = 0; c < keep_.size(); c++) x[keep_[c]] = positions[c].X, y[keep_[c]] = positions[c].Y, z[keep_[c]] = positions[c].Z;
        check(earhip_allo_create_positions(name_.c_str(), (int)n_full_, x.data(), y.data(), z.data(), &h_));
      }
      ~AllocentricGainCalculator() { earhip_allo_destroy(h_); }
      AllocentricGainCalculator(const AllocentricGainCalculator &) = delete;
      AllocentricGainCalculator &operator=(const AllocentricGainCalculator &) = delete;

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
      /// polar position or `cartesian == false`, width / height / depth, channelLock, a non-zero divergence, screenRef, a
      /// polar exclusion zone (for all but the last a Cartesian block still takes ear::conversion and the polar calculators).
      template <typename T>
      void calculate(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                     std::vector<std::vector<T>> &diffuseGains) const {
        Batch b = gather(metadata);
        const size_t n = metadata.size();
        std::vector<float> d(n * n_full_), f(n * n_full_);
        check(earhip_allo_calculate(h_, n, b.x.data(), b.y.data(), b.z.data(), b.gain.data(), b.diffuse.data(),
                                    b.excluded.data(), d.data(), f.data()));
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
        check(earhip_host_alloc(ctx.get(), n * (5 * sizeof(double) + sizeof(uint32_t) + sizeof(int) + 2 * n_full_ * sizeof(float)),
                                &mem));
        double *x = static_cast<double *>(mem), *y = x + n, *z = y + n, *gain = z + n, *diffuse = gain + n;
        uint32_t *excluded = reinterpret_cast<uint32_t *>(diffuse + n);
        int *status = reinterpret_cast<int *>(excluded + n);
        float *d = reinterpret_cast<float *>(status + n), *f = d + n * n_full_;
        for (size_t i = 0; i < n; i++) {
          x[i] = b.x[i], y[i] = b.y[i], z[i] = b.z[i], gain[i] = b.gain[i], diffuse[i] = b.diffuse[i];
          excluded[i] = b.excluded[i];
        }
        int st = earhip_allo_calculate_device(ctx.get(), h_, n, x, y, z, gain, diffuse, excluded, d, f, status);
        if (st == EARHIP_OK) st = earhip_ctx_synchronize(ctx.get());
        std::string msg = st == EARHIP_OK ? std::string() : std::string(earhip_last_error());
        for (size_t i = 0; i < n && st == EARHIP_OK; i++)
          if (status[i] != 0) {
            st = EARHIP_INVALID_ARGUMENT;
            msg = "metadata block " + std::to_string(i) + ": the position and the gain must be finite and the diffuse within [0, 1]";
          }
        if (st == EARHIP_OK) scatter(n, d, f, directGains, diffuseGains);
        earhip_host_release(ctx.get(), mem);
        check(st, msg);
      }

     private:
      struct Batch {
        std::vector<double> x, y, z, gain, diffuse;
        std::vector<uint32_t> excluded;
      };
      Batch gather(const std::vector<ObjectsTypeMetadata> &metadata) const {
        const size_t n = metadata.size();
        Batch b;
        b.x.resize(n), b.y.resize(n), b.z.resize(n), b.gain.resize(n), b.diffuse.resize(n), b.excluded.assign(n, 0);
        for (size_t i = 0; i < n; i++) {
          const ObjectsTypeMetadata &m = metadata[i];
          if (!m.position.isCartesian) throw not_implemented("position: polar");
          if (!m.cartesian) throw not_implemented("cartesian == false");
          if (m.width != 0.0) throw not_implemented("width");
          if (m.height != 0.0) throw not_implemented("height");
          if (m.depth != 0.0) throw not_implemented("depth");
          if (m.channelLock.flag) throw not_implemented("channelLock");
          if (m.objectDivergence.divergence != 0.0) throw not_implemented("divergence");
          if (m.screenRef) throw not_implemented("screenRef");
          b.x[i] = m.position.cartesian.X, b.y[i] = m.position.cartesian.Y, b.z[i] = m.position.cartesian.Z;
          b.gain[i] = m.gain, b.diffuse[i] = m.diffuse;
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
