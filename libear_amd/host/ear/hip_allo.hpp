// ear/hip_allo.hpp — a gain calculator for Objects blocks with Cartesian positions (cartesian == 1): the C++ face of group T
// of the C ABI (include/earhip.h, where the allocentric panner's gains are specified, after ITU-R BS.2127-0 7.3.10).  libear
// carries only a stub of this panner, and ear::GainCalculatorObjects and ear::hip::ObjectsGainCalculator keep refusing
// Cartesian blocks, so there is no libear class this one mirrors; it has the constructor and calculate overloads of
// ObjectsGainCalculator (hip_objects.hpp) and follows the conventions of the mirror classes (exceptions for status codes).
// It is pure host: only calculate_device, the batch form that runs one device launch, takes a Context.
// This class is the point-source form; AllocentricObjectsGainCalculator (hip_allo_objects.hpp, group U) also takes extent,
// channelLock and CartesianObjectDivergence.
#pragma once
#include <cstdint>
#include <vector>

#include "gain_calculators.hpp"

namespace ear {
  namespace hip {
    class AllocentricGainCalculator {
     public:
      /// layout: an ITU-R BS.2051 layout (getLayout), with or without its LFE channels; its loudspeakers stand where the
      /// built-in table of group T puts them.  A layout of the caller's own has no table: not_implemented.
      explicit AllocentricGainCalculator(const Layout &layout) : allo_(layout) {}
      /// any layout, with the loudspeakers where the caller says: one position per channel of `layout`, in its order (those
      /// of LFE channels are ignored)
      AllocentricGainCalculator(const Layout &layout, const std::vector<CartesianPosition> &positions) : allo_(layout, positions) {}

      /// one metadata block -> direct and diffuse gain vectors, which must have the layout's channel count
      template <typename T>
      void calculate(const ObjectsTypeMetadata &metadata, std::vector<T> &directGains, std::vector<T> &diffuseGains,
                     const WarningCB & = default_warning_cb) const {
        ear::detail::calculate_one(*this, allo_.layout, metadata, directGains, diffuseGains);
      }
      /// a batch of metadata blocks, on the calling thread.  Refused with not_implemented, the message naming the field: a
      /// polar position or `cartesian == false`, width / height / depth, channelLock, a non-zero divergence, screenRef, a
      /// polar exclusion zone (for all but the last a Cartesian block still takes ear::conversion and the polar calculators).
      template <typename T>
      void calculate(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                     std::vector<std::vector<T>> &diffuseGains) const {
        const Rows b = allo_.gather(metadata, refuse);
        const size_t n = metadata.size(), n_full = allo_.layout.n_full;
        std::vector<float> d(n * n_full), f(n * n_full);
        check(earhip_allo_calculate(allo_.get(), n, b.v[Rows::X].data(), b.v[Rows::Y].data(), b.v[Rows::Z].data(),
                                    b.v[Rows::GAIN].data(), b.v[Rows::DIFFUSE].data(), b.excluded.data(), d.data(), f.data()));
        allo_.layout.scatter(n, d.data(), directGains);
        allo_.layout.scatter(n, f.data(), diffuseGains);
      }
      /// the same batch in one device launch, through buffers in host memory the device reaches.  A block the host form
      /// refuses throws here too, before anything is written.
      template <typename T>
      void calculate_device(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                            std::vector<std::vector<T>> &diffuseGains, Context &ctx = default_context()) const {
        const Rows b = allo_.gather(metadata, refuse);
        const size_t n = metadata.size();
        if (n == 0) return directGains.clear(), diffuseGains.clear();
        const ear::detail::DeviceBatch<Arrays> batch(ctx, n, allo_.layout.n_full);
        const Arrays &a = batch.arrays;
        for (size_t i = 0; i < n; i++) {
          a.x[i] = b.v[Rows::X][i], a.y[i] = b.v[Rows::Y][i], a.z[i] = b.v[Rows::Z][i];
          a.gain[i] = b.v[Rows::GAIN][i], a.diffuse[i] = b.v[Rows::DIFFUSE][i], a.excluded[i] = b.excluded[i];
        }
        batch.finish(earhip_allo_calculate_device(ctx.get(), allo_.get(), n, a.x, a.y, a.z, a.gain, a.diffuse, a.excluded, a.d,
                                                  a.f, a.status),
                     a.status, n, [](size_t i) {
                       return ear::detail::bad_block(i, "the position and the gain must be finite and the diffuse within [0, 1]");
                     });
        allo_.layout.scatter(n, a.d, directGains);
        allo_.layout.scatter(n, a.f, diffuseGains);
      }

      /// the arrays of calculate_device's block, in the order they are carved
      struct Arrays {
        Arrays(ear::detail::Carver &c, size_t n, size_t n_full)
            : x(c.take<double>(n)), y(c.take<double>(n)), z(c.take<double>(n)), gain(c.take<double>(n)),
              diffuse(c.take<double>(n)), excluded(c.take<uint32_t>(n)), status(c.take<int>(n)), d(c.take<float>(n * n_full)),
              f(c.take<float>(n * n_full)) {}
        double *x, *y, *z, *gain, *diffuse;
        uint32_t *excluded;
        int *status;
        float *d, *f;
      };

     private:
      typedef ear::detail::AlloHandle::Rows Rows;
      static void refuse(const ObjectsTypeMetadata &m) {
        if (!m.position.isCartesian) throw not_implemented("position: polar");
        if (!m.cartesian) throw not_implemented("cartesian == false");
        if (m.width != 0.0) throw not_implemented("width");
        if (m.height != 0.0) throw not_implemented("height");
        if (m.depth != 0.0) throw not_implemented("depth");
        if (m.channelLock.flag) throw not_implemented("channelLock");
        if (m.objectDivergence.divergence != 0.0) throw not_implemented("divergence");
        if (m.screenRef) throw not_implemented("screenRef");
      }

      const ear::detail::AlloHandle allo_;
    };
  }  // namespace hip
}  // namespace ear
