// ear/hip_allo_objects.hpp — the gain calculator for every Objects block with Cartesian positions (cartesian == 1), behind
// ear::hip::ScreenHandler::apply_cartesian where it has screenRef: the C++ face of group U of the C ABI (include/earhip.h, where the gains are specified, after ITU-R BS.2127-0
// 7.3.6, 7.3.7, 7.3.10 and 7.3.11).  Beyond AllocentricGainCalculator (hip_allo.hpp), whose constructors and calculate /
// calculate_device overloads it has, it takes width, height and depth, channelLock (flag and maxDistance) and
// CartesianObjectDivergence.  libear carries only a stub of this panner, so there is no libear class this one mirrors.  It is
// pure host: only calculate_device, the batch form that runs one device launch, takes a Context.
#pragma once
#include <cstdint>
#include <vector>

#include "gain_calculators.hpp"

namespace ear {
  namespace hip {
    class AllocentricObjectsGainCalculator {
     public:
      /// layout: an ITU-R BS.2051 layout (getLayout), with or without its LFE channels; its loudspeakers stand where the
      /// built-in table of group T puts them.  A layout of the caller's own has no table: not_implemented.
      explicit AllocentricObjectsGainCalculator(const Layout &layout) : allo_(layout) {}
      /// any layout, with the loudspeakers where the caller says: one position per channel of `layout`, in its order (those
      /// of LFE channels are ignored)
      AllocentricObjectsGainCalculator(const Layout &layout, const std::vector<CartesianPosition> &positions)
          : allo_(layout, positions) {}

      /// one metadata block -> direct and diffuse gain vectors, which must have the layout's channel count
      template <typename T>
      void calculate(const ObjectsTypeMetadata &metadata, std::vector<T> &directGains, std::vector<T> &diffuseGains,
                     const WarningCB & = default_warning_cb) const {
        ear::detail::calculate_one(*this, allo_.layout, metadata, directGains, diffuseGains);
      }
      /// a batch of metadata blocks, on the calling thread.  Refused with not_implemented, the message naming the field: a
      /// polar position or `cartesian == false`, a non-zero PolarObjectDivergence, screenRef (ear::hip::ScreenHandler::apply_cartesian comes first
      /// and clears it), a polar exclusion zone.
      template <typename T>
      void calculate(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &directGains,
                     std::vector<std::vector<T>> &diffuseGains) const {
        const Rows b = allo_.gather(metadata, refuse);
        const size_t n = metadata.size(), n_full = allo_.layout.n_full;
        std::vector<float> d(n * n_full), f(n * n_full);
        check(earhip_allo_calculate_objects(allo_.get(), n, b.v[0].data(), b.v[1].data(), b.v[2].data(), b.v[3].data(),
                                            b.v[4].data(), b.v[5].data(), b.v[6].data(), b.v[7].data(), b.lock.data(),
                                            b.v[8].data(), b.v[9].data(), b.v[10].data(), b.excluded.data(), d.data(), f.data()));
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
        double *const *v = a.v;
        for (size_t i = 0; i < n; i++) {
          for (int k = 0; k < Rows::kDoubles; k++) v[k][i] = b.v[k][i];
          a.excluded[i] = b.excluded[i], a.lock[i] = b.lock[i];
        }
        batch.finish(earhip_allo_calculate_objects_device(ctx.get(), allo_.get(), n, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7],
                                                          a.lock, v[8], v[9], v[10], a.excluded, a.d, a.f, a.status),
                     a.status, n, [](size_t i) {
                       return ear::detail::bad_block(i, "the position and the gain must be finite, the sizes, the positionRange "
                                                        "and the maxDistance not negative, the diffuse and the divergence within "
                                                        "[0, 1]");
                     });
        allo_.layout.scatter(n, a.d, directGains);
        allo_.layout.scatter(n, a.f, diffuseGains);
      }

      /// the arrays of calculate_device's block, in the order they are carved (v: as AlloHandle::Rows::v)
      struct Arrays {
        Arrays(ear::detail::Carver &c, size_t n, size_t n_full) {
          for (double *&p : v) p = c.take<double>(n);
          excluded = c.take<uint32_t>(n), status = c.take<int>(n);
          d = c.take<float>(n * n_full), f = c.take<float>(n * n_full);
          lock = c.take<unsigned char>(n);
        }
        double *v[ear::detail::AlloHandle::Rows::kDoubles];
        uint32_t *excluded;
        int *status;
        float *d, *f;
        unsigned char *lock;
      };

     private:
      typedef ear::detail::AlloHandle::Rows Rows;
      static void refuse(const ObjectsTypeMetadata &m) {
        if (!m.position.isCartesian) throw not_implemented("position: polar");
        if (!m.cartesian) throw not_implemented("cartesian == false");
        if (!m.objectDivergence.isCartesian && m.objectDivergence.divergence != 0.0)
          throw not_implemented("objectDivergence: polar");
        if (m.screenRef) throw not_implemented("screenRef");
      }

      const ear::detail::AlloHandle allo_;
    };
  }  // namespace hip
}  // namespace ear
