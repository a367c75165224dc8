// ear/hip_hoa.hpp — an Ambisonic encoder for Objects metadata and the rotation of the HOA bus: the C++ face of group Q of the
// C ABI (include/earhip.h, where the encoded value and the rotation matrix are specified).  libear renders scene-based content
// to loudspeakers (GainCalculatorHOA) but has no way into the scene-based domain, so there is no libear class this one
// mirrors; it follows the conventions of the mirror classes (exceptions for status codes, a context argument that defaults to
// the process-wide one), as hip_objects.hpp and hip_src.hpp do.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "hip_batch.hpp"

namespace ear {
  namespace hip {
    class HOAEncoder {
     public:
      /// one (order, degree) pair per channel of the bus (at most 64, orders up to 7); normalization "SN3D", "N3D" or "FuMa"
      HOAEncoder(const std::vector<int> &orders, const std::vector<int> &degrees, const std::string &normalization = "SN3D")
          : orders_(orders), degrees_(degrees), norm_(normalization) {
        if (orders_.size() != degrees_.size()) throw invalid_argument("orders and degrees must be the same size");
        // (checks the channel list and the normalization now, not at the first calculate)
        std::vector<float> row(orders_.size() ? orders_.size() : 1);
        const double zero = 0.0;
        check(earhip_hoa_encode((int)orders_.size(), orders_.data(), degrees_.data(), norm_.c_str(), 1, &zero, &zero, nullptr,
                                row.data()));
      }
      size_t num_channels() const { return orders_.size(); }

      /// one metadata block -> its gain vector on the bus (resized to the channel count), on the calling thread: no device
      template <typename T>
      void calculate(const ObjectsTypeMetadata &metadata, std::vector<T> &gains) const {
        refuse(metadata);
        std::vector<float> row(orders_.size());
        check(earhip_hoa_encode((int)orders_.size(), orders_.data(), degrees_.data(), norm_.c_str(), 1,
                                &metadata.position.polar.azimuth, &metadata.position.polar.elevation, &metadata.gain,
                                row.data()));
        gains.assign(row.begin(), row.end());
      }

      /// a batch of metadata blocks (all objects x blocks of a renderer) in one device launch, through buffers in host memory
      /// the device reaches.  A block the single form refuses throws here too, before anything is written.
      template <typename T>
      void calculate(const std::vector<ObjectsTypeMetadata> &metadata, std::vector<std::vector<T>> &gains,
                     Context &ctx = default_context()) const {
        const size_t n = metadata.size(), nc = orders_.size();
        for (size_t i = 0; i < n; i++) refuse(metadata[i]);
        gains.assign(n, std::vector<T>(nc));
        if (n == 0) return;
        const ear::detail::DeviceBatch<Arrays> batch(ctx, n, nc);
        const Arrays &a = batch.arrays;
        for (size_t i = 0; i < n; i++) {
          a.az[i] = metadata[i].position.polar.azimuth, a.el[i] = metadata[i].position.polar.elevation;
          a.gain[i] = metadata[i].gain;
        }
        batch.finish(earhip_hoa_encode_device(ctx.get(), (int)nc, orders_.data(), degrees_.data(), norm_.c_str(), n, a.az, a.el,
                                              a.gain, a.out, a.status),
                     a.status, n, [](size_t i) {
                       return ear::detail::bad_block(
                           i, "azimuth, elevation and gain must be finite and the elevation within +-90 degrees");
                     });
        for (size_t i = 0; i < n; i++)
          for (size_t c = 0; c < nc; c++) gains[i][c] = (T)a.out[i * nc + c];
      }

      /// R [n_coef][n_coef] with encode(q u) = R encode(u): q is a proper rotation, row-major, acting on ADM Cartesian
      /// column vectors (x right, y front, z up).  Apply a static one with GainInterpolator / earhip_interp_apply_constant
      /// (point[in][out] = R[out][in]), a head-tracked one as interpolation points.
      template <typename T = float>
      std::vector<std::vector<T>> rotation(const double q[9]) const {
        const size_t nc = orders_.size();
        std::vector<float> r(nc * nc);
        check(earhip_hoa_rotation_matrix((int)nc, orders_.data(), degrees_.data(), norm_.c_str(), q, r.data()));
        std::vector<std::vector<T>> out(nc, std::vector<T>(nc));
        for (size_t i = 0; i < nc; i++)
          for (size_t j = 0; j < nc; j++) out[i][j] = (T)r[i * nc + j];
        return out;
      }

      /// the arrays of the batch form's block, in the order they are carved
      struct Arrays {
        Arrays(ear::detail::Carver &c, size_t n, size_t nc)
            : az(c.take<double>(n)), el(c.take<double>(n)), gain(c.take<double>(n)), out(c.take<float>(n * nc)),
              status(c.take<int>(n)) {}
        double *az, *el, *gain;
        float *out;
        int *status;
      };

     private:
      // The bus has no diffuse path and the encoder no extent, lock, divergence or zones: a field it would have to drop
      // silently is refused, as libear's gain calculators refuse what they do not render.
      static void refuse(const ObjectsTypeMetadata &m) {
        if (m.cartesian || m.position.isCartesian) throw not_implemented("cartesian");
        if (m.width != 0.0 || m.height != 0.0 || m.depth != 0.0) throw not_implemented("extent");
        if (m.diffuse != 0.0) throw not_implemented("diffuse");
        if (m.channelLock.flag) throw not_implemented("channelLock");
        if (m.objectDivergence.divergence != 0.0) throw not_implemented("divergence");
        if (!m.zoneExclusion.zones.empty()) throw not_implemented("zoneExclusion");
        if (m.screenRef) throw not_implemented("screenRef");
      }

      std::vector<int> orders_, degrees_;
      std::string norm_;
    };
  }  // namespace hip
}  // namespace ear
