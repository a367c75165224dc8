// ear/conversion.hpp — libear's ear::conversion (include/ear/conversion.hpp:1-83) over earhip group K: the
// ITU-R BS.2127 section 10 conversion of Objects positions and extents between polar and Cartesian.  The
// single-element functions are libear's free functions, computed on the calling thread by the library's host
// forms (no device needed, as in libear).  The batch overloads convert a renderer's metadata in one device
// launch.  One difference from libear: a polar azimuth that is infinite or beyond +-2^40 degrees throws
// ear::invalid_argument, where libear's angle loops do not return.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "hip_batch.hpp"

namespace ear {
  namespace conversion {
    /// structure for holding extent parameters without using an entire ObjectsTypeMetadata object
    struct ExtentParams {
      double width;
      double height;
      double depth;
    };

    /// convert a Cartesian position to polar
    inline PolarPosition pointCartToPolar(const CartesianPosition &pos) {
      double az, el, d;
      hip::check(earhip_conversion_to_polar(1, &pos.X, &pos.Y, &pos.Z, nullptr, nullptr, nullptr, &az, &el, &d,
                                            nullptr, nullptr, nullptr));
      return PolarPosition(az, el, d);
    }

    /// convert a polar position to Cartesian
    inline CartesianPosition pointPolarToCart(const PolarPosition &pos) {
      double x, y, z;
      hip::check(earhip_conversion_to_cartesian(1, &pos.azimuth, &pos.elevation, &pos.distance, nullptr, nullptr,
                                                nullptr, &x, &y, &z, nullptr, nullptr, nullptr));
      return CartesianPosition(x, y, z);
    }

    /// convert a Cartesian position and extent parameters to polar
    inline std::pair<PolarPosition, ExtentParams> extentCartToPolar(const CartesianPosition &pos,
                                                                    const ExtentParams &extent) {
      double az, el, d;
      ExtentParams out;
      hip::check(earhip_conversion_to_polar(1, &pos.X, &pos.Y, &pos.Z, &extent.width, &extent.height, &extent.depth,
                                            &az, &el, &d, &out.width, &out.height, &out.depth));
      return {PolarPosition(az, el, d), out};
    }

    /// convert a polar position and extent parameters to Cartesian
    inline std::pair<CartesianPosition, ExtentParams> extentPolarToCart(const PolarPosition &pos,
                                                                        const ExtentParams &extent) {
      double x, y, z;
      ExtentParams out;
      hip::check(earhip_conversion_to_cartesian(1, &pos.azimuth, &pos.elevation, &pos.distance, &extent.width,
                                                &extent.height, &extent.depth, &x, &y, &z, &out.width, &out.height,
                                                &out.depth));
      return {CartesianPosition(x, y, z), out};
    }

    /// in-place conversion of Objects metadata to polar.  The cartesian flag is ignored: the type of the
    /// position decides.  Cartesian metadata is converted and the flag cleared; polar metadata only has its flag
    /// fixed up.
    inline void toPolar(ObjectsTypeMetadata &otm) {
      otm.cartesian = otm.position.isCartesian;
      if (otm.cartesian) {
        std::pair<PolarPosition, ExtentParams> res =
            extentCartToPolar(otm.position.cartesian, ExtentParams{otm.width, otm.height, otm.depth});
        otm.cartesian = false;
        otm.position = res.first;
        otm.width = res.second.width;
        otm.height = res.second.height;
        otm.depth = res.second.depth;
      }
    }

    /// in-place conversion of Objects metadata to Cartesian, the mirror image of toPolar
    inline void toCartesian(ObjectsTypeMetadata &otm) {
      otm.cartesian = otm.position.isCartesian;
      if (!otm.cartesian) {
        std::pair<CartesianPosition, ExtentParams> res =
            extentPolarToCart(otm.position.polar, ExtentParams{otm.width, otm.height, otm.depth});
        otm.cartesian = true;
        otm.position = res.first;
        otm.width = res.second.width;
        otm.height = res.second.height;
        otm.depth = res.second.depth;
      }
    }

    namespace detail {
      // the batch form: the elements that need converting go to the device in one launch, through buffers in
      // host memory the device reaches (a DeviceBatch), converted in place; the others have their flag fixed
      /// the arrays of convert_batch's block, in the order they are carved: positions and extents, converted in place
      struct Arrays {
        Arrays(ear::detail::Carver &c, size_t n) {
          for (double *&p : a) p = c.take<double>(n);
          status = c.take<int>(n);
        }
        double *a[6];
        int *status;
      };
      inline void convert_batch(std::vector<ObjectsTypeMetadata> &metadata, hip::Context &ctx, bool to_polar) {
        std::vector<size_t> idx;
        for (size_t i = 0; i < metadata.size(); i++) {
          ObjectsTypeMetadata &m = metadata[i];
          m.cartesian = m.position.isCartesian;
          if (m.cartesian == to_polar) idx.push_back(i);
        }
        const size_t n = idx.size();
        if (n == 0) return;
        const ear::detail::DeviceBatch<Arrays> batch(ctx, n);
        double *const *a = batch.arrays.a;
        int *status = batch.arrays.status;
        for (size_t j = 0; j < n; j++) {
          const ObjectsTypeMetadata &m = metadata[idx[j]];
          if (to_polar) {
            a[0][j] = m.position.cartesian.X, a[1][j] = m.position.cartesian.Y, a[2][j] = m.position.cartesian.Z;
          } else {
            a[0][j] = m.position.polar.azimuth, a[1][j] = m.position.polar.elevation;
            a[2][j] = m.position.polar.distance;
          }
          a[3][j] = m.width, a[4][j] = m.height, a[5][j] = m.depth;
        }
        // libear stops at the first failing element: so does the batch, before anything is written back
        batch.finish(to_polar ? earhip_conversion_to_polar_device(ctx.get(), n, a[0], a[1], a[2], a[3], a[4], a[5], a[0], a[1],
                                                                  a[2], a[3], a[4], a[5], status)
                              : earhip_conversion_to_cartesian_device(ctx.get(), n, a[0], a[1], a[2], a[3], a[4], a[5], a[0],
                                                                      a[1], a[2], a[3], a[4], a[5], status),
                     status, n, [&idx, status](size_t j) {
                       const bool azimuth = status[j] == EARHIP_INVALID_ARGUMENT;
                       return ear::detail::bad_block(
                           idx[j], azimuth ? "azimuth is infinite or beyond +-2^40 degrees" : "could not find sector", status[j]);
                     });
        for (size_t j = 0; j < n; j++) {
          ObjectsTypeMetadata &m = metadata[idx[j]];
          if (to_polar)
            m.position = PolarPosition(a[0][j], a[1][j], a[2][j]);
          else
            m.position = CartesianPosition(a[0][j], a[1][j], a[2][j]);
          m.cartesian = !to_polar;
          m.width = a[3][j], m.height = a[4][j], m.depth = a[5][j];
        }
      }
    }  // namespace detail

    /// toPolar over a batch of metadata blocks (all objects x blocks of a renderer) in one device launch
    inline void toPolar(std::vector<ObjectsTypeMetadata> &metadata, hip::Context &ctx) {
      detail::convert_batch(metadata, ctx, true);
    }
    /// toCartesian over a batch of metadata blocks in one device launch
    inline void toCartesian(std::vector<ObjectsTypeMetadata> &metadata, hip::Context &ctx) {
      detail::convert_batch(metadata, ctx, false);
    }
  }  // namespace conversion
}  // namespace ear
