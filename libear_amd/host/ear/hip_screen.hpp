// ear/hip_screen.hpp — screenRef scaling and screenEdgeLock of Objects metadata: the C++ face of group R of the C ABI
// (include/earhip.h, where both steps are specified).  libear refuses screenRef, and ear::GainCalculatorObjects and
// ear::hip::ObjectsGainCalculator keep refusing it, so there is no libear class this one mirrors: it is a stage of its own that
// hands back metadata with the position rewritten and screenRef cleared, the way ear::conversion::toPolar hands back polar
// metadata, and the calculators then accept the result.  It follows the conventions of the mirror classes (exceptions for
// status codes, a context argument that defaults to the process-wide one), as hip_objects.hpp and hip_hoa.hpp do.
//
// libear's Objects position has no screenEdgeLock field and the mirror keeps libear's schema, so the lock is an argument.
#pragma once
#include <array>
#include <cstddef>
#include <string>
#include <vector>

#include "hip_batch.hpp"

namespace ear {
  namespace hip {
    class ScreenHandler {
     public:
      /// no reproduction screen: every block passes through (screenRef is still cleared: there is nothing to scale to)
      ScreenHandler() : has_screen_(false), reproduction_(earhip_screen()) {}
      /// throws ear::invalid_argument for a screen group R refuses (e.g. one across the rear seam)
      explicit ScreenHandler(const Screen &reproduction) : has_screen_(true), reproduction_(to_c(reproduction)) {
        double e[4];
        check(earhip_screen_edges(&reproduction_, e));
      }

      /// left azimuth, right azimuth, bottom elevation, top elevation of a screen, degrees
      static std::array<double, 4> edges(const Screen &screen) {
        const earhip_screen s = to_c(screen);
        std::array<double, 4> e;
        check(earhip_screen_edges(&s, e.data()));
        return e;
      }

      /// one metadata block, on the calling thread (no device): scaled from m.referenceScreen to the reproduction screen when
      /// m.screenRef is set, then locked to the edges `lock` names ("left" / "right", "bottom" / "top").  Returns a copy with
      /// the position rewritten and screenRef = false.  Cartesian metadata throws not_implemented("cartesian"), as in the
      /// calculators: convert with ear::conversion::toPolar first.
      ObjectsTypeMetadata apply(const ObjectsTypeMetadata &m, const ScreenEdgeLock &lock = ScreenEdgeLock()) const {
        refuse(m);
        const unsigned char ref = m.screenRef ? 1 : 0, lh = horizontal_code(lock), lv = vertical_code(lock);
        const earhip_screen reference = to_c(m.referenceScreen);
        ObjectsTypeMetadata out = m;
        check(earhip_screen_apply(&reference, has_screen_ ? &reproduction_ : nullptr, 1, &m.position.polar.azimuth,
                                  &m.position.polar.elevation, &ref, &lh, &lv, &out.position.polar.azimuth,
                                  &out.position.polar.elevation));
        out.screenRef = false;
        return out;
      }

      /// a batch of metadata blocks (all objects x blocks of a renderer), rewritten in place on the device through buffers in
      /// host memory the device reaches: one launch per distinct reference screen (a programme has one).  locks: empty, or one
      /// per block.  A block the single form refuses throws here too, before anything is written.  The results are the bits
      /// of the single form.
      void apply(std::vector<ObjectsTypeMetadata> &metadata,
                 const std::vector<ScreenEdgeLock> &locks = std::vector<ScreenEdgeLock>(),
                 Context &ctx = default_context()) const {
        const size_t n = metadata.size();
        if (!locks.empty() && locks.size() != n) throw invalid_argument("locks must be empty or one per metadata block");
        std::vector<unsigned char> lh(n, 0), lv(n, 0);
        for (size_t i = 0; i < n; i++) {
          refuse(metadata[i]);
          if (!locks.empty()) lh[i] = horizontal_code(locks[i]), lv[i] = vertical_code(locks[i]);
        }
        if (n == 0) return;
        // the blocks grouped by reference screen, in order of first appearance
        std::vector<earhip_screen> screens;
        std::vector<size_t> group(n);
        for (size_t i = 0; i < n; i++) {
          const earhip_screen s = to_c(metadata[i].referenceScreen);
          size_t g = 0;
          while (g < screens.size() && !same(screens[g], s)) g++;
          if (g == screens.size()) screens.push_back(s);
          group[i] = g;
        }
        const ear::detail::DeviceBatch<Arrays> batch(ctx, n);
        const Arrays &a = batch.arrays;
        std::vector<size_t> idx(n);
        std::vector<size_t> first(screens.size() + 1, 0);
        size_t j = 0;
        for (size_t g = 0; g < screens.size(); g++) {
          first[g] = j;
          for (size_t i = 0; i < n; i++)
            if (group[i] == g) {
              const ObjectsTypeMetadata &m = metadata[i];
              idx[j] = i, a.az[j] = m.position.polar.azimuth, a.el[j] = m.position.polar.elevation;
              a.ref[j] = m.screenRef ? 1 : 0, a.h[j] = lh[i], a.v[j] = lv[i];
              j++;
            }
        }
        first[screens.size()] = n;
        int st = EARHIP_OK;
        for (size_t g = 0; g < screens.size() && st == EARHIP_OK; g++) {
          const size_t o = first[g];
          st = earhip_screen_apply_device(ctx.get(), &screens[g], has_screen_ ? &reproduction_ : nullptr, first[g + 1] - o,
                                          a.az + o, a.el + o, a.ref + o, a.h + o, a.v + o, a.az + o, a.el + o, a.status + o);
        }
        batch.finish(st, a.status, n, [&idx](size_t k) {
          return ear::detail::bad_block(idx[k], "azimuth and elevation must be finite, the azimuth within +-2^40 and the "
                                                "elevation within +-90 degrees");
        });
        for (size_t k = 0; k < n; k++) {
          ObjectsTypeMetadata &m = metadata[idx[k]];
          m.position.polar.azimuth = a.az[k], m.position.polar.elevation = a.el[k];
          m.screenRef = false;
        }
      }

      /// the arrays of the batch form's block, in the order they are carved
      struct Arrays {
        Arrays(ear::detail::Carver &c, size_t n)
            : az(c.take<double>(n)), el(c.take<double>(n)), status(c.take<int>(n)), ref(c.take<unsigned char>(n)),
              h(c.take<unsigned char>(n)), v(c.take<unsigned char>(n)) {}
        double *az, *el;
        int *status;
        unsigned char *ref, *h, *v;
      };

     private:
      static earhip_screen to_c(const Screen &s) {
        earhip_screen c = earhip_screen();
        c.cartesian = s.isCartesian ? 1 : 0;
        if (s.isCartesian) {
          c.aspect_ratio = s.cartesian.aspectRatio, c.width_x = s.cartesian.widthX;
          c.x = s.cartesian.centrePosition.X, c.y = s.cartesian.centrePosition.Y, c.z = s.cartesian.centrePosition.Z;
        } else {
          c.aspect_ratio = s.polar.aspectRatio, c.width_azimuth = s.polar.widthAzimuth;
          c.azimuth = s.polar.centrePosition.azimuth, c.elevation = s.polar.centrePosition.elevation;
          c.distance = s.polar.centrePosition.distance;
        }
        return c;
      }
      // (to_c zeroes the fields of the other kind, so equal screens have equal fields)
      static bool same(const earhip_screen &a, const earhip_screen &b) {
        return a.cartesian == b.cartesian && a.aspect_ratio == b.aspect_ratio && a.azimuth == b.azimuth &&
               a.elevation == b.elevation && a.distance == b.distance && a.x == b.x && a.y == b.y && a.z == b.z &&
               a.width_azimuth == b.width_azimuth && a.width_x == b.width_x;
      }
      static void refuse(const ObjectsTypeMetadata &m) {
        if (m.cartesian || m.position.isCartesian) throw not_implemented("cartesian");
      }
      static unsigned char horizontal_code(const ScreenEdgeLock &lock) {
        if (!lock.horizontal) return 0;
        if (*lock.horizontal == "left") return 1;
        if (*lock.horizontal == "right") return 2;
        throw adm_error("invalid horizontal screenEdgeLock: '" + *lock.horizontal + "' (left or right)");
      }
      static unsigned char vertical_code(const ScreenEdgeLock &lock) {
        if (!lock.vertical) return 0;
        if (*lock.vertical == "bottom") return 1;
        if (*lock.vertical == "top") return 2;
        throw adm_error("invalid vertical screenEdgeLock: '" + *lock.vertical + "' (bottom or top)");
      }

      bool has_screen_;
      earhip_screen reproduction_;
    };
  }  // namespace hip
}  // namespace ear
