// ear/hip_screen.hpp — screenRef scaling and screenEdgeLock of Objects metadata: the C++ face of group R of the C ABI
// (include/earhip.h, where both steps are specified).  libear refuses screenRef, and ear::GainCalculatorObjects and
// ear::hip::ObjectsGainCalculator keep refusing it, so there is no libear class this one mirrors: it is a stage of its own that
// hands back metadata with the position rewritten and screenRef cleared, the way ear::conversion::toPolar hands back polar
// metadata, and the calculators then accept the result.  It follows the conventions of the mirror classes (exceptions for
// status codes, a context argument that defaults to the process-wide one), as hip_objects.hpp and hip_hoa.hpp do.
//
// apply works on polar blocks (group R), in front of the polar calculators; apply_cartesian on Cartesian blocks (group V), in
// front of ear::hip::AllocentricObjectsGainCalculator.
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

      /// the reproduction screen as the C ABI takes it, nullptr without one
      const earhip_screen *reproduction() const { return has_screen_ ? &reproduction_ : nullptr; }

      /// left azimuth, right azimuth, bottom elevation, top elevation of a screen, degrees
      static std::array<double, 4> edges(const Screen &screen) {
        const earhip_screen s = to_c(screen);
        std::array<double, 4> e;
        check(earhip_screen_edges(&s, e.data()));
        return e;
      }

      /// a Screen as the C ABI takes it (the fields of the other kind are zero)
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
      /// group R's lock codes of a screenEdgeLock's strings; a string that names no edge throws adm_error
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
        const Codes codes = lock_codes(metadata, locks, refuse);
        if (n == 0) return;
        const Groups g = group_by_reference(metadata);
        const std::vector<earhip_screen> &screens = g.screens;
        const std::vector<size_t> &idx = g.idx, &first = g.first;
        const ear::detail::DeviceBatch<Arrays> batch(ctx, n);
        const Arrays &a = batch.arrays;
        for (size_t j = 0; j < n; j++) {
          const ObjectsTypeMetadata &m = metadata[idx[j]];
          a.az[j] = m.position.polar.azimuth, a.el[j] = m.position.polar.elevation;
          a.ref[j] = m.screenRef ? 1 : 0, a.h[j] = codes.h[idx[j]], a.v[j] = codes.v[idx[j]];
        }
        int st = EARHIP_OK;
        for (size_t s = 0; s < screens.size() && st == EARHIP_OK; s++) {
          const size_t o = first[s];
          st = earhip_screen_apply_device(ctx.get(), &screens[s], has_screen_ ? &reproduction_ : nullptr, first[s + 1] - o,
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

      /// one CARTESIAN metadata block (cartesian == true and a Cartesian position), on the calling thread (no device), over
      /// group V: to polar, scaled and locked as in apply, back to Cartesian.  Returns a copy with the Cartesian position
      /// rewritten and screenRef = false; extent and every other field are untouched, and a block with neither screenRef nor
      /// a lock keeps the bits of its position.  ear::hip::AllocentricObjectsGainCalculator then accepts the block.  A polar
      /// position or cartesian == false throws not_implemented naming the field, as that calculator does.
      ObjectsTypeMetadata apply_cartesian(const ObjectsTypeMetadata &m, const ScreenEdgeLock &lock = ScreenEdgeLock()) const {
        refuse_polar(m);
        const unsigned char ref = m.screenRef ? 1 : 0, lh = horizontal_code(lock), lv = vertical_code(lock);
        const earhip_screen reference = to_c(m.referenceScreen);
        const CartesianPosition &p = m.position.cartesian;
        ObjectsTypeMetadata out = m;
        CartesianPosition &q = out.position.cartesian;
        check(earhip_screen_apply_cartesian(&reference, has_screen_ ? &reproduction_ : nullptr, 1, &p.X, &p.Y, &p.Z, &ref, &lh,
                                            &lv, &q.X, &q.Y, &q.Z));
        out.screenRef = false;
        return out;
      }

      /// a batch of Cartesian metadata blocks, rewritten in place on the device as the polar batch form does it: one launch
      /// per distinct reference screen, locks empty or one per block, and a block the single form refuses throws here too,
      /// before anything is written.  The results are the bits of earhip_screen_apply_cartesian_device; they are NOT promised
      /// to be the single form's bits (the conversions call the device's math library; the two agree to a few ulps).
      void apply_cartesian(std::vector<ObjectsTypeMetadata> &metadata,
                           const std::vector<ScreenEdgeLock> &locks = std::vector<ScreenEdgeLock>(),
                           Context &ctx = default_context()) const {
        const size_t n = metadata.size();
        const Codes codes = lock_codes(metadata, locks, refuse_polar);
        if (n == 0) return;
        const Groups g = group_by_reference(metadata);
        const ear::detail::DeviceBatch<CartesianArrays> batch(ctx, n);
        const CartesianArrays &a = batch.arrays;
        for (size_t j = 0; j < n; j++) {
          const ObjectsTypeMetadata &m = metadata[g.idx[j]];
          a.x[j] = m.position.cartesian.X, a.y[j] = m.position.cartesian.Y, a.z[j] = m.position.cartesian.Z;
          a.ref[j] = m.screenRef ? 1 : 0, a.h[j] = codes.h[g.idx[j]], a.v[j] = codes.v[g.idx[j]];
        }
        int st = EARHIP_OK;
        for (size_t s = 0; s < g.screens.size() && st == EARHIP_OK; s++) {
          const size_t o = g.first[s];
          st = earhip_screen_apply_cartesian_device(ctx.get(), &g.screens[s], has_screen_ ? &reproduction_ : nullptr,
                                                    g.first[s + 1] - o, a.x + o, a.y + o, a.z + o, a.ref + o, a.h + o, a.v + o,
                                                    a.x + o, a.y + o, a.z + o, a.status + o);
        }
        batch.finish(st, a.status, n, [&g](size_t k) {
          return ear::detail::bad_block(g.idx[k], "x, y and z must be finite");
        });
        for (size_t k = 0; k < n; k++) {
          ObjectsTypeMetadata &m = metadata[g.idx[k]];
          m.position.cartesian.X = a.x[k], m.position.cartesian.Y = a.y[k], m.position.cartesian.Z = a.z[k];
          m.screenRef = false;
        }
      }

      /// the arrays of the polar batch form's block, in the order they are carved
      struct Arrays {
        Arrays(ear::detail::Carver &c, size_t n)
            : az(c.take<double>(n)), el(c.take<double>(n)), status(c.take<int>(n)), ref(c.take<unsigned char>(n)),
              h(c.take<unsigned char>(n)), v(c.take<unsigned char>(n)) {}
        double *az, *el;
        int *status;
        unsigned char *ref, *h, *v;
      };
      /// those of the Cartesian batch form
      struct CartesianArrays {
        CartesianArrays(ear::detail::Carver &c, size_t n)
            : x(c.take<double>(n)), y(c.take<double>(n)), z(c.take<double>(n)), status(c.take<int>(n)),
              ref(c.take<unsigned char>(n)), h(c.take<unsigned char>(n)), v(c.take<unsigned char>(n)) {}
        double *x, *y, *z;
        int *status;
        unsigned char *ref, *h, *v;
      };

     private:
      /// what the two batch forms do before any device work.  The lock codes of every block, after `refuse` had its say on it
      struct Codes {
        std::vector<unsigned char> h, v;
      };
      static Codes lock_codes(const std::vector<ObjectsTypeMetadata> &metadata, const std::vector<ScreenEdgeLock> &locks,
                              void (*refuse)(const ObjectsTypeMetadata &)) {
        const size_t n = metadata.size();
        if (!locks.empty() && locks.size() != n) throw invalid_argument("locks must be empty or one per metadata block");
        Codes c;
        c.h.assign(n, 0), c.v.assign(n, 0);
        for (size_t i = 0; i < n; i++) {
          refuse(metadata[i]);
          if (!locks.empty()) c.h[i] = horizontal_code(locks[i]), c.v[i] = vertical_code(locks[i]);
        }
        return c;
      }
      /// The blocks grouped by reference screen, in order of first appearance: element j of the batch's arrays is block
      /// idx[j], and the elements of screens[s] are first[s] .. first[s + 1]
      struct Groups {
        std::vector<earhip_screen> screens;
        std::vector<size_t> idx, first;
      };
      static Groups group_by_reference(const std::vector<ObjectsTypeMetadata> &metadata) {
        const size_t n = metadata.size();
        Groups g;
        std::vector<size_t> group(n);
        for (size_t i = 0; i < n; i++) {
          const earhip_screen s = to_c(metadata[i].referenceScreen);
          size_t k = 0;
          while (k < g.screens.size() && !same(g.screens[k], s)) k++;
          if (k == g.screens.size()) g.screens.push_back(s);
          group[i] = k;
        }
        g.idx.resize(n);
        size_t j = 0;
        for (size_t k = 0; k < g.screens.size(); k++) {
          g.first.push_back(j);
          for (size_t i = 0; i < n; i++)
            if (group[i] == k) g.idx[j++] = i;
        }
        g.first.push_back(n);
        return g;
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
      // (the fields and their order are AllocentricObjectsGainCalculator's)
      static void refuse_polar(const ObjectsTypeMetadata &m) {
        if (!m.position.isCartesian) throw not_implemented("position: polar");
        if (!m.cartesian) throw not_implemented("cartesian == false");
      }
      bool has_screen_;
      earhip_screen reproduction_;
    };
  }  // namespace hip
}  // namespace ear
