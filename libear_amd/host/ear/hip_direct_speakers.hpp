// ear/hip_direct_speakers.hpp — DirectSpeakers with a Cartesian position or a screenEdgeLock: the C++ face of group X of the C
// ABI (include/earhip.h, where every step is specified).  libear refuses both, and ear::GainCalculatorDirectSpeakers keeps
// refusing them, so this class stands beside it as ear::hip::ObjectsGainCalculator stands beside ear::GainCalculatorObjects:
// the same constructor arguments, the same two calculate forms over the same DirectSpeakersTypeMetadata, and it takes
// position.cartesian (X, Y, Z with XMin ... ZMax) and both screenEdgeLocks.  The bed of a programme whose Objects are
// Cartesian — channels at (-1, 1, 0), (-1, 0, 0), ... with labels that are no BS.2051 labels — goes through it as it is.
//
// The Cartesian bounds test and the fall-through by the BS.2127 section 10 conversion are this project's reading of BS.2127-0
// section 8 (see the group's comment).  A batch with neither a Cartesian position nor a lock gives the bits of
// ear::GainCalculatorDirectSpeakers.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "hip_batch.hpp"
#include "hip_screen.hpp"

namespace ear {
  namespace hip {
    class DirectSpeakersGainCalculator {
     public:
      /// no reproduction screen: a screenEdgeLock changes nothing.  layout and additionalSubstitutions as
      /// ear::GainCalculatorDirectSpeakers takes them
      explicit DirectSpeakersGainCalculator(const Layout &layout, std::map<std::string, std::string> additionalSubstitutions = {},
                                            Context &ctx = default_context())
          : layout_(layout), has_screen_(false), reproduction_(earhip_screen()) {
        create(additionalSubstitutions, ctx);
      }
      /// with a reproduction screen, to whose edges a screenEdgeLock moves a position; throws ear::invalid_argument for a
      /// screen group R refuses (e.g. one across the rear seam)
      DirectSpeakersGainCalculator(const Layout &layout, const Screen &reproduction,
                                   std::map<std::string, std::string> additionalSubstitutions = {},
                                   Context &ctx = default_context())
          : DirectSpeakersGainCalculator(layout, ScreenHandler(reproduction), additionalSubstitutions, ctx) {}
      /// with the reproduction screen of a ScreenHandler (none, if it has none)
      DirectSpeakersGainCalculator(const Layout &layout, const ScreenHandler &screen,
                                   std::map<std::string, std::string> additionalSubstitutions = {},
                                   Context &ctx = default_context())
          : layout_(layout), has_screen_(screen.reproduction() != nullptr),
            reproduction_(has_screen_ ? *screen.reproduction() : earhip_screen()) {
        create(additionalSubstitutions, ctx);
      }
      ~DirectSpeakersGainCalculator() { earhip_direct_speakers_destroy(h_); }
      DirectSpeakersGainCalculator(const DirectSpeakersGainCalculator &) = delete;
      DirectSpeakersGainCalculator &operator=(const DirectSpeakersGainCalculator &) = delete;

      /// one channel's metadata -> its gains, which must have the layout's channel count
      template <typename T>
      void calculate(const DirectSpeakersTypeMetadata &metadata, std::vector<T> &gains,
                     const WarningCB &warning_cb = default_warning_cb) {
        const bool adm_error_first = metadata.audioPackFormatID && metadata.speakerLabels.empty();
        if (!adm_error_first) layout_.check_size(gains.size(), gains.size());
        std::vector<std::vector<T>> g;
        calculate(std::vector<DirectSpeakersTypeMetadata>(1, metadata), g, warning_cb);
        gains = g[0];
      }
      /// a batch of channels; the ones that need the point source panner, polar and Cartesian alike, go to the device in one
      /// launch.  The warnings of each channel reach warning_cb in order (on an error: those raised up to it, then the
      /// throw).  A screenEdgeLock string that names no edge is ear::invalid_argument.
      template <typename T>
      void calculate(const std::vector<DirectSpeakersTypeMetadata> &metadata, std::vector<std::vector<T>> &gains,
                     const WarningCB &warning_cb = default_warning_cb) {
        const size_t n = metadata.size();
        ear::detail::DirectSpeakersRows rows(metadata);
        std::vector<earhip_ds_cartesian> cart(n);
        for (size_t i = 0; i < n; i++) {
          const SpeakerPosition &pos = metadata[i].position;
          const ScreenEdgeLock &lock = pos.isCartesian ? pos.cartesian.screenEdgeLock : pos.polar.screenEdgeLock;
          try {
            rows.md[i].screen_edge_lock_horizontal = ScreenHandler::horizontal_code(lock);
            rows.md[i].screen_edge_lock_vertical = ScreenHandler::vertical_code(lock);
          } catch (const adm_error &e) {
            throw invalid_argument((n > 1 ? "metadata[" + std::to_string(i) + "]: " : std::string()) + e.what());
          }
          earhip_ds_cartesian &c = cart[i];
          c = earhip_ds_cartesian();
          if (!pos.isCartesian) continue;
          const CartesianSpeakerPosition &p = pos.cartesian;
          c.x = p.X, c.y = p.Y, c.z = p.Z;
          c.has_x_min = (bool)p.XMin, c.x_min = p.XMin.value_or(0.0);
          c.has_x_max = (bool)p.XMax, c.x_max = p.XMax.value_or(0.0);
          c.has_y_min = (bool)p.YMin, c.y_min = p.YMin.value_or(0.0);
          c.has_y_max = (bool)p.YMax, c.y_max = p.YMax.value_or(0.0);
          c.has_z_min = (bool)p.ZMin, c.z_min = p.ZMin.value_or(0.0);
          c.has_z_max = (bool)p.ZMax, c.z_max = p.ZMax.value_or(0.0);
        }
        std::vector<float> g(n * layout_.n_full);
        std::vector<int> warnings(2 * n, 0);
        const int status = earhip_direct_speakers_calculate_screen(h_, has_screen_ ? &reproduction_ : nullptr, n, rows.md.data(),
                                                                   cart.data(), g.data(), warnings.data());
        ear::detail::DirectSpeakersRows::finish(status, warnings, warning_cb);
        layout_.scatter(n, g.data(), gains);
      }

      /// the loudspeakers of the caller's layout as the Cartesian bounds test sees them (first: the nominal positions) and
      /// as the nearest-candidate rule does (second: the real ones), through the BS.2127 section 10 point conversion
      std::pair<std::vector<CartesianPosition>, std::vector<CartesianPosition>> cartesianPositions() const {
        std::vector<double> nominal(3 * layout_.n_full), real(3 * layout_.n_full);
        check(earhip_direct_speakers_cartesian_positions(h_, nominal.data(), real.data()));
        std::pair<std::vector<CartesianPosition>, std::vector<CartesianPosition>> out;
        for (int c : layout_.keep) {
          out.first.push_back(CartesianPosition(nominal[3 * c], nominal[3 * c + 1], nominal[3 * c + 2]));
          out.second.push_back(CartesianPosition(real[3 * c], real[3 * c + 1], real[3 * c + 2]));
        }
        return out;
      }

     private:
      void create(const std::map<std::string, std::string> &additionalSubstitutions, Context &ctx) {
        std::vector<const char *> from, to;
        for (auto &kv : additionalSubstitutions) from.push_back(kv.first.c_str()), to.push_back(kv.second.c_str());
        check(earhip_direct_speakers_create_positions(ctx.get(), layout_.name.c_str(), (int)layout_.n_full, layout_.az.data(),
                                                      layout_.el.data(), (int)from.size(), from.data(), to.data(), &h_));
      }

      const ear::detail::LayoutBinding layout_;
      bool has_screen_;
      earhip_screen reproduction_;
      earhip_direct_speakers *h_ = nullptr;
    };
  }  // namespace hip
}  // namespace ear
