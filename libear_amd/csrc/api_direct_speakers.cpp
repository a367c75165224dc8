// api_direct_speakers.cpp — the gain calculator for DirectSpeakers channels (earhip group I, DirectSpeakers;
// libear src/direct_speakers/gain_calculator_direct_speakers.cpp:58-320).  Label, LFE and bounds logic over a
// few dozen loudspeakers is host code, as in libear; the channels that fall back to the point source panner go
// to the device panner of group I, all of a call's in one launch.  Group X (earhip_direct_speakers_calculate_screen) is the same
// calculator for the channels libear refuses: a Cartesian position and a screenEdgeLock, over the cores of groups K, R and V.
#include <cctype>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "conversion.h"
#include "layout_registry.h"
#include "screen.h"
#include "screen_cart.h"

using namespace earhip;

namespace {
const double kTol = 1e-5;  // gain_calculator_direct_speakers.cpp:255
const double kPi = 3.14159265358979323846264338327950288;

// Warning::Code (libear_amd/host/ear/warnings.hpp; include/ear/warnings.hpp in libear)
const int kFreqSpeakerLabelLfeMismatch = 1, kFreqNotLfe = 2;

// libear's polar -> Cartesian convention (src/common/geom.cpp:82-87)
void cart(double az, double el, double dist, double (&v)[3]) {
  const double a = -az * kPi / 180.0, e = el * kPi / 180.0;
  v[0] = std::sin(a) * std::cos(e) * dist;
  v[1] = std::cos(a) * std::cos(e) * dist;
  v[2] = std::sin(e) * dist;
}

// is x within the range from start anticlockwise to end, widened by tol? (src/common/geom.cpp:7-28)
bool inside_angle_range(double x, double start, double end, double tol) {
  while (end - 360.0 > start) end -= 360.0;
  while (end < start) end += 360.0;
  const double start_tol = start - tol;
  while (x - 360.0 >= start_tol) x -= 360.0;
  while (x < start_tol) x += 360.0;
  return x <= end + tol;
}

// the capture of ^urn:itu:bs:2051:[0-9]+:speaker:(.*)$ (gain_calculator_direct_speakers.hpp:88-89); false when
// the label does not match.  (ECMAScript's `.` matches no line terminator, so neither does the capture.)
bool speaker_urn(const std::string &label, std::string &capture) {
  static const char prefix[] = "urn:itu:bs:2051:", middle[] = ":speaker:";
  const size_t np = sizeof(prefix) - 1, nm = sizeof(middle) - 1;
  if (label.compare(0, np, prefix) != 0) return false;
  size_t i = np;
  while (i < label.size() && label[i] >= '0' && label[i] <= '9') i++;
  if (i == np || label.compare(i, nm, middle) != 0) return false;
  capture = label.substr(i + nm);
  return capture.find_first_of("\r\n") == std::string::npos;
}

// an audioPackFormatID of the common definitions (AP_0001xxxx), whose channels libear maps by its rule table
bool common_definitions_pack(const char *id) {
  if (std::strlen(id) != 11 || std::strncmp(id, "AP_0001", 7) != 0) return false;
  for (int i = 7; i < 11; i++)
    if (!std::isxdigit((unsigned char)id[i])) return false;
  return true;
}

// The candidates of a bounds test: the only one, or the nearest to p when it is more than kTol nearer than the next
// (:222-242), else -1
struct Nearest {
  int best = -1, n_found = 0;
  double best_d = 0.0, second_d = 0.0;
  void add(int c, const double *q, const double *p) {
    const double d = std::sqrt((q[0] - p[0]) * (q[0] - p[0]) + (q[1] - p[1]) * (q[1] - p[1]) +
                               (q[2] - p[2]) * (q[2] - p[2]));
    if (n_found == 0 || d < best_d) {
      second_d = best_d;
      best_d = d, best = c;
    } else if (n_found == 1 || d < second_d) {
      second_d = d;
    }
    n_found++;
  }
  int pick() const {
    if (n_found == 1) return best;
    if (n_found > 1 && std::fabs(best_d - second_d) > kTol) return best;
    return -1;
  }
};
}  // namespace

struct earhip_direct_speakers {
  const LayoutEntry *L = nullptr;
  earhip_panner *panner = nullptr;  // NULL without a context
  std::vector<double> real_xyz;     // [n][3] real positions (distance 1)
  // group X: the nominal and the real positions through group K's point conversion, [n][3] each, and the first code
  // a conversion returned at create (the table is then not used)
  std::vector<double> nominal_cart, real_cart;
  int cart_status = EARHIP_OK;
  std::map<std::string, std::string> subst;
  std::vector<double> pan_az, pan_el;  // staging of the panner fallback
  std::vector<float> pan_direct, pan_diffuse;
  std::vector<size_t> pan_rows;

  ~earhip_direct_speakers() {
    if (panner) earhip_panner_destroy(panner);
  }

  // :139-150
  std::string nominal_label(const std::string &label) const {
    std::string ret = label, capture;
    if (speaker_urn(label, capture)) ret = capture;
    auto it = subst.find(label);
    if (it != subst.end()) ret = it->second;
    return ret;
  }

  // the channel whose nominal position lies within the bounds (:152-181, :222-242), or -1
  int within_bounds(const earhip_ds_metadata &m, bool lfe) const {
    const double az_min = m.has_azimuth_min ? m.azimuth_min : m.azimuth;
    const double az_max = m.has_azimuth_max ? m.azimuth_max : m.azimuth;
    const double el_min = m.has_elevation_min ? m.elevation_min : m.elevation;
    const double el_max = m.has_elevation_max ? m.elevation_max : m.elevation;
    const double d_min = m.has_distance_min ? m.distance_min : m.distance;
    const double d_max = m.has_distance_max ? m.distance_max : m.distance;
    double p[3];
    cart(m.azimuth, m.elevation, m.distance, p);
    Nearest found;
    for (int c = 0; c < L->n; c++) {
      const LayoutChannel &ch = L->channels[c];
      if (ch.is_lfe != lfe) continue;
      const double nominal_distance = 1.0;  // (BS.2051 positions are on the unit sphere)
      if ((inside_angle_range(ch.azimuth, az_min, az_max, kTol) || std::fabs(ch.elevation) >= 90.0 - kTol) &&
          ch.elevation > el_min - kTol && ch.elevation < el_max + kTol && nominal_distance > d_min - kTol &&
          nominal_distance < d_max + kTol) {
        found.add(c, &real_xyz[3 * c], p);
      }
    }
    return found.pick();
  }

  int index_of(const std::string &name) const {
    for (int c = 0; c < L->n; c++)
      if (name == L->channels[c].name) return c;
    return -1;
  }

  // steps 1-4 of one channel (:244-291): true when a label placed it.  allow_cartesian: group X, which serves the position
  bool by_label(const earhip_ds_metadata &m, bool allow_cartesian, float *g, int *warn, bool &lfe) const {
    require(m.n_labels >= 0 && (m.n_labels == 0 || m.labels != nullptr), "labels must not be NULL");
    for (int k = 0; k < m.n_labels; k++) require(m.labels[k] != nullptr, "labels must not be NULL");
    // :247-253
    if (m.audio_pack_format_id && m.n_labels == 0)
      throw Error{EARHIP_ADM_ERROR,
                  "ADM error: common definitions audioPackFormatID specified without any speakerLabels as specified "
                  "in the common definitions file"};
    if (m.cartesian && !allow_cartesian) throw Error{EARHIP_NOT_IMPLEMENTED, "Cartesian position"};
    // :111-137
    int n_warn = 0;
    const bool lfe_freq = m.has_low_pass && m.low_pass <= 200.0 && !m.has_high_pass;
    if (!lfe_freq && (m.has_low_pass || m.has_high_pass)) warn[n_warn++] = kFreqNotLfe;
    bool lfe_name = false;
    for (int k = 0; k < m.n_labels; k++) {
      const std::string nominal = nominal_label(m.labels[k]);
      lfe_name = lfe_name || nominal == "LFE1" || nominal == "LFE2";
    }
    if (lfe_freq != lfe_name && m.n_labels > 0) warn[n_warn++] = kFreqSpeakerLabelLfeMismatch;
    lfe = lfe_freq || lfe_name;
    // :259-276: the mapping rules of the common-definitions packs are not carried (earhip.h)
    if (m.audio_pack_format_id && common_definitions_pack(m.audio_pack_format_id))
      throw Error{EARHIP_NOT_IMPLEMENTED, std::string("the ITU-R BS.2127 mapping rules of common-definitions packs "
                                                      "(audioPackFormatID ") +
                                              m.audio_pack_format_id + ")"};
    // :278-291: the first label that names a channel of the same type
    for (int k = 0; k < m.n_labels; k++) {
      const int c = index_of(nominal_label(m.labels[k]));
      if (c >= 0 && L->channels[c].is_lfe == lfe) {
        g[c] = 1.0f;
        return true;
      }
    }
    return false;
  }

  // step 6 up to the panner (:304-313): true when the channel needs the point source panner
  bool fall_through(bool lfe, float *g) const {
    if (lfe) {
      const int lfe1 = index_of("LFE1");
      if (lfe1 >= 0) g[lfe1] = 1.0f;
      return false;
    }
    return true;
  }

  // one channel (:244-320) up to the panner: returns true when the channel needs the point source panner
  bool channel(const earhip_ds_metadata &m, float *g, int *warn) const {
    bool lfe = false;
    if (by_label(m, false, g, warn, lfe)) return false;
    // :293 (src/common/screen_edge_lock.hpp:15-17)
    if (m.screen_edge_lock_horizontal || m.screen_edge_lock_vertical) throw Error{EARHIP_NOT_IMPLEMENTED, "screenEdgeLock"};
    // :295-302
    const int c = within_bounds(m, lfe);
    if (c >= 0) {
      g[c] = 1.0f;
      return false;
    }
    return fall_through(lfe, g);
  }

  // group X, step 5b for a Cartesian position p (after the lock) with its bounds: the channel of the same LFE type whose
  // converted nominal position lies within them, the nearest of several by the converted real positions, or -1
  int within_cartesian_bounds(const double p[3], const double lo[3], const double hi[3], bool lfe) const {
    Nearest found;
    for (int c = 0; c < L->n; c++) {
      if (L->channels[c].is_lfe != lfe) continue;
      const double *q = &nominal_cart[3 * c];
      if (q[0] > lo[0] - kTol && q[0] < hi[0] + kTol && q[1] > lo[1] - kTol && q[1] < hi[1] + kTol && q[2] > lo[2] - kTol &&
          q[2] < hi[2] + kTol)
        found.add(c, &real_cart[3 * c], p);
    }
    return found.pick();
  }

  // group X: one channel up to the panner; true when it needs the point source panner, at (az, el)
  bool channel_screen(const earhip_ds_metadata &m, const earhip_ds_cartesian *cart_md, const screen::Map &map, float *g,
                      int *warn, double &az, double &el) const {
    if (m.cartesian) require(cart_md != nullptr, "a Cartesian position needs the cart array");
    bool lfe = false;
    if (by_label(m, true, g, warn, lfe)) return false;
    // step 5a
    const unsigned lock_h = (unsigned)m.screen_edge_lock_horizontal, lock_v = (unsigned)m.screen_edge_lock_vertical;
    require(lock_h <= 2 && lock_v <= 2, "screenEdgeLock: a lock code is 0, 1 or 2");
    if (!m.cartesian) {
      earhip_ds_metadata locked = m;
      if (screen::apply_one(map, m.azimuth, m.elevation, 0u, lock_h, lock_v, locked.azimuth, locked.elevation) != 0)
        fail_invalid("screenEdgeLock: azimuth " + std::to_string(m.azimuth) + ", elevation " + std::to_string(m.elevation) +
                     ": the angles must be finite, the azimuth within +-2^40 and the elevation within +-90 degrees");
      const int c = within_bounds(locked, lfe);
      if (c >= 0) {
        g[c] = 1.0f;
        return false;
      }
      az = locked.azimuth, el = locked.elevation;
      return fall_through(lfe, g);
    }
    const earhip_ds_cartesian &k = *cart_md;
    const int has[6] = {k.has_x_min, k.has_x_max, k.has_y_min, k.has_y_max, k.has_z_min, k.has_z_max};
    const double bound[6] = {k.x_min, k.x_max, k.y_min, k.y_max, k.z_min, k.z_max};
    require(std::isfinite(k.x) && std::isfinite(k.y) && std::isfinite(k.z), "a Cartesian position must be finite");
    for (int b = 0; b < 6; b++) require(!has[b] || std::isfinite(bound[b]), "a Cartesian bound that is present must be finite");
    if (cart_status != EARHIP_OK)
      throw Error{EARHIP_INVALID_ARGUMENT, "a loudspeaker position of this calculator has no Cartesian form (group K's point "
                                           "conversion returned code " + std::to_string(cart_status) + ")"};
    double p[3];
    int st = screen::apply_cart_one(map, k.x, k.y, k.z, 0u, lock_h, lock_v, p);
    if (st != EARHIP_OK)
      throw Error{EARHIP_INVALID_ARGUMENT, "screenEdgeLock: group K's point conversion returned code " + std::to_string(st)};
    double lo[3], hi[3];
    for (int a = 0; a < 3; a++) lo[a] = has[2 * a] ? bound[2 * a] : p[a], hi[a] = has[2 * a + 1] ? bound[2 * a + 1] : p[a];
    const int c = within_cartesian_bounds(p, lo, hi, lfe);
    if (c >= 0) {
      g[c] = 1.0f;
      return false;
    }
    if (!fall_through(lfe, g)) return false;
    double polar[3];
    st = conv::point_cart_to_polar(p[0], p[1], p[2], polar);
    if (st != EARHIP_OK)
      throw Error{EARHIP_INVALID_ARGUMENT, "group K's point conversion to polar returned code " + std::to_string(st)};
    // (a guard in front of the launch: the conversion reports no overflow of its own)
    require(std::isfinite(polar[0]) && std::isfinite(polar[1]), "group K's point conversion to polar gave no finite direction");
    az = polar[0], el = polar[1];
    return true;
  }
};

static int ds_create(earhip_ctx *ctx, const char *layout, int n_channels, const double *azimuth,
                     const double *elevation, int n_subst, const char *const *from, const char *const *to,
                     earhip_direct_speakers **out) {
  return guarded([&] {
    require(out != nullptr, "NULL argument");
    const LayoutEntry &L = find_layout(layout);
    require((azimuth == nullptr) == (elevation == nullptr), "azimuth and elevation come together");
    if (azimuth) {
      require(n_channels == L.n, "one position per channel of the layout (LFE channels included)");
      for (int c = 0; c < L.n; c++)
        require(std::isfinite(azimuth[c]) && std::isfinite(elevation[c]), "loudspeaker positions must be finite");
    }
    require(n_subst >= 0 && (n_subst == 0 || (from != nullptr && to != nullptr)), "substitutions must not be NULL");
    std::unique_ptr<earhip_direct_speakers> ds(new earhip_direct_speakers);
    ds->L = &L;
    // :80-83: the defaults, then the caller's where they do not name the same label (std::map::insert)
    ds->subst = {{"LFE", "LFE1"}, {"LFEL", "LFE1"}, {"LFER", "LFE2"}};
    for (int k = 0; k < n_subst; k++) {
      require(from[k] != nullptr && to[k] != nullptr, "substitutions must not be NULL");
      ds->subst.insert(std::make_pair(std::string(from[k]), std::string(to[k])));
    }
    ds->real_xyz.resize(3 * (size_t)L.n);
    for (int c = 0; c < L.n; c++) {
      double v[3];
      cart(azimuth ? azimuth[c] : L.channels[c].azimuth, elevation ? elevation[c] : L.channels[c].elevation, 1.0, v);
      for (int k = 0; k < 3; k++) ds->real_xyz[3 * c + k] = v[k];
    }
    // group X: both sets of positions as group K's point conversion places them (distance 1)
    ds->nominal_cart.assign(3 * (size_t)L.n, std::nan(""));
    ds->real_cart.assign(3 * (size_t)L.n, std::nan(""));
    for (int c = 0; c < L.n && ds->cart_status == EARHIP_OK; c++) {
      double q[3], r[3];
      int st = conv::point_polar_to_cart(L.channels[c].azimuth, L.channels[c].elevation, 1.0, q);
      if (st == EARHIP_OK)
        st = conv::point_polar_to_cart(azimuth ? azimuth[c] : L.channels[c].azimuth,
                                       elevation ? elevation[c] : L.channels[c].elevation, 1.0, r);
      ds->cart_status = st;
      for (int k = 0; k < 3 && st == EARHIP_OK; k++) ds->nominal_cart[3 * c + k] = q[k], ds->real_cart[3 * c + k] = r[k];
    }
    // :62: the point source panner of the layout without its LFE channels (their columns stay zero)
    if (ctx) {
      const int st = panner_create(ctx, layout, azimuth ? n_channels : 0, azimuth, elevation, &ds->panner, false);
      if (st != EARHIP_OK) throw Error{st, earhip_last_error()};
    }
    *out = ds.release();
  });
}

// What both entry points do with a batch: one(i, row, warn, az, el) runs channel i up to the panner and returns true, with
// the position to pan, when the channel needs it; every such channel then goes to the panner in one launch.
template <typename One>
static void calculate_batch(earhip_direct_speakers *ds, size_t n, const earhip_ds_metadata *md, float *gains,
                            int *warnings_out, One &&one) {
  require(n == 0 || (md != nullptr && gains != nullptr), "metadata and gains must not be NULL");
  require(n < ((size_t)1 << 28), "too many channels");
  const size_t N = (size_t)ds->L->n;
  std::memset(gains, 0, sizeof(float) * n * N);
  if (warnings_out) std::memset(warnings_out, 0, sizeof(int) * 2 * n);
  ds->pan_az.clear();
  ds->pan_el.clear();
  ds->pan_rows.clear();
  for (size_t i = 0; i < n; i++) {
    int warn[2] = {0, 0};
    try {
      double az = 0.0, el = 0.0;
      if (one(i, gains + i * N, warn, az, el)) {
        require(ds->panner != nullptr, "a channel needs the point source panner: create with a context");
        ds->pan_az.push_back(az);
        ds->pan_el.push_back(el);
        ds->pan_rows.push_back(i);
      }
    } catch (Error &e) {
      if (warnings_out) warnings_out[2 * i] = warn[0], warnings_out[2 * i + 1] = warn[1];
      if (n > 1) e.msg = "metadata[" + std::to_string(i) + "]: " + e.msg;
      throw;
    }
    if (warnings_out) warnings_out[2 * i] = warn[0], warnings_out[2 * i + 1] = warn[1];
  }
  // :314-318: one launch for every channel that falls back to the panner (the panner normalises its gain
  // vector, so the position's distance does not enter)
  const size_t m = ds->pan_rows.size();
  if (m == 0) return;
  ds->pan_direct.resize(m * N);
  ds->pan_diffuse.resize(m * N);
  const int st = earhip_panner_calculate(ds->panner, m, ds->pan_az.data(), ds->pan_el.data(), nullptr, nullptr, nullptr,
                                         ds->pan_direct.data(), ds->pan_diffuse.data());
  if (st != EARHIP_OK) throw Error{st, earhip_last_error()};
  for (size_t k = 0; k < m; k++)
    std::memcpy(gains + ds->pan_rows[k] * N, ds->pan_direct.data() + k * N, sizeof(float) * N);
}

extern "C" {

int earhip_direct_speakers_create(earhip_ctx *ctx, const char *layout, int n_subst, const char *const *from,
                                  const char *const *to, earhip_direct_speakers **out) {
  return ds_create(ctx, layout, 0, nullptr, nullptr, n_subst, from, to, out);
}

int earhip_direct_speakers_create_positions(earhip_ctx *ctx, const char *layout, int n_channels, const double *azimuth,
                                            const double *elevation, int n_subst, const char *const *from,
                                            const char *const *to, earhip_direct_speakers **out) {
  return ds_create(ctx, layout, n_channels, azimuth, elevation, n_subst, from, to, out);
}

int earhip_direct_speakers_destroy(earhip_direct_speakers *ds) {
  return guarded([&] { delete ds; });
}

int earhip_direct_speakers_num_channels(const earhip_direct_speakers *ds, int *n_channels) {
  return guarded([&] {
    require(ds != nullptr && n_channels != nullptr, "NULL argument");
    *n_channels = ds->L->n;
  });
}

int earhip_direct_speakers_calculate(earhip_direct_speakers *ds, size_t n, const earhip_ds_metadata *md, float *gains,
                                     int *warnings_out) {
  return guarded([&] {
    require(ds != nullptr, "NULL argument");
    calculate_batch(ds, n, md, gains, warnings_out, [&](size_t i, float *g, int *warn, double &az, double &el) {
      az = md[i].azimuth, el = md[i].elevation;
      return ds->channel(md[i], g, warn);
    });
  });
}

int earhip_direct_speakers_calculate_screen(earhip_direct_speakers *ds, const earhip_screen *reproduction, size_t n,
                                            const earhip_ds_metadata *md, const earhip_ds_cartesian *cart, float *gains,
                                            int *warnings_out) {
  return guarded([&] {
    require(ds != nullptr, "NULL argument");
    // the map of earhip_screen_apply[_cartesian] for a NULL reference: the default screen's edges to the reproduction's
    screen::Map map = screen::identity_map();
    if (reproduction) {
      earhip_screen reference;
      double e_ref[4], e_rep[4];
      int st = earhip_screen_default(&reference);
      if (st == EARHIP_OK) st = earhip_screen_edges(&reference, e_ref);
      if (st == EARHIP_OK) st = earhip_screen_edges(reproduction, e_rep);
      if (st != EARHIP_OK) throw Error{st, std::string("reproduction screen: ") + earhip_last_error()};
      map = screen::make_map(e_ref, e_rep);
    }
    calculate_batch(ds, n, md, gains, warnings_out, [&](size_t i, float *g, int *warn, double &az, double &el) {
      return ds->channel_screen(md[i], cart ? cart + i : nullptr, map, g, warn, az, el);
    });
  });
}

int earhip_direct_speakers_cartesian_positions(const earhip_direct_speakers *ds, double *nominal_xyz, double *real_xyz) {
  return guarded([&] {
    require(ds != nullptr && nominal_xyz != nullptr && real_xyz != nullptr, "NULL argument");
    if (ds->cart_status != EARHIP_OK)
      throw Error{EARHIP_INVALID_ARGUMENT, "a loudspeaker position of this calculator has no Cartesian form (group K's point "
                                           "conversion returned code " + std::to_string(ds->cart_status) + ")"};
    std::memcpy(nominal_xyz, ds->nominal_cart.data(), sizeof(double) * ds->nominal_cart.size());
    std::memcpy(real_xyz, ds->real_cart.data(), sizeof(double) * ds->real_cart.size());
  });
}

int earhip_direct_speakers_missed(earhip_direct_speakers *ds, unsigned *count) {
  return guarded([&] {
    require(ds != nullptr && count != nullptr, "NULL argument");
    *count = 0;
    if (ds->panner) {
      const int st = earhip_panner_missed(ds->panner, count);
      if (st != EARHIP_OK) throw Error{st, earhip_last_error()};
    }
  });
}

}  // extern "C"
