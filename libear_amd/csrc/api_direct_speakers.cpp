// api_direct_speakers.cpp — the gain calculator for DirectSpeakers channels (earhip group I, DirectSpeakers;
// libear src/direct_speakers/gain_calculator_direct_speakers.cpp:58-320).  Label, LFE and bounds logic over a
// few dozen loudspeakers is host code, as in libear; the channels that fall back to the point source panner go
// to the device panner of group I, all of a call's in one launch.
#include <cctype>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "layout_registry.h"

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
}  // namespace

struct earhip_direct_speakers {
  const LayoutEntry *L = nullptr;
  earhip_panner *panner = nullptr;  // NULL without a context
  std::vector<double> real_xyz;     // [n][3] real positions (distance 1)
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
    int best = -1, n_found = 0;
    double best_d = 0.0, second_d = 0.0;
    for (int c = 0; c < L->n; c++) {
      const LayoutChannel &ch = L->channels[c];
      if (ch.is_lfe != lfe) continue;
      const double nominal_distance = 1.0;  // (BS.2051 positions are on the unit sphere)
      if ((inside_angle_range(ch.azimuth, az_min, az_max, kTol) || std::fabs(ch.elevation) >= 90.0 - kTol) &&
          ch.elevation > el_min - kTol && ch.elevation < el_max + kTol && nominal_distance > d_min - kTol &&
          nominal_distance < d_max + kTol) {
        const double *q = &real_xyz[3 * c];
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
    }
    if (n_found == 1) return best;
    if (n_found > 1 && std::fabs(best_d - second_d) > kTol) return best;
    return -1;
  }

  int index_of(const std::string &name) const {
    for (int c = 0; c < L->n; c++)
      if (name == L->channels[c].name) return c;
    return -1;
  }

  // one channel (:244-320) up to the panner: returns true when the channel needs the point source panner
  bool channel(const earhip_ds_metadata &m, float *g, int *warn) const {
    require(m.n_labels >= 0 && (m.n_labels == 0 || m.labels != nullptr), "labels must not be NULL");
    for (int k = 0; k < m.n_labels; k++) require(m.labels[k] != nullptr, "labels must not be NULL");
    // :247-253
    if (m.audio_pack_format_id && m.n_labels == 0)
      throw Error{EARHIP_ADM_ERROR,
                  "ADM error: common definitions audioPackFormatID specified without any speakerLabels as specified "
                  "in the common definitions file"};
    if (m.cartesian) throw Error{EARHIP_NOT_IMPLEMENTED, "Cartesian position"};
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
    const bool lfe = lfe_freq || lfe_name;
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
        return false;
      }
    }
    // :293 (src/common/screen_edge_lock.hpp:15-17)
    if (m.screen_edge_lock_horizontal || m.screen_edge_lock_vertical) throw Error{EARHIP_NOT_IMPLEMENTED, "screenEdgeLock"};
    // :295-302
    const int c = within_bounds(m, lfe);
    if (c >= 0) {
      g[c] = 1.0f;
      return false;
    }
    // :304-313
    if (lfe) {
      const int lfe1 = index_of("LFE1");
      if (lfe1 >= 0) g[lfe1] = 1.0f;
      return false;
    }
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
    // :62: the point source panner of the layout without its LFE channels (their columns stay zero)
    if (ctx) {
      const int st = panner_create(ctx, layout, azimuth ? n_channels : 0, azimuth, elevation, &ds->panner, false);
      if (st != EARHIP_OK) throw Error{st, earhip_last_error()};
    }
    *out = ds.release();
  });
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
        if (ds->channel(md[i], gains + i * N, warn)) {
          require(ds->panner != nullptr, "a channel needs the point source panner: create with a context");
          ds->pan_az.push_back(md[i].azimuth);
          ds->pan_el.push_back(md[i].elevation);
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
