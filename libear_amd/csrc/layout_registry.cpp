// layout_registry.cpp — loudspeaker layouts of the caller's own (include/earhip.h group H: earhip_layout_define,
// earhip_layout_kind, earhip_layout_hull) and the one lookup of a layout by name.  libear's Layout(name, channels) is a
// public constructor and its panner triangulates any such layout with a convex hull
// (src/common/point_source_panner.cpp:484-487); here a layout is defined once, by name, and every entry point that
// takes a layout name then accepts it.  Host code: no context, no device.
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "layout_registry.h"
#include "panner.h"

using namespace earhip;

namespace {

// A definition: the entry and everything it points at.  Held by pointer and never removed, so that a handle (a
// panner, a DirectSpeakers calculator) may keep the address of its LayoutEntry.
struct Definition {
  std::string name;
  std::vector<std::string> channel_names;
  std::vector<LayoutChannel> channels;
  std::vector<int> facets;  // {n, v0 .. v(n-1)}* 0
  LayoutEntry entry;
};

std::mutex g_mutex;
std::vector<std::unique_ptr<Definition>> g_defined;  // guarded by g_mutex

const LayoutEntry *builtin_layout(const char *name) {
  for (int i = 0; i < kNumLayouts; i++)
    if (std::strcmp(kLayouts[i].name, name) == 0) return &kLayouts[i];
  return nullptr;
}

const Definition *defined_layout(const char *name) {  // g_mutex held
  for (auto &d : g_defined)
    if (d->name == name) return d.get();
  return nullptr;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

bool same_content(const Definition &a, const Definition &b) {
  if (a.channels.size() != b.channels.size()) return false;
  for (size_t c = 0; c < a.channels.size(); c++) {
    const LayoutChannel &x = a.channels[c], &y = b.channels[c];
    if (a.channel_names[c] != b.channel_names[c] || x.is_lfe != y.is_lfe || !same_bits(x.azimuth, y.azimuth) ||
        !same_bits(x.elevation, y.elevation) || !same_bits(x.az_lo, y.az_lo) || !same_bits(x.az_hi, y.az_hi) ||
        !same_bits(x.el_lo, y.el_lo) || !same_bits(x.el_hi, y.el_hi))
      return false;
  }
  return true;
}

std::unique_ptr<Definition> make_definition(const char *name, int n_channels, const earhip_layout_channel_def *channels) {
  require(name != nullptr && channels != nullptr, "NULL argument");
  const size_t name_len = std::strlen(name);
  require(name_len >= 1 && name_len <= 63, "a layout name has 1 to 63 characters");
  if (builtin_layout(name)) fail_invalid(std::string("layout name is an ITU-R BS.2051 name: ") + name);
  require(n_channels >= 1 && n_channels <= kMaxLayoutChannels, "a layout has 1 to 32 channels");
  std::unique_ptr<Definition> d(new Definition);
  d->name = name;
  int n_speakers = 0;
  for (int c = 0; c < n_channels; c++) {
    const earhip_layout_channel_def &ch = channels[c];
    const std::string at = "channel " + std::to_string(c) + ": ";
    if (ch.name == nullptr || ch.name[0] == '\0' || std::strlen(ch.name) > 31) fail_invalid(at + "a channel name has 1 to 31 characters");
    for (auto &other : d->channel_names)
      if (other == ch.name) fail_invalid(at + "the name " + ch.name + " is used twice");
    if (!(std::isfinite(ch.azimuth) && std::isfinite(ch.elevation))) fail_invalid(at + "the nominal position must be finite");
    if (!(std::fabs(ch.elevation) <= 90.0 && std::fabs(ch.azimuth) <= 180.0))
      fail_invalid(at + "the nominal azimuth lies in [-180, 180] and the elevation in [-90, 90]");
    LayoutChannel lc = {nullptr, ch.azimuth, ch.elevation, ch.azimuth, ch.azimuth, ch.elevation, ch.elevation, ch.is_lfe != 0};
    if (ch.has_ranges) {
      for (int k = 0; k < 2; k++)
        if (!(std::isfinite(ch.azimuth_range[k]) && std::isfinite(ch.elevation_range[k]))) fail_invalid(at + "the ranges must be finite");
      lc.az_lo = ch.azimuth_range[0], lc.az_hi = ch.azimuth_range[1];
      lc.el_lo = ch.elevation_range[0], lc.el_hi = ch.elevation_range[1];
    }
    d->channel_names.push_back(ch.name);
    d->channels.push_back(lc);
    n_speakers += lc.is_lfe ? 0 : 1;
  }
  require(n_speakers >= 1, "a layout has at least one channel that is not an LFE");
  if (n_speakers > kMaxLayoutSpeakers)
    throw Error{EARHIP_NOT_IMPLEMENTED, "layouts with more than " + std::to_string(kMaxLayoutSpeakers) + " loudspeakers that are not LFE"};
  for (int c = 0; c < n_channels; c++) d->channels[c].name = d->channel_names[c].c_str();  // (the strings no longer move)
  d->entry = {d->name.c_str(), n_channels, d->channels.data(), nullptr};
  return d;
}

// all of a definition's geometry: the hull of the nominal augmented set as its facet list, then what a create with
// nominal positions would do on the host
void triangulate(Definition &d) {
  try {
    for (auto &f : nominal_hull(d.entry)) {
      if (f.size() > 4) fail_internal("facets with more than 4 vertices are not supported");
      d.facets.push_back((int)f.size());
      d.facets.insert(d.facets.end(), f.begin(), f.end());
    }
    d.facets.push_back(0);
    d.entry.facets = d.facets.data();
    panner_dry_run(d.entry);  // (panner.h)
  } catch (const LayoutFailure &e) {
    throw Error{e.status, e.msg};
  }
}

}  // namespace

const LayoutEntry &earhip::find_layout(const char *name) {
  require(name != nullptr, "layout name must not be NULL");
  if (const LayoutEntry *L = builtin_layout(name)) return *L;
  {
    std::lock_guard<std::mutex> lock(g_mutex);
    if (const Definition *d = defined_layout(name)) return d->entry;
  }
  throw Error{EARHIP_UNKNOWN_LAYOUT, std::string("unknown layout: ") + name};
}

extern "C" {

int earhip_layout_define(const char *name, int n_channels, const earhip_layout_channel_def *channels) {
  return guarded([&] {
    std::unique_ptr<Definition> d = make_definition(name, n_channels, channels);
    std::lock_guard<std::mutex> lock(g_mutex);
    if (const Definition *have = defined_layout(name)) {
      if (!same_content(*have, *d)) fail_invalid(std::string("layout ") + name + " is already defined with other content");
      return;
    }
    require(g_defined.size() < (size_t)kMaxDefinedLayouts, "too many defined layouts");
    triangulate(*d);
    g_defined.push_back(std::move(d));
  });
}

int earhip_layout_kind(const char *name, int *kind) {
  return guarded([&] {
    require(name != nullptr && kind != nullptr, "NULL argument");
    std::lock_guard<std::mutex> lock(g_mutex);
    *kind = builtin_layout(name) ? 1 : defined_layout(name) ? 2 : 0;
  });
}

int earhip_layout_hull(const char *name, int vertex_capacity, double *xyz_nominal, int *mix_to, int *n_vertices, int *n_virtual,
                       int facet_capacity, int *facets, int *n_facet_ints) {
  return guarded([&] {
    const LayoutEntry &L = find_layout(name);
    require(L.facets != nullptr, "the layout has no triangulation of its own (0+2+0 pans on 0+5+0)");
    require(vertex_capacity >= 0 && facet_capacity >= 0, "capacities must not be negative");
    const std::vector<AugVertex> verts = augment_layout(L, nullptr, nullptr);
    std::vector<int> full_of;  // loudspeaker that is not LFE -> channel of the full layout
    for (int c = 0; c < L.n; c++)
      if (!L.channels[c].is_lfe) full_of.push_back(c);
    int n_ints = 1, virt = 0;
    for (const int *f = L.facets; *f; f += 1 + *f) n_ints += 1 + *f;
    for (auto &v : verts) virt += v.pole != 0;
    if (n_vertices) *n_vertices = (int)verts.size();
    if (n_virtual) *n_virtual = virt;
    if (n_facet_ints) *n_facet_ints = n_ints;
    if (xyz_nominal || mix_to) {
      require(vertex_capacity >= (int)verts.size(), "vertex_capacity is smaller than the number of vertices");
      for (size_t i = 0; i < verts.size(); i++) {
        const HullPoint p = aug_point(verts[i]);
        if (xyz_nominal) xyz_nominal[3 * i] = p[0], xyz_nominal[3 * i + 1] = p[1], xyz_nominal[3 * i + 2] = p[2];
        if (mix_to) mix_to[i] = verts[i].mix_to < 0 ? -1 : full_of[(size_t)verts[i].mix_to];
      }
    }
    if (facets) {
      require(facet_capacity >= n_ints, "facet_capacity is smaller than the facet list");
      std::memcpy(facets, L.facets, sizeof(int) * (size_t)n_ints);
    }
  });
}

}  // extern "C"
