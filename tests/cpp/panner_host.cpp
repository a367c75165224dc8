// panner_host.cpp — libear_amd/csrc/panner.h compiled for the host alone (g++, no HIP, under ASan and UBSan): the region
// builder, the region walk and the stereo downmix that the device kernels run, and the lock and zone tables of a layout.
// tests/test_panner_core_cpu.py writes the input file and reads the output file:
//   in:  int32 n_defined (0: `name` is a BS.2051 layout), has_positions, n_facet_ints (0: the layout's table; a defined
//        layout: the hull of its nominal positions, as earhip_layout_define makes it), n_dirs, n_masks, n_zones;
//        char name[64]; n_defined x { char name[32]; float64 azimuth, elevation; int32 is_lfe, 0 };
//        has_positions: float64 azimuth[n], elevation[n] (n: channels of the layout, LFE included);
//        int32 facets[n_facet_ints] ({count, vertices}* 0); float64 xyz[n_dirs][3]; uint32 masks[n_masks];
//        earhip_exclusion_zone zones[n_zones]
//   out: int32 status (EARHIP_*), text_len; char text[text_len] (what the set-up refused); and when status is 0:
//        int32 n_pv, n_regions, n_speakers, 0; float64 pv[n_dirs][n_pv]; uint8 missed[n_dirs];
//        int32 lock_order[n_speakers]; uint32 excluded_channels; float64 downmix[n_masks][n][n]
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../libear_amd/csrc/layout_table.h"
#include "../../libear_amd/csrc/layout_registry.h"
#include "../../libear_amd/csrc/panner.h"

using namespace earhip;

namespace {
template <typename T>
bool get(std::FILE *f, T *p, size_t count) {
  return count == 0 || std::fread(p, sizeof(T), count, f) == count;
}
template <typename T>
bool put(std::FILE *f, const T *p, size_t count) {
  return count == 0 || std::fwrite(p, sizeof(T), count, f) == count;
}
struct ChannelRecord {
  char name[32];
  double azimuth, elevation;
  int32_t is_lfe, pad;
};
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[6];
  char name[64];
  if (!get(f, hdr, 6) || !get(f, name, 64) || name[63] != '\0') return 2;
  const int n_defined = hdr[0], has_positions = hdr[1], n_facet_ints = hdr[2], n_dirs = hdr[3], n_masks = hdr[4], n_zones = hdr[5];
  if (n_defined < 0 || n_defined > kMaxLayoutChannels || n_facet_ints < 0 || n_dirs < 0 || n_masks < 0 || n_zones < 0) return 2;
  std::vector<ChannelRecord> rec((size_t)n_defined);
  if (!get(f, rec.data(), rec.size())) return 2;
  std::vector<LayoutChannel> channels;
  LayoutEntry L = {name, 0, nullptr, nullptr};
  if (n_defined) {
    for (ChannelRecord &r : rec) {
      if (r.name[31] != '\0') return 2;
      channels.push_back({r.name, r.azimuth, r.elevation, r.azimuth, r.azimuth, r.elevation, r.elevation, r.is_lfe != 0});
    }
    L.n = n_defined, L.channels = channels.data();
  } else {
    const LayoutEntry *found = nullptr;
    for (int i = 0; i < kNumLayouts; i++)
      if (std::string(kLayouts[i].name) == name) found = &kLayouts[i];
    if (!found) return 2;
    L = *found;
  }
  std::vector<double> az((size_t)(has_positions ? L.n : 0)), el(az.size());
  std::vector<int> facets((size_t)n_facet_ints);
  std::vector<double> xyz(3 * (size_t)n_dirs + 1);
  std::vector<uint32_t> masks((size_t)n_masks);
  std::vector<earhip_exclusion_zone> zones((size_t)n_zones);
  if (!get(f, az.data(), az.size()) || !get(f, el.data(), el.size()) || !get(f, facets.data(), facets.size()) ||
      !get(f, xyz.data(), 3 * (size_t)n_dirs) || !get(f, masks.data(), masks.size()) || !get(f, zones.data(), zones.size()))
    return 2;
  std::fclose(f);
  if (n_facet_ints && facets.back() != 0) return 2;

  int32_t status[2] = {EARHIP_OK, 0};
  std::string text;
  PanParams P;
  std::vector<PanRegion> regions;
  std::vector<double> pv_out, downmix;
  std::vector<uint8_t> missed((size_t)n_dirs, 0);
  std::vector<int32_t> lock_order;
  uint32_t excluded = 0;
  int32_t shape[4] = {0, 0, 0, 0};
  try {
    if (n_facet_ints) {
      L.facets = facets.data();
    } else if (n_defined) {
      for (auto &facet : nominal_hull(L)) {
        facets.push_back((int)facet.size());
        facets.insert(facets.end(), facet.begin(), facet.end());
      }
      facets.push_back(0);
      L.facets = facets.data();
      panner_dry_run(L);
    }
    regions = pan_params(L, has_positions ? az.data() : nullptr, has_positions ? el.data() : nullptr, P);
    P.table.regions = regions.data();
    const int n_pv = P.stereo ? 2 : P.table.n_real;
    pv_out.assign((size_t)n_dirs * n_pv, 0.0);
    for (int i = 0; i < n_dirs; i++) {
      const Vec3 p = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
      double real[kMaxPanOut], pv[kMaxPanOut];
      if (!pan_full(P.table, p, real)) {
        missed[(size_t)i] = 1;
        continue;
      }
      pan_outputs(P, real, pv);
      for (int c = 0; c < n_pv; c++) pv_out[(size_t)i * n_pv + c] = pv[c];
    }
    const std::vector<ObjSpeaker> sp = objects_speakers(L);
    const std::vector<int> rank = objects_lock_rank(sp);
    lock_order.resize(sp.size());
    for (size_t s = 0; s < sp.size(); s++) lock_order[(size_t)rank[s]] = sp[s].full;
    excluded = objects_excluded_channels(sp, n_zones, zones.data());
    const size_t NN = (size_t)L.n * L.n;
    downmix.resize((size_t)n_masks * NN);
    for (int m = 0; m < n_masks; m++) objects_zone_downmix(L, masks[(size_t)m], downmix.data() + (size_t)m * NN);
    shape[0] = n_pv, shape[1] = P.table.n_regions, shape[2] = (int32_t)sp.size();
  } catch (const LayoutFailure &e) {
    status[0] = e.status, text = e.msg;
  }
  status[1] = (int32_t)text.size();
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  bool ok = put(f, status, 2) && put(f, text.data(), text.size());
  if (status[0] == EARHIP_OK)
    ok = ok && put(f, shape, 4) && put(f, pv_out.data(), pv_out.size()) && put(f, missed.data(), missed.size()) &&
         put(f, lock_order.data(), lock_order.size()) && put(f, &excluded, 1) && put(f, downmix.data(), downmix.size());
  return std::fclose(f) == 0 && ok ? 0 : 2;
}
