// allo_table.h — where the allocentric panner (earhip group T) stands the loudspeakers of the BS.2051 layouts of
// layout_table.h: on the cube [-1, 1]^3, ADM axes (x right, y front, z up), keyed by (layout, channel name).  A row with a
// layout applies to that layout alone and comes before the rows for every layout.  Written after ITU-R BS.2127-0 7.3.10
// without a reference implementation to compare against; earhip_allo_create_positions replaces the table.
#pragma once

#include <cstring>

namespace earhip {

struct AlloPosition {
  const char *layout;  // nullptr: every layout
  const char *name;
  double x, y, z;
};

constexpr double kAlloS = 1.41421356237309504880168872420969808 - 1.0;  // sqrt(2) - 1

static const AlloPosition kAlloPositions[] = {
    {"9+10+3", "M+030", -kAlloS, 1.0, 0.0},
    {"9+10+3", "M-030", kAlloS, 1.0, 0.0},
    {nullptr, "M+000", 0.0, 1.0, 0.0},
    {nullptr, "M+030", -1.0, 1.0, 0.0},
    {nullptr, "M-030", 1.0, 1.0, 0.0},
    {nullptr, "M+SC", -kAlloS, 1.0, 0.0},
    {nullptr, "M-SC", kAlloS, 1.0, 0.0},
    {nullptr, "M+060", -1.0, kAlloS, 0.0},
    {nullptr, "M-060", 1.0, kAlloS, 0.0},
    {nullptr, "M+090", -1.0, 0.0, 0.0},
    {nullptr, "M-090", 1.0, 0.0, 0.0},
    {nullptr, "M+110", -1.0, -1.0, 0.0},
    {nullptr, "M-110", 1.0, -1.0, 0.0},
    {nullptr, "M+135", -1.0, -1.0, 0.0},
    {nullptr, "M-135", 1.0, -1.0, 0.0},
    {nullptr, "M+180", 0.0, -1.0, 0.0},
    {nullptr, "U+000", 0.0, 1.0, 1.0},
    {nullptr, "U+030", -1.0, 1.0, 1.0},
    {nullptr, "U-030", 1.0, 1.0, 1.0},
    {nullptr, "U+045", -1.0, 1.0, 1.0},
    {nullptr, "U-045", 1.0, 1.0, 1.0},
    {nullptr, "U+090", -1.0, 0.0, 1.0},
    {nullptr, "U-090", 1.0, 0.0, 1.0},
    {nullptr, "U+110", -1.0, -1.0, 1.0},
    {nullptr, "U-110", 1.0, -1.0, 1.0},
    {nullptr, "U+135", -1.0, -1.0, 1.0},
    {nullptr, "U-135", 1.0, -1.0, 1.0},
    {nullptr, "U+180", 0.0, -1.0, 1.0},
    {nullptr, "UH+180", 0.0, -1.0, 1.0},
    {nullptr, "T+000", 0.0, 0.0, 1.0},
    {nullptr, "B+000", 0.0, 1.0, -1.0},
    {nullptr, "B+045", -1.0, 1.0, -1.0},
    {nullptr, "B-045", 1.0, 1.0, -1.0},
};

// the row of a channel of a layout; nullptr: the table has none
inline const AlloPosition *allo_position(const char *layout, const char *name) {
  for (const AlloPosition &p : kAlloPositions)
    if (std::strcmp(p.name, name) == 0 && (p.layout == nullptr || std::strcmp(p.layout, layout) == 0)) return &p;
  return nullptr;
}

}  // namespace earhip
