// Host unit test of the launch planner and the scratch layout (libear_amd/csrc/curves.h): for a fixed list of cases — a
// handful of base cases, one factor varied at a time — the plan plan_mix makes, one line per case, compared with
// tests/golden/plan_table.txt (written by the planner as it was before the kernel kind replaced its five flags); and for
// every case the regions of the scratch buffer: in order, disjoint, ending at the total scratch_units returns.
// No HIP call is made: runs without a GPU.
//   test_plan_table <golden file>     compare (exit status 0: equal)
//   test_plan_table                   print the table
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "curves.h"

using namespace earhip;

struct Case {
  const char *name;
  int M = 1024, ncols = 48, nsamples = 512 * 1024;
  bool strict = false;
  int max_gsplit = 16, use_mfma = 3;
  size_t lds = 128 * 1024;  // the hinge builder's dynamic LDS on the device
  int nrt = 8, spl = 4;
  std::vector<std::pair<Opt, int>> opts;
  CurveStats st;
  Case(const char *n) : name(n) {}
};

// the base cases: curves on the 512-sample grid (Grid), curves that hold most of the time off the grid (Pieces, paired),
// curves that ramp all the time off the grid (Hinge), exact f32 on the grid (F32Grid)
static Case on_grid(const char *n) {
  Case c(n);
  c.st.aligned_tile = 512, c.st.ramp_share = 0.25, c.st.gain_scale = 1.0f;
  return c;
}
static Case holding(const char *n) {
  Case c(n);
  c.st.aligned_tile = 0, c.st.ramp_share = 0.25, c.st.gain_scale = 1.0f, c.st.point_density = 1.0 / 2048;
  c.st.pair_waste256 = 0.01, c.st.pair_waste512 = 0.01, c.st.hinge_exact_share = 2.0, c.st.deltas256 = 0.2;
  return c;
}
static Case ramping(const char *n) {
  Case c(n);
  c.st.aligned_tile = 0, c.st.ramp_share = 1.0, c.st.gain_scale = 1.0f, c.st.point_density = 1.0 / 480;
  c.st.pair_waste256 = 0.5, c.st.pair_waste512 = 0.5, c.st.hinge_exact_share = 0.0, c.st.deltas256 = 1.5;
  return c;
}
static Case exact_grid(const char *n) {
  Case c = on_grid(n);
  c.use_mfma = 1, c.st.grid512_strict = true;
  return c;
}

static std::vector<Case> cases() {
  std::vector<Case> v;
  auto add = [&v](Case c) -> Case & { v.push_back(c); return v.back(); };
  // ---- curves on the grid
  add(on_grid("grid"));
  add(on_grid("grid_aligned256")).st.aligned_tile = 256;
  add(on_grid("grid_short")).nsamples = 512 * 8;  // block mode: object splits across workgroups
  add(on_grid("grid_short_gsplit1")).nsamples = 512 * 8, v.back().max_gsplit = 1;
  add(on_grid("grid_one_block")).nsamples = 512;
  add(on_grid("grid_odd_length")).nsamples = 512 * 33 + 37;
  add(on_grid("grid_h2_tile256")).opts = {{OPT_H2_TILE, 256}};
  add(on_grid("grid_short_h2_tile512")).nsamples = 512 * 8, v.back().opts = {{OPT_H2_TILE, 512}};
  add(on_grid("grid_M31")).M = 31;
  add(on_grid("grid_M32")).M = 32;
  add(on_grid("grid_M128_short")).M = 128, v.back().nsamples = 512 * 8;
  add(on_grid("grid_no_scale")).st.gain_scale = 0.0f;  // non-finite gains: the f32 slot kernel
  add(on_grid("grid_strict")).strict = true;
  add(on_grid("grid_strict_spl2")).strict = true, v.back().spl = 2;
  for (int ncols : {5, 10, 24, 96}) add(on_grid("grid_cols")).ncols = ncols;
  for (int ncols : {5, 24}) add(on_grid("grid_short_cols")).ncols = ncols, v.back().nsamples = 512 * 8;
  for (int mfma = 0; mfma <= 6; mfma++) add(on_grid("grid_mfma")).use_mfma = mfma;
  add(on_grid("slots_mfma2_nrt4")).use_mfma = 2, v.back().nrt = 4;
  add(on_grid("slots_mfma2_M8_short")).use_mfma = 2, v.back().M = 8, v.back().nsamples = 512 * 8;
  add(on_grid("slots_mfma2_M256_short")).use_mfma = 2, v.back().M = 256, v.back().nsamples = 512 * 8;
  add(on_grid("slots_mfma2_M65536")).use_mfma = 2, v.back().M = kMaxSlotObjects, v.back().nsamples = 512 * 8;
  add(on_grid("valu_mfma2_M65537")).use_mfma = 2, v.back().M = kMaxSlotObjects + 1, v.back().nsamples = 512 * 8;
  // ---- curves that hold most of the time, off the grid
  add(holding("pieces"));
  add(holding("pieces_short")).nsamples = 512 * 8;
  add(holding("pieces_one_block")).nsamples = 512;
  add(holding("pieces_waste512")).st.pair_waste512 = 0.2;
  add(holding("pieces_waste256")).st.pair_waste256 = 0.2;
  add(holding("pieces_pairs0")).opts = {{OPT_P2_PAIRS, 0}};
  add(holding("pieces_waste256_pairs1")).st.pair_waste256 = 0.2, v.back().opts = {{OPT_P2_PAIRS, 1}};
  add(holding("pieces_p2_tile256")).opts = {{OPT_P2_TILE, 256}};
  add(holding("pieces_short_p2_tile512")).nsamples = 512 * 8, v.back().opts = {{OPT_P2_TILE, 512}};
  add(holding("pieces_M31")).M = 31;
  add(holding("pieces_M32")).M = 32;
  add(holding("pieces_M65536")).M = kMaxPieceObjects, v.back().nsamples = 512 * 8;
  add(holding("pieces_M65537")).M = kMaxPieceObjects + 1, v.back().nsamples = 512 * 8;  // beyond both lists: the VALU kernel
  add(holding("pieces_no_scale")).st.gain_scale = 0.0f;
  add(holding("pieces_strict")).strict = true;
  for (int ncols : {5, 24}) add(holding("pieces_cols")).ncols = ncols;
  for (int mfma = 0; mfma <= 6; mfma++) add(holding("pieces_mfma")).use_mfma = mfma;
  add(holding("pieces_hinge1")).opts = {{OPT_HINGE, 1}};  // (not a curve set for the hinge kernel: exact share 2)
  add(holding("pieces_hinge1_exact_share")).opts = {{OPT_HINGE, 1}}, v.back().st.hinge_exact_share = 0.5;
  // ---- curves that ramp all the time, off the grid
  add(ramping("hinge"));
  add(ramping("hinge_short")).nsamples = 512 * 8;
  add(ramping("hinge_hg_tile256")).opts = {{OPT_HG_TILE, 256}};
  add(ramping("hinge_hg_tile512")).opts = {{OPT_HG_TILE, 512}};
  add(ramping("hinge_hinge0")).opts = {{OPT_HINGE, 0}};
  add(ramping("hinge_hinge1")).opts = {{OPT_HINGE, 1}};
  add(ramping("hinge_exact_share")).st.hinge_exact_share = 0.01;
  add(ramping("hinge_ramp_share")).st.ramp_share = 0.45;
  // (the cost comparison with the packed lists: the lists win, the hinge kernel wins, and with two column tiles it is not made)
  add(ramping("hinge_cost_lists")).st.ramp_share = 0.55, v.back().st.deltas256 = 0.6, v.back().st.point_density = 1.0 / 960;
  add(ramping("hinge_cost_hinge")).st.ramp_share = 0.55, v.back().st.deltas256 = 1.0, v.back().st.point_density = 1.0 / 960;
  add(ramping("hinge_cost_cols24")).st.ramp_share = 0.55, v.back().st.deltas256 = 0.6, v.back().st.point_density = 1.0 / 960,
      v.back().ncols = 24;
  // (ramp-then-hold curves the paired lists take up to 1024 objects on three column tiles)
  for (int M : {1024, 1025}) add(ramping("hinge_mostly_ramping_M")).M = M, v.back().st.ramp_share = 0.6, v.back().st.pair_waste256 = 0.01;
  add(ramping("hinge_mostly_ramping_cols24")).ncols = 24, v.back().st.ramp_share = 0.6, v.back().st.pair_waste256 = 0.01;
  // (the builder's LDS: 16 bytes per object)
  for (int M : {4096, 4097}) add(ramping("hinge_lds64k_M")).M = M, v.back().lds = 64 * 1024, v.back().nsamples = 512 * 64;
  for (int M : {8192, 8193}) add(ramping("hinge_lds128k_M")).M = M, v.back().nsamples = 512 * 64;
  add(ramping("hinge_M31")).M = 31;
  add(ramping("hinge_M32")).M = 32;
  for (int ncols : {5, 24}) add(ramping("hinge_cols")).ncols = ncols;
  for (int mfma = 0; mfma <= 6; mfma++) add(ramping("hinge_mfma")).use_mfma = mfma;
  add(ramping("hinge_mfma6_exact_share")).use_mfma = 6, v.back().st.hinge_exact_share = 1.5;
  // ---- exact f32 on the 512-sample grid
  add(exact_grid("f32grid"));
  add(exact_grid("f32grid_short")).nsamples = 512 * 8;
  add(exact_grid("f32grid_off_grid")).st.grid512_strict = false;
  add(exact_grid("f32grid_part_tile")).nsamples = 512 * 3 + 64;
  add(exact_grid("f32grid_M15")).M = 15;
  add(exact_grid("f32grid_M16")).M = 16;
  add(exact_grid("f32grid_no_scale")).st.gain_scale = 0.0f;
  for (int ncols : {5, 24}) add(exact_grid("f32grid_cols")).ncols = ncols;
  // ---- above 1024 objects: the plans tests/many_objects_cases.py writes down for its short calls on one bus of 10 columns (one
  // call of 1024 samples on the 512-sample grid, one of 768 on the 256-sample grid), every forced kernel, with and without
  // object splits across workgroups; and the 16-bit object index on 6 columns
  for (int max_gsplit : {16, 1})
    for (int M : {1536, 2048, 4096, 4097, 8192, 8193})
      for (int nsamples : {1024, 768})
        for (int mfma : {1, 3, 4, 5, 6}) {
          auto set = [&](Case &c) { c.M = M, c.ncols = 10, c.nsamples = nsamples, c.max_gsplit = max_gsplit, c.use_mfma = mfma; };
          Case &g = add(on_grid(max_gsplit == 16 ? "many_grid" : "many_grid_gsplit1"));
          set(g), g.st.ramp_share = 1.0, g.st.pair_waste256 = 0.0, g.st.hinge_exact_share = 0.0;
          g.st.aligned_tile = nsamples % 512 ? 256 : 512, g.st.grid512_strict = nsamples % 512 == 0;
          set(add(holding(max_gsplit == 16 ? "many_holding" : "many_holding_gsplit1"))), v.back().st.hinge_exact_share = 0.0;
          set(add(ramping(max_gsplit == 16 ? "many_ramping" : "many_ramping_gsplit1")));
        }
  for (int M : {kMaxPieceObjects, kMaxPieceObjects + 1})
    for (int mfma : {1, 3, 5}) {
      Case &c = add(holding("many_holding_index16"));
      c.M = M, c.ncols = 6, c.nsamples = 512, c.use_mfma = mfma, c.st.hinge_exact_share = 0.0;
    }
  // ---- beyond one column group (tests/wide_bus_cases.py: 96 objects, 2 blocks of 512 on 25 x 2, 32 x 2 and 49 x 2 columns): every
  // forced kernel on the three curve families, in block mode
  for (int ncols : {50, 64, 98})
    for (int mfma : {1, 3, 4, 5, 6}) {
      auto set = [&](Case &c) { c.M = 96, c.ncols = ncols, c.nsamples = 1024, c.use_mfma = mfma; };
      Case &g = add(on_grid("wide_grid"));
      set(g), g.st.ramp_share = 1.0, g.st.pair_waste256 = 0.0, g.st.hinge_exact_share = 0.0, g.st.grid512_strict = true;
      set(add(holding("wide_holding"))), v.back().st.hinge_exact_share = 0.0;
      set(add(ramping("wide_ramping")));
    }
  return v;
}

static int failures = 0;
static void check(bool ok, const Case &c, const char *what) {
  if (ok) return;
  if (failures++ < 20) printf("%s (M %d, cols %d, %d samples): %s\n", c.name, c.M, c.ncols, c.nsamples, what);
}

static std::string table() {
  std::string out = "# case M ncols nsamples mfma | kind tile ntiles wsplit gsplit tpw paired pw wide hinge_tile scratch_units\n";
  for (const Case &c : cases()) {
    earhip_ctx ctx;
    ctx.num_cus = 256;
    ctx.use_mfma = c.use_mfma;
    ctx.hinge_build_lds = c.lds;
    ctx.nrt = c.nrt;
    ctx.spl = c.spl;
    for (const auto &o : c.opts) ctx.opt[o.first].set = true, ctx.opt[o.first].v = o.second;
    const ColumnPlan cp = ColumnPlan::make(c.ncols);
    const MixLaunch ml = plan_mix(&ctx, cp, c.M, c.nsamples, c.strict, c.max_gsplit, c.st);
    // (a set of one-point curves: its piece lists have a slot per object and the padding, CurveSet::piece_cap)
    const CurveSet cs(c.M, c.ncols);
    const size_t units = scratch_units(cs, ml, c.M);
    char line[512];
    snprintf(line, sizeof line, "%s %d %d %d %d | %d %d %d %d %d %d %d %d %d %d %zu\n", c.name, c.M, c.ncols, c.nsamples, c.use_mfma,
             (int)ml.kind, ml.tile(), ml.ntiles, ml.wsplit, ml.gsplit, ml.tpw, (int)ml.paired, ml.pw, (int)ml.wide, ml.hinge_tile, units);
    out += line;
    // The layout.  The regions in use together lie in order, without overlap, and the last ends at the total (offsets are whole
    // 16-byte units; the hinge lists and the lists standing by for them are two views of the same memory); and every array of the
    // list views the launchers take from it — entries, count words, overflow words, as the kernels index them — lies inside its
    // region, computed here from the structs' own extents.
    const ScratchLayout lay = scratch_layout(cs, ml, c.M);
    check(lay.total == units, c, "scratch_units is not the layout's total");
    typedef ScratchLayout::Region Region;
    auto walk = [&](const Region &a, const Region &b) {
      check(a.at == 0 && (!b.units || b.at == a.units), c, "a region does not start where the one before it ends");
      check(a.units + b.units <= lay.total, c, "a region ends beyond the total");
      return a.units + b.units;
    };
    const size_t used = std::max(walk(lay.desc, lay.slots), std::max(walk(lay.pieces, lay.piece_stage), walk(lay.hinge, lay.hinge_stage)));
    check(used == lay.total, c, "the regions do not end at the total");
    std::vector<SegDesc> buf(1);  // (only addresses are compared: nothing is read or written through them)
    SegDesc *base = buf.data();
    auto inside = [&](const void *p, size_t bytes, const Region &r, const char *what) {
      const char *lo = reinterpret_cast<const char *>(base) + 16 * r.at, *q = static_cast<const char *>(p);
      check(q >= lo && q + bytes <= lo + 16 * r.units, c, what);
    };
    const size_t M = (size_t)c.M, nt = (size_t)ml.ntiles, pt = (size_t)lay.piece_tiles;
    if (ml.kind == GainKernel::Slots) {
      const SlotLists sl = lay.slot_lists(base);
      inside(sl.slots, sizeof(Slot) * kTileSlots * M * nt, lay.slots, "slot entries outside their region");
      inside(sl.count, sizeof(int) * 4 * nt, lay.slots, "slot counts outside their region");
      inside(sl.ovf, sizeof(int) * M * nt, lay.slots, "slot overflow words outside their region");
      check((const char *)sl.count >= (const char *)(sl.slots + kTileSlots * M * nt) && sl.ovf >= sl.count + 4 * nt, c, "slot arrays overlap");
    }
    if (ml.kind == GainKernel::Pieces || ml.kind == GainKernel::Hinge) {
      const PieceLists pl = lay.piece_lists(base, ml.paired);
      inside(pl.pieces, sizeof(Piece) * (size_t)pl.cap() * pt, lay.pieces, "piece entries outside their region");
      inside(pl.count, sizeof(int) * 8 * pt, lay.pieces, "piece counts outside their region");
      inside(pl.ovf, sizeof(int) * M * pt, lay.pieces, "piece overflow words outside their region");
      check((const char *)pl.count >= (const char *)(pl.pieces + (size_t)pl.cap() * pt) && pl.ovf >= pl.count + 8 * pt, c, "piece arrays overlap");
      inside(lay.piece_staging(base), sizeof(PairRec) * M * pt, lay.piece_stage, "piece staging matrix outside its region");
      // (the lists of a call of nsamples have no more tiles than the buffer was sized for)
      check(scratch_layout(cs, ml, c.M, c.nsamples).total <= units, c, "a call's layout is larger than scratch_units");
    }
    if (ml.kind == GainKernel::Hinge) {
      const HingeLists hl = lay.hinge_lists(base);
      inside(hl.lin, sizeof(LinEntry) * (size_t)hl.cap * nt, lay.hinge, "hinge line entries outside their region");
      inside(hl.hinge, sizeof(HingeEntry) * (size_t)hl.cap * nt, lay.hinge, "hinge entries outside their region");
      inside(hl.cflags, sizeof(uint32_t) * (size_t)(hl.cap / 32) * nt, lay.hinge, "hinge chunk flags outside their region");
      inside(hl.count, sizeof(int) * 4 * nt, lay.hinge, "hinge counts outside their region");
      inside(hl.ovf, sizeof(int) * M * nt, lay.hinge, "hinge overflow words outside their region");
      inside(lay.hinge_staging(base), sizeof(HingeCached) * M * nt, lay.hinge_stage, "hinge staging matrix outside its region");
    }
  }
  return out;
}

int main(int argc, char **argv) {
  const std::string got = table();
  if (argc < 2) {
    fputs(got.c_str(), stdout);
    return failures != 0;
  }
  std::string want;
  if (FILE *f = fopen(argv[1], "rb")) {
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) want.append(buf, n);
    fclose(f);
  }
  if (got != want) {
    size_t at = 0;
    while (at < got.size() && at < want.size() && got[at] == want[at]) at++;
    const size_t b = got.rfind('\n', at) == std::string::npos ? 0 : got.rfind('\n', at) + 1;
    printf("the plan table differs from %s, first at:\n  got  %s\n", argv[1], got.substr(b, got.find('\n', at) - b).c_str());
    const size_t wb = want.rfind('\n', at) == std::string::npos ? 0 : want.rfind('\n', at) + 1;
    if (at < want.size()) printf("  want %s\n", want.substr(wb, want.find('\n', at) - wb).c_str());
    return 1;
  }
  printf("%zu cases, %d layout failures\n", cases().size(), failures);
  return failures != 0;
}
