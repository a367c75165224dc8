"""The case table of the render path beyond 24 loudspeakers: bus widths at which ColumnPlan::make (libear_amd/csrc/curves.h:34-48)
makes more than one column group — what no BS.2051 layout reaches (9+10+3 on two buses is 48 columns, the last width of one group) —
the scene of each case, the options it runs under and the plan it must run, shared by tests/test_wide_bus_cpu.py (the references
against each other and the column plans, no device) and tests/test_gpu_wide_bus.py.

Plain Python: nothing here needs a device.  The expected plans are WRITTEN DOWN from the rules of curves.h for a chip of 256 compute
units (2 * num_cus = 512 workgroups wanted), not computed by the library.

Column plans (ColumnPlan::make, :34-48; tests/cpp/test_column_plan.cpp holds the same numbers against the code).  VALU kernel:
groups = ceil(cols / 24), a wave takes nout = 24 columns at all these widths (cols / groups > 16), ngroups = min(groups, 8) waves per
workgroup, nz = ceil(groups / ngroups) on grid.z.  Matrix-core kernels: mg = ceil(cols / 48) groups of nct = 3 column tiles,
mgroups = min(mg, 8), mnz = ceil(mg / mgroups); the split-operand kernels and F32Grid put all mnz * mgroups groups on grid.z
(api_core.hip:160), the slot kernel mgroups waves in a workgroup and mnz on grid.z (api_core.hip:288).  row = max(nz * ngroups * 24,
mnz * mgroups * 48):
  columns  ngroups nz  mgroups mnz  row
  48       2       1   1       1    48     (the widest BS.2051 case: where the suite stopped)
  49 50 64 3       1   2       1    96
  96       4       1   2       1    96
  98       5       1   3       1    144
  194      8       2   5       1    384
  386      8       3   8       2    768

Kernel (plan_mix, :770-924).  The families are those of tests/many_objects_cases.py, whose docstring derives their statistics, and
every width here has nct = 3; M = 33, 96 or 288 objects is at least 32 (:784, :807) and at most 1024.  So by family and EARHIP_MFMA the
kernel, tile and list layout are those of many_objects_cases._T:
  3 / unset   `grid`: Grid (:784-785).  `holding`, `integer`: the piece lists, paired (:831-832: pair_waste256 0, ramp_share < 0.7 — the
              bound of three column tiles up to 1024 objects).  `ramping`: the hinge kernel (:848), and it stays there through the
              cost comparison of three column tiles (:863-866): hinge 0.56 + 0.077 * 512 / 480 = 0.642, lists 0.151 + 0.238 * (1 + ramp
              pieces per object and 256-sample tile, between 1 and 2 for ramps of 480: 1.53) = 0.753, not below 0.97 * 0.642.
  1           `grid` with blocks of 512: F32Grid (:881-882); with blocks of 256 the call has no 512-sample grid: the slot lists.
              Every other family: the slot lists (:889).
  4           Grid whatever the curves (:785; M / gsplit <= 1024, :800).
  5           the piece lists (:808, :851), paired by the rule above: `holding`, `integer` paired, `grid`, `ramping` packed.
  6           the hinge kernel (:850: hinge_exact_share <= 1 in every family).
  strict      Valu, libear's own arithmetic (:779, :884).
Tile (:757-767): Grid 256 (no call here is long enough for 512, :877), Pieces 256 (:836-837), Hinge 512, F32Grid 512, Slots 16 nrt = 128,
  Valu 64 spl = 256.  ntiles = ceil(nsamples / tile) (:893).
gsplit, split-operand kernels and F32Grid (:788-793): doubles while g < 16, ntiles * mnz * mgroups * g < 512 and M / (2 g) >= 64:
  96 and 33 objects: 1 (96 / 2 < 64).  288 objects at 64 columns: 288 / 2 = 144, 288 / 4 = 72, 288 / 8 = 36 < 64: 4 (at most 4 tiles x 2
  groups x 4 = 32 workgroups: the other bound is far).
gsplit, slot lists (:908-922; max_waves = 4, tiles_per_wg = 4: common.h:168-169):
  96 objects, mgroups = 2 (49 .. 96 columns): tpw = min(4, ntiles, 4 / 2) = 2 (:909; :914 leaves it: ceil(96 / 128) = 1), wsplit =
     max(1, min(4 / (2 * 2), 96 / 8)) = 1, per_wg = 96; g doubles while (ntiles / 2) * g < 512 and 96 / (2 g) >= 8: 48, 24, 12, then
     96 / 16 = 6: gsplit 8.
  96 objects, mgroups = 3, 5, 8: 4 / mgroups is 1 or 0: tpw = 1, wsplit = 1, per_wg = 96: gsplit 8 as above (8 tiles x mnz 2 x 8 = 128
     workgroups at the most).
  288 objects, mgroups = 2: :914 takes tpw to max(1, (4 / 2) / ceil(288 / 128 = 3)) = 1, wsplit = min(4 / 2, 36) = 2, per_wg = 144:
     72, 36, 18, 9 >= 8 and then g = 16 = max_gsplit: gsplit 16.
  33 objects, mgroups = 5 or 8: tpw = 1, wsplit = 1, per_wg = 33: 33 / 2 = 16, 33 / 4 = 8, 33 / 8 = 4 < 8: gsplit 4.
Valu in strict mode: gsplit = 1 (:902-905).
last_list_layout: the plan's `paired` for Pieces and Hinge (False for Hinge: :870), None for every other kernel.

The extra scene `scales` (families `holding+scales`, `ramping+scales`; 25 x 2 and 32 x 2): channel c's gains on both buses times
2^(-4 (c % 4)) — but channel 24 of 25 on two buses takes 2^-12 (its rule value is 2^0, as column 25's, the first diffuse column).
A column's scale of the split-operand kernels (gcol, its inverse applied at write-out) is a power of two from the column's largest
gain: neighbouring columns' scales then differ by 2^12 across
  32 x 2: the tile boundaries 15|16 and 31|32 (= the bus boundary: channel 31 | diffuse channel 0) and the group boundary 47|48
          (diffuse channels 15 | 16);
  25 x 2: the tile boundary 15|16 and the bus boundary 24|25.  (At 31|32 and 47|48 — diffuse channels 6 | 7 and 22 | 23 — the rule gives
          2^4: a bus of odd width keeps the rule's phase from serving every boundary.  Enough for what it is for: a scale of the wrong
          group, read 48 columns off, is that of diffuse channel c + 48 - 25 = c + 23, whose exponent differs from c's by 4 (23 % 4 = 3)
          or 12.)
A column scale taken from a NEIGHBOURING column across one of these boundaries then costs a channel a power of 16 at least — orders
of magnitude beyond every bar — instead of hiding in the similar scales of uniform(0, 1) gains.  What the rule cannot show at 32 x 2 is a
scale read a whole tile or group off: its period of 4 divides 16 and 48, so column j + 48 has column j's factor there (tried: with the
piece-list kernel's inverse scales read from group 0 for every group, all of `scales` at 32 x 2 still passed; at 25 x 2 the odd bus
width shifts the phase and three of its cases failed).  Hence a second scene, `tiles` (`holding+tiles`, `ramping+tiles`; 25 x 2, 32 x 2
and 49 x 2): COLUMN j = bus * N + channel times 2^(-4 ((j // 16) % 4)) — every 16-column tile its own factor, 2^0, 2^-4, 2^-8 in group
0 and 2^-12 in the first tile of group 1 (98 columns: 2^0, 2^-4 in group 1's other tiles, 2^-8 in group 2).  A scale, a gain row or a
store taken one, two or three tiles off — a whole group is three — changes a column by a power of 16; on its loudspeaker the column
weighs 2^-12 of the other bus's at the least, so the channel moves by 2e-4 or more of itself, against bars of 1e-6."""
import functools

import many_objects_cases as mc
from many_objects_cases import VALU, SLOTS, KERNELS, Case

# (loudspeakers, buses): columns — 50: the bus boundary inside tile 1 of group 0, 2 real columns in group 1; 64: the widest defined
# layout, one real and two padded tiles in group 1; 49: one real column in group 1; 96: two full groups; 98: three groups;
# 194: the VALU kernel's nz = 2; 386: mnz = 2, mgroups = 8
WIDTHS = ((25, 2), (32, 2), (49, 1), (48, 2), (49, 2), (97, 2), (193, 2))
COLUMN_PLANS = {  # columns: (nout, ngroups, nz, nct, mgroups, mnz, row)
    48: (24, 2, 1, 3, 1, 1, 48),
    49: (24, 3, 1, 3, 2, 1, 96),
    50: (24, 3, 1, 3, 2, 1, 96),
    64: (24, 3, 1, 3, 2, 1, 96),
    96: (24, 4, 1, 3, 2, 1, 96),
    98: (24, 5, 1, 3, 3, 1, 144),
    194: (24, 8, 2, 3, 5, 1, 384),
    386: (24, 8, 3, 3, 8, 2, 768),
}
FAMILIES = ("grid", "holding", "ramping", "integer")
SEEDS = {"grid": 7, "holding": 11, "ramping": 13, "integer": 0}
# object splits across workgroups by object count (derived above)
SPLIT_GSPLIT = {33: 1, 96: 1, 288: 4}
SLOTS_GSPLIT = {33: 4, 96: 8, 288: 16}
# every kernel kind must be seen running at these widths (the last test of test_gpu_wide_bus.py)
COVERAGE_COLUMNS = (50, 64, 98)


def columns(case):
    return mc.n_out(case) * case.buses


def base_family(family):
    return family.split("+")[0]


def _plan(family, mfma, M, nsamples):
    k = 3 if mfma is None else mfma
    kernel, tile, lay = mc._T[base_family(family)][k]
    if base_family(family) == "grid" and k == 1 and nsamples % 512:  # (blocks of 256: no curve set for the 512-sample grid)
        kernel, tile = SLOTS, 128
    gsplit = SLOTS_GSPLIT[M] if kernel == SLOTS else SPLIT_GSPLIT[M]
    return dict(kernel=kernel, tile=tile, ntiles=-(-nsamples // tile), gsplit=gsplit, layout=lay)


def _id(family, N, K, M, block, nb, mfma):
    return f"{family}-{N}x{K}-M{M}-{nb}x{block}-{mc._mf(mfma)}"


def _build():
    cases = []

    def add(group, family, N, K, M, block, nb):
        for mfma in KERNELS:
            cases.append(Case(_id(family, N, K, M, block, nb, mfma), group, M, N, K, block, nb, family, SEEDS[base_family(family)] + N,
                              {"EARHIP_MFMA": mfma}, _plan(family, mfma, M, block * nb)))
    for family in FAMILIES:
        # ---- every kernel at every width: 96 objects (three chunks of 32, above the slot route of fewer than 32), 2 x 512
        for N, K in WIDTHS:
            add("width", family, N, K, 96, 512, 2)
        # ---- 3 x 256: 768 samples, a part tile for the 512-sample kernels
        for N, K in ((25, 2), (49, 2)):
            add("part", family, N, K, 96, 256, 3)
        # ---- object splits across workgroups and column groups at once: K2 sums 4 (16) partial slabs of 64 columns
        add("gsplit", family, 32, 2, 288, 512, 2)
        # ---- a chunk and one object, at the two widest
        for N, K in ((97, 2), (193, 2)):
            add("m33", family, N, K, 33, 512, 2)
    # ---- column scales 2^12 apart across tile, group and bus boundaries
    for family in ("holding+scales", "ramping+scales"):
        for N, K in ((25, 2), (32, 2)):
            add("scales", family, N, K, 96, 512, 2)
    # ---- every 16-column tile its own scale: a scale, row or store a tile or a group off
    for family in ("holding+tiles", "ramping+tiles"):
        for N, K in ((25, 2), (32, 2), (49, 2)):
            add("tiles", family, N, K, 96, 512, 2)
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids)
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}

# strict mode (kernel 0, the VALU kernel): every width, a family of ramps and the roll call; a part tile; and — the device's FFT
# stands between a diffuse bus and a comparison bit for bit — every column plan again as ONE bus of that many columns
STRICT = ([(f, N, K, 96, 512, 2) for N, K in WIDTHS for f in ("holding", "integer")] + [("grid", 25, 2, 96, 256, 3), ("ramping", 49, 2, 96, 256, 3)]
          + [("holding", N, 1, 96, 512, 2) for N in (50, 64, 96, 98, 194, 386)] + [("ramping", 50, 1, 96, 256, 3), ("grid", 98, 1, 96, 256, 3)])


def strict_case(family, N, K, M, block, nb):
    return Case(f"strict-{family}-{N}x{K}-M{M}-{nb}x{block}", "strict", M, N, K, block, nb, family, 23 + N, {},
                dict(kernel=VALU, tile=256, ntiles=-(-block * nb // 256), gsplit=1, layout=None))


STRICT_CASES = [strict_case(*v) for v in STRICT]


def channel_scales(N, K):
    """the `scales` scene's factor per channel (both buses)"""
    import numpy as np
    s = np.array([2.0 ** (-4 * (c % 4)) for c in range(N)], np.float32)
    if N == 25 and K == 2:
        s[24] = 2.0 ** -12
    return s


def tile_scales(N, K):
    """the `tiles` scene's factor per column, [K][N]"""
    import numpy as np
    j = np.arange(N * K)
    return (2.0 ** (-4 * ((j // 16) % 4))).astype(np.float32).reshape(K, N)


def make_curves(family, M, N, K, block, nblocks, seed):
    import numpy as np
    curves = mc.make_curves(base_family(family), M, N, block, nblocks, seed)
    if family == "integer" and K == 2:  # the roll call on the direct bus, the diffuse bus silent: the output is the answer, delayed
        curves = [(t, d, np.zeros_like(d)) for t, d, _ in curves]
    if family.endswith("+scales"):
        s = channel_scales(N, K)
        curves = [(t, d * s, f * s) for t, d, f in curves]  # (powers of two: exact)
    if family.endswith("+tiles"):
        s = tile_scales(N, K)
        curves = [(t, d * s[0], f * s[1]) for t, d, f in curves]
    return curves


@functools.lru_cache(maxsize=3)
def _scene(family, M, N, K, block, nblocks, seed):
    import scenes
    total = block * nblocks
    curves = make_curves(family, M, N, K, block, nblocks, seed)
    x = mc.integer_inputs(M, total) if family == "integer" else scenes.audio(M, total, seed=seed + 1)
    # (truth: the suite's own object-by-object float64 render — these scenes are small enough for it)
    return mc.build_scene(family, curves, x, mc.speakers(N), K, block, object_by_object=True)


def scene(case):
    """the scene of a case and its CPU references, made once and read-only (many_objects_cases.Scene)"""
    return _scene(case.family, case.M, case.layout, case.buses, case.block, case.nblocks, case.seed)


def scene_key(case):
    return (case.family, case.M, case.layout, case.buses, case.block, case.nblocks, case.seed)


def distinct_scenes(integer):
    seen, out = set(), []
    for c in CASES + STRICT_CASES:
        if (c.family == "integer") == integer and scene_key(c) not in seen:
            seen.add(scene_key(c))
            out.append(c)
    return out
