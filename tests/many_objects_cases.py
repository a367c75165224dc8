"""The case table of the gain stage above 1024 objects: object counts at which plan_mix (libear_amd/csrc/curves.h) or a list
builder (api_core.hip) changes what it does, the scene of each case, the options it runs under and the plan it must run,
shared by tests/test_many_objects_cpu.py (the references against each other, no device) and tests/test_gpu_many_objects.py.

Plain Python: nothing here needs a device.  The expected plans are WRITTEN DOWN from plan_mix's rules for a chip of 256 compute
units (2 * num_cus = 512 workgroups wanted), not computed by the library.  The derivation, with the lines of curves.h used:

Column plan (ColumnPlan::make, :34-48): 10 or 6 columns on one bus: nct = 1, mgroups = mnz = ngroups = nz = 1; 24 channels x 2
buses = 48 columns: nct = 3, mgroups = mnz = 1.

Curve statistics (stats_of, :533-609; points that repeat their predecessor are dropped first, :167-188):
  grid     dense_curves on the block grid from time 0: every segment a ramp as long as the block (ramp_share 1, no segment
           shorter than kHingeMinLen = 128: hinge_exact_share 0), aligned_tile = block (512; 256 for blocks of 256, :381-411),
           grid512_strict with blocks of 512 only (:475).
  holding  adm_curves(period 700, ramp 150): ramps of 150 and holds of 550 at a phase per object: aligned_tile 0, ramp_share
           600 / 2250 or 750 / 2950 per object (< 0.5), two ramps never meet one tile of 256 or 512 samples (550 between them):
           pair_waste 0; no segment shorter than 128: hinge_exact_share 0.
  ramping  adm_curves(period 480, ramp 480): after the repeats are dropped a point every 480 samples, every segment a ramp:
           ramp_share 1, aligned_tile 0 (phases differ, 480 is no multiple of 256), hinge_exact_share 0.
  mostly   adm_curves(period 960, ramp 600) over 2048 samples: 4 or 5 ramps of 600 and 3 or 4 holds of 360 per object:
           ramp_share 2400 / 3480 = 0.690 or 3000 / 4440 = 0.676 — between 0.5 and 0.7; pair_waste256 0 (360 > 256);
           hinge_exact_share 0.
  integer  integer_curves below: three objects in four have one point at time 0; every fourth steps twice (two points at one
           time) — half of those at 256 and 512, the others at times off every tile grid and more than 256 samples apart.
           Steps have no length: ramp_share 0; an eighth of the objects is off the 256-sample grid, more than the M / 64
           aligned_tile tolerates (:402-408): aligned_tile 0; two steps never meet one 256-sample tile: pair_waste256 0; a step
           is a segment shorter than 128: hinge_exact_share min(1, ...) is far above 0.005 and never above 1.

Kernel (plan_mix, :770-924), EARHIP_MFMA unset = 3:
  3 / unset   Grid (3) where aligned (:784-785): `grid`.  Else the piece lists (:807-808), paired when pair_waste256 < 0.06 and
              ramp_share < 0.5 (:831-832; 0.7 for nct == 3 and M <= 1024): `holding`, `integer`, `mostly` at 1024.  The hinge kernel
              (:848) for M <= min(8192, LDS / 16) = 8192, hinge_exact_share <= 0.005, ramp_share >= 0.5 and not paired by rule:
              `ramping` up to 8192 objects, `mostly` at 1025; above 8192 `ramping` stays on the lists, packed.
              (:863-866, three column tiles only: the cost comparison.  `ramping` at 2049: hinge 0.56 + 0.077 * 512 / 480 = 0.642,
              lists 0.151 + 0.238 * (1 + 2.87 / 1.875) = 0.753: the hinge kernel.  `mostly` at 1025, from the scene's own points by
              the formulas of stats_of: ramp_share 0.6876, 0.0020138 points per sample, 0.97915 ramp pieces per object and
              256-sample tile: hinge 0.56 + 0.077 * 512 * 0.0020138 = 0.63939, lists 0.151 + 0.238 * 1.97915 = 0.62204, not below
              0.97 * 0.63939 = 0.62021: the hinge kernel.)
  1           neither (:784, :808): F32Grid (2) where grid512_strict and the call is whole 512-sample tiles (:881-882), else the
              slot lists (1) up to 65536 objects, else Valu (0) (:889).
  4           Grid (3) at any object count: whatever the curves (:785) while a workgroup's share of the objects, M / gsplit, is at
              most 1024 (:800); off the grid with more (EARHIP_GSPLIT=1 here, and 65536 / 16) the slot lists (1) or, above 65536
              objects, Valu (0): the gate behind `object_splits`, added with these tests — forced onto always-ramping curves with
              the whole list through one workgroup the grid kernel's exact path was 1.3 to 1.44 times libear's own distance from
              float64 (bar 3), measured at 1536 .. 8193 objects.
  5           the piece lists (:808, :851), layout by the rule above.
  6           the hinge kernel where M <= 8192 and hinge_exact_share <= 1 (:850), else the piece lists.
  beyond 65536 objects the lists are refused (:807) and 3, 5, 6, 1 end on Valu (:889), as tests/golden/plan_table.txt has it
  (pieces_M65537, valu_mfma2_M65537).
Tile (:757-767): Grid 256 (wide needs nsamples / 512 >= 512, :877), Pieces 64 pw = 256 (no long call, :836-837), Hinge 512,
  F32Grid 512, Slots 16 nrt = 128, Valu 64 spl = 256.  ntiles = ceil(nsamples / tile) (:893).
gsplit: split-operand kernels and F32Grid double while g < max_gsplit, ntiles * g < 512 and M / (2 g) >= 64 (:788-793): 16 from
  1024 objects on (max_gsplit = 16, api_render.hip:443; EARHIP_GSPLIT=1: 1).  Slots: tpw = 1 above 512 objects (:914), wsplit = 4
  (:915), per_wg = M / 4, doubling while per_wg / (2 g) >= 8 (:921): 16.  Valu the same with ngroups = 1: 16.
last_list_layout: the plan's `paired` for Pieces and Hinge (False for Hinge: :870), None for every other kernel
  (api_render.hip:363)."""
import functools
from collections import namedtuple

VALU, SLOTS, F32GRID, GRID, PIECES, HINGE = range(6)
KERNELS = (None, 1, 3, 4, 5, 6)  # EARHIP_MFMA; None: the library's choice

Case = namedtuple("Case", "id group M layout buses block nblocks family seed opts plan")
# plan: kernel, tile, ntiles, gsplit, layout (of the lists: True paired, False packed, None: the kernel has none)

FULL_M = (1536, 2048, 4096, 4097, 8192, 8193)
PARTITIONS = ((512, 2), (256, 3))  # (block, blocks of the one call): 1024 samples; 768: a part tile

# (kernel, tile, list layout) by family and EARHIP_MFMA on one bus of 10 or 6 columns; "big": above 8192 objects, where it differs
_T = {
    "grid": {3: (GRID, 256, None), 1: (F32GRID, 512, None), 4: (GRID, 256, None), 5: (PIECES, 256, False),
             6: (HINGE, 512, False), "big6": (PIECES, 256, False)},
    "holding": {3: (PIECES, 256, True), 1: (SLOTS, 128, None), 4: (GRID, 256, None), 5: (PIECES, 256, True),
                6: (HINGE, 512, False), "big6": (PIECES, 256, True)},
    "ramping": {3: (HINGE, 512, False), "big3": (PIECES, 256, False), 1: (SLOTS, 128, None), 4: (GRID, 256, None),
                5: (PIECES, 256, False), 6: (HINGE, 512, False), "big6": (PIECES, 256, False)},
    "integer": {3: (PIECES, 256, True), 1: (SLOTS, 128, None), 4: (GRID, 256, None), 5: (PIECES, 256, True),
                6: (HINGE, 512, False), "big6": (PIECES, 256, True)},
}


def _plan(family, mfma, M, nsamples, gsplit):
    k = 3 if mfma is None else mfma
    row = _T[family]
    kernel, tile, lay = row.get(f"big{k}", row[k]) if M > 8192 else row[k]
    if family == "grid" and k == 1 and nsamples % 512:  # (blocks of 256: no curve set for the 512-sample grid)
        kernel, tile = SLOTS, 128
    if k == 4 and family != "grid" and M // gsplit > 1024:  # (forced off its grid: up to 1024 objects per workgroup)
        kernel, tile = SLOTS, 128
    if M > 65536 and kernel in (SLOTS, PIECES, HINGE):
        kernel, tile, lay = VALU, 256, None
    return dict(kernel=kernel, tile=tile, ntiles=-(-nsamples // tile), gsplit=gsplit, layout=lay)


def _opts(mfma, **more):
    o = {"EARHIP_MFMA": mfma}
    o.update(more)
    return o


def _mf(mfma):
    return "auto" if mfma is None else f"mfma{mfma}"


def _build():
    cases = []
    add = cases.append
    seeds = {"grid": 7, "holding": 11, "ramping": 13, "mostly": 17, "integer": 0}
    # ---- the full matrix, and the 2-block partition again with the whole list through one workgroup (EARHIP_GSPLIT=1)
    for family in ("grid", "holding", "ramping", "integer"):
        for M in FULL_M:
            for block, nb in PARTITIONS:
                for gs in (16, 1) if nb == 2 else (16,):
                    for mfma in KERNELS:
                        o = _opts(mfma, EARHIP_GSPLIT=1) if gs == 1 else _opts(mfma)
                        add(Case(f"{family}-M{M}-{nb}x{block}-{_mf(mfma)}" + ("-gsplit1" if gs == 1 else ""), "full" if gs == 16 else "gsplit1",
                                 M, "4+5+0", 1, block, nb, family, seeds[family] + M, o, _plan(family, mfma, M, block * nb, gs)))
    # ---- the rule edge of the paired lists on three column tiles (24 channels x 2 buses), the library's choice
    add(Case("mostly-M1024", "edge", 1024, "9+10+3", 2, 512, 4, "mostly", 17, _opts(None),
             dict(kernel=PIECES, tile=256, ntiles=8, gsplit=16, layout=True)))
    add(Case("mostly-M1025", "edge", 1025, "9+10+3", 2, 512, 4, "mostly", 17, _opts(None),
             dict(kernel=HINGE, tile=512, ntiles=4, gsplit=16, layout=False)))
    # ---- two buses: K2 sums 16 partial slabs
    add(Case("holding-M2049-2bus", "twobus", 2049, "9+10+3", 2, 512, 2, "holding", 11, _opts(None),
             dict(kernel=PIECES, tile=256, ntiles=4, gsplit=16, layout=True)))
    add(Case("ramping-M2049-2bus", "twobus", 2049, "9+10+3", 2, 512, 2, "ramping", 13, _opts(None),
             dict(kernel=HINGE, tile=512, ntiles=2, gsplit=16, layout=False)))
    # ---- the 16-bit object index: 65536 on the lists, 65537 beyond them
    for family, kernels in (("holding", (None, 1, 5)), ("integer", KERNELS)):
        for M in (65536, 65537):
            for gs in (16, 1) if family == "integer" else (16,):
                for mfma in kernels:
                    o = _opts(mfma, EARHIP_GSPLIT=1) if gs == 1 else _opts(mfma)
                    add(Case(f"{family}-M{M}-1x512-{_mf(mfma)}" + ("-gsplit1" if gs == 1 else ""), "index16", M, "0+5+0", 1, 512, 1, family,
                             seeds[family] + 1, o, _plan(family, mfma, M, 512, gs)))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids)
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}

# the hinge list builder (`ramping`, EARHIP_MFMA=6, one call of 2 blocks of 512 on 4+5+0): its forms per object count — tiles per
# workgroup v wherever M v <= 8192 (api_core.hip:179-185), and the two-kernel builder (api_core.hip:186-203)
BUILDER = {
    1024: [{"EARHIP_HBUILD_TPW": v} for v in (1, 2, 4, 8)],
    2048: [{"EARHIP_HBUILD_TPW": v} for v in (1, 2, 4)],
    4096: [{"EARHIP_HBUILD_TPW": v} for v in (1, 2)],
    4097: [{"EARHIP_HBUILD_TPW": 1}, {"EARHIP_BUILD_2K": 1}],
    8192: [{"EARHIP_HBUILD_TPW": 1}, {"EARHIP_BUILD_2K": 1}],
}


def builder_case(M):
    return Case(f"builder-M{M}", "builder", M, "4+5+0", 1, 512, 2, "ramping", 13 + M, _opts(6),
                dict(kernel=HINGE, tile=512, ntiles=2, gsplit=16, layout=False))


# strict mode: (family, M, layout, block, blocks)
STRICT = [(f, M, "4+5+0" if M < 65536 else "0+5+0", 512, 2 if M < 65536 else 1) for f in ("holding", "integer") for M in (2048, 8193, 65537)]


def strict_case(family, M, layout, block, nb):
    return Case(f"strict-{family}-M{M}", "strict", M, layout, 1, block, nb, family, 23, {},
                dict(kernel=VALU, tile=256, ntiles=-(-block * nb // 256), gsplit=1, layout=None))


def speakers(layout):
    """the loudspeaker names of a case's `layout`: a BS.2051 layout's own, or, for a plain channel count N (tests/wide_bus_cases.py:
    widths no BS.2051 layout has), made-up ones S000 .. — design_decorrelators takes any names"""
    if isinstance(layout, int):
        return [f"S{c:03d}" for c in range(layout)]
    from layouts import LAYOUTS
    return LAYOUTS[layout]


def n_out(case):
    return len(speakers(case.layout))


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def integer_steps(j):
    """the two step times of stepping object j (object 4 j): even j on the tile grid, odd j off it and 257 samples or more apart"""
    if j % 2 == 0:
        return 256, 512
    s1 = 37 + (j * 13) % 200
    return s1, s1 + 257 + (j * 7) % 100


def integer_curves(M, N):
    """The roll call: object m feeds channel m % N alone, with a gain of 1 or 2; every fourth object steps to the other value
    and back (two points at one time); the others hold one point."""
    import numpy as np
    curves = []
    for m in range(M):
        a = 1 + (m // 4 + m // N) % 2
        if m % 4:
            g = np.zeros((1, N), np.float32)
            g[0, m % N] = a
            curves.append((np.zeros(1, np.int64), g, None))
            continue
        s1, s2 = integer_steps(m // 4)
        g = np.zeros((4, N), np.float32)
        g[:, m % N] = (a, 3 - a, 3 - a, a)
        curves.append((np.array([s1, s1, s2, s2], np.int64), g, None))
    return curves


def integer_inputs(M, total):
    import numpy as np
    m = np.arange(M, dtype=np.int64)[:, None]
    s = np.arange(total, dtype=np.int64)[None, :]
    return (((7 * m + s) % 5) - 2).astype(np.float32)


def integer_answer(M, N, total):
    """(the int64 render of the roll call, the largest sum of |gain x| of a channel and sample: no partial sum in any order is
    larger) — from the rule of integer_curves, not from its curves: a step at time t holds from sample t on"""
    import numpy as np
    m = np.arange(M, dtype=np.int64)
    a = 1 + (m // 4 + m // N) % 2
    g = np.repeat(a[:, None], total, axis=1)
    s = np.arange(total)
    for mm in range(0, M, 4):
        s1, s2 = integer_steps(mm // 4)
        g[mm, (s >= s1) & (s < s2)] = 3 - a[mm]
    x = integer_inputs(M, total).astype(np.int64)
    p = g * x
    out = np.zeros((N, total), np.int64)
    mag = np.zeros((N, total), np.int64)
    for c in range(N):
        out[c] = p[c::N].sum(axis=0)
        mag[c] = np.abs(p[c::N]).sum(axis=0)
    return out, int(mag.max())


def make_curves(family, M, N, block, nblocks, seed):
    import scenes
    total = block * nblocks
    if family == "grid":
        return scenes.dense_curves(M, N, block, nblocks, seed=seed)
    if family == "holding":
        return scenes.adm_curves(M, N, total, period=700, ramp=150, seed=seed)
    if family == "ramping":
        return scenes.adm_curves(M, N, total, period=480, ramp=480, seed=seed)
    if family == "mostly":
        return scenes.adm_curves(M, N, total, period=960, ramp=600, seed=seed)
    assert family == "integer"
    return integer_curves(M, N)


def bus_f64(curves, x, N, bus=0, chunk=4096):
    """float64 evaluation of one bus, libear's segmentation in exact arithmetic (what scenes.render_f64 computes object by
    object), vectorised: per chunk of objects the two weights of every sample on its segment's end points, and one float64
    matrix product per point index"""
    import numpy as np
    M, total = x.shape
    t = np.arange(total, dtype=np.float64)[None, :]
    out = np.zeros((N, total))
    for m0 in range(0, M, chunk):
        cs = curves[m0:m0 + chunk]
        K = max(len(c[0]) for c in cs)
        T = np.empty((len(cs), K), np.float64)
        G = np.empty((len(cs), K, N), np.float64)
        for i, c in enumerate(cs):
            n = len(c[0])
            T[i, :n], T[i, n:] = c[0], c[0][-1]
            G[i, :n], G[i, n:] = c[1 + bus], c[1 + bus][-1]
        k = np.zeros((len(cs), total), np.int64)
        for j in range(K):
            k += T[:, j:j + 1] <= t
        lo, hi = np.clip(k - 1, 0, K - 1), np.clip(k, 0, K - 1)
        tlo, thi = np.take_along_axis(T, lo, 1), np.take_along_axis(T, hi, 1)
        span = thi - tlo
        p = np.where(span > 0, (t - tlo) / np.where(span > 0, span, 1.0), 0.0)
        xs = x[m0:m0 + chunk].astype(np.float64)
        wlo, whi = xs * (1.0 - p), xs * p
        for j in range(K):
            w = np.where(lo == j, wlo, 0.0) + np.where(hi == j, whi, 0.0)
            out += G[:, j, :].T @ w
    return out


Scene = namedtuple("Scene", "curves x dec delay want truth answer magnitude")


def build_scene(family, curves, x, names, buses, block, object_by_object=False):
    """the CPU references of one scene on the loudspeakers `names`: the oracle's render of `curves` over the inputs `x`, and the
    float64 evaluation (object_by_object: scenes.render_f64 instead of the vectorised bus_f64 — small scenes) or, for the roll
    call, the int64 answer"""
    import numpy as np
    import _oracle
    import scenes
    M, total = x.shape
    N = len(names)
    x.setflags(write=False)
    if buses == 2:
        dec, delay = _oracle.design_decorrelators(names), _oracle.compensation_delay()
        o = _oracle.ObjectsRenderer(M, N, block, dec, delay)
    else:  # direct bus only: zero decorrelators, no delay => the output is the direct bus exactly
        dec, delay = None, 0
        o = _oracle.ObjectsRenderer(M, N, block, np.zeros((N, 1), np.float32), 0)
    zeros = {}
    for m, (t, d, f) in enumerate(curves):
        o.set_points(m, 0, t, d)
        if buses == 2:
            o.set_points(m, 1, t, f)
        else:
            o.set_points(m, 1, t, zeros.setdefault(d.shape, np.zeros_like(d)))
    want = o.process(x)
    want.setflags(write=False)
    answer = magnitude = truth = None
    if family == "integer":
        answer, magnitude = integer_answer(M, N, total)
        if buses == 2:  # (the roll call on the direct bus beside a silent diffuse bus: the answer, delayed)
            answer = np.concatenate([np.zeros((N, delay), np.int64), answer], axis=1)[:, :total]
    elif object_by_object:
        truth = scenes.render_f64([(t, d, f if buses == 2 else None) for t, d, f in curves], x, N, dec, delay)
    else:
        truth = bus_f64(curves, x, N, 0)
        if buses == 2:
            diffuse = bus_f64(curves, x, N, 1)
            for c in range(N):
                truth[c] = np.convolve(diffuse[c], dec[c].astype(np.float64))[:total] + np.concatenate([np.zeros(delay), truth[c]])[:total]
    return Scene(curves, x, dec, delay, want, truth, answer, magnitude)


@functools.lru_cache(maxsize=3)
def _scene(family, M, layout, buses, block, nblocks, seed):
    import scenes
    names = speakers(layout)
    total = block * nblocks
    curves = make_curves(family, M, len(names), block, nblocks, seed)
    x = integer_inputs(M, total) if family == "integer" else scenes.audio(M, total, seed=seed + 1)
    return build_scene(family, curves, x, names, buses, block)


def scene(case):
    """the scene of a case and its CPU references, made once and read-only: the oracle's render (`want`), and the float64
    evaluation (`truth`) or, for the roll call, the int64 answer and the largest sum of magnitudes"""
    return _scene(case.family, case.M, case.layout, case.buses, case.block, case.nblocks, case.seed)


def scene_key(case):
    return (case.family, case.M, case.layout, case.buses, case.block, case.nblocks, case.seed)


def matrix_points(family, M, N, seed):
    """one curve of [M][N] matrices on common times, for earhip_gain_interp (libear's LinearInterpMatrix): `holding` a ramp of
    150, a hold of 350 and a ramp of 150; `integer` the roll call with every stepping object's steps at 137 and 384"""
    import numpy as np
    if family == "holding":
        v = np.random.default_rng(seed).uniform(0.0, 1.0, (3, M, N)).astype(np.float32)
        return np.array([-100, 50, 400, 550], np.int64), np.stack([v[0], v[1], v[1], v[2]])
    m = np.arange(M)
    a = (1 + (m // 4 + m // N) % 2).astype(np.float32)
    b = np.where(m % 4 == 0, 3 - a, a).astype(np.float32)
    vals = np.zeros((4, M, N), np.float32)
    for k, g in enumerate((a, b, b, a)):
        vals[k, m, m % N] = g
    return np.array([137, 137, 384, 384], np.int64), vals


def per_sample(a, b):
    """the worst |a - b| of one sample over the largest |b| of its channel, over all channels"""
    import numpy as np
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)))
