"""The case table of the gain kernels' rare paths — the exact redo of a wave whose f16 totals overflowed, rows that cannot be read or
stored as 16-byte vectors (GainMixParams::vec_ok == 0), a call without a probed input scale, a non-finite input sample — with the
scene of each case, the options it runs under and the plan and form it must run, shared by tests/test_rare_paths_cpu.py (the
conditions that make the scenes mean what they say, no device) and tests/test_gpu_rare_paths.py.

Plain Python: nothing here needs a device.  Every scene has 128 objects: plan_mix (libear_amd/csrc/curves.h) then splits the objects
of a split-operand or f32 grid call over gsplit = 2 workgroups while the call has fewer than 2 x (compute units) tiles and
EARHIP_GSPLIT does not say 1 (object_splits: M / (2 g) >= 64 ends it at 2), and a call runs the form the DEVICE picks — the plain
form here, every object at one level — only where ntiles x gsplit >= 2 x (compute units) (acquire_call_words, api_core.hip); a
shorter call, and a call without a probe (EARHIP_XSCALE, unaligned input rows), runs the wide form.

Groups (A, the piece-list rows of SPLIT_KERNELS, lives in tests/test_gpu_render.py):
  B  the plain form's redo in calls long enough for the device to pick the form: long_scene(), bursts 10^4 above the level in
     unprobed samples; piece lists with P2_WGS 0 / 1 / 3 / 8 (bit-equal), GSPLIT unset and 1, the call cut in two; hinge kernel.
     The piece-list kernel carries its pipeline from one tile's list into the next only where p2_persistent (gain_p2.h:517) says so:
     not on 256-sample tiles with three column tiles (9+10+3 on two buses), where launch_pieces keeps a workgroup per tile whatever
     P2_WGS says — there the sweep compares four equal launches.  So every piece-list case of B runs on 0+5+0 as well (two buses:
     12 columns, one column tile), where both tile sizes carry; carried() is the rule, Case.extra["carried"] what a case runs.
  C  a fixed input scale 2^k (EARHIP_XSCALE = 7, 16, 18) on full-scale inputs: no, some, every wave span overflows.
  D  rows that are not vectors, four ways, on every kernel kind 0 .. 5.
  E  one inf / NaN in the list kernels: everything outside its workgroup tile is the render of a zero in its place, bit for bit."""
import functools
from collections import namedtuple

import numpy as np

import scenes

VALU, SLOTS, F32GRID, GRID, PIECES, HINGE = range(6)
KNAME = {VALU: "valu", SLOTS: "slots", F32GRID: "f32grid", GRID: "grid", PIECES: "pieces", HINGE: "hinge"}
CUS = 256            # compute units of an MI355X: what the CPU file checks the long scenes for (the GPU file reads the device's)
F16_OVERFLOW = 65520.0  # the smallest magnitude that rounds to an infinite f16
M = 128

Case = namedtuple("Case", "id group kernel tile layout buses form paired opts scene extra")
# form: what Renderer.wide_form() must say — "wide" True, "plain" False, "none" None (the kernel has no split operands)
# paired: what Renderer.last_list_layout() must say (None: no lists)


def n_out(layout):
    from layouts import LAYOUTS
    return len(LAYOUTS[layout])


# ---- probe, scale, overflow: the rules of the library, restated ------------------------------------------------------------------
def probed_in(obj, s, calls):
    """does k_level_probe read sample s of this object's row in one of the `calls` [(first sample, samples)] that hold it"""
    for start, n in calls:
        if start <= s < start + n and (s - start) in _probed(obj, n):
            return True
    return False


@functools.lru_cache(maxsize=None)
def _probed(obj, n):
    return frozenset(scenes.probed_samples(obj, n))


def probed_scale_log2(x, start=0, n=None):
    """log2 of the input scale of a call over samples [start, start + n) of x: probed_input_scale (gain_split.h:71-78) — the largest
    probed magnitude, in [2^E, 2^(E + 1)), goes to [2^7, 2^8): 2^(7 - E)"""
    n = x.shape[1] - start if n is None else n
    top = 0.0
    for obj in range(x.shape[0]):
        idx = np.fromiter(_probed(obj, n), dtype=np.int64) + start
        top = max(top, float(np.max(np.abs(x[obj, idx]))))
    assert top > 0.0
    E = int(np.floor(np.log2(top)))
    return 7 - max(-60, min(20, E))


def overflow_share(x, k, span=64):
    """the share of the 64-sample wave spans of a call that hold a sample with |x| 2^k >= 65520 (their f16 totals are not finite)"""
    total = x.shape[1]
    hot = (np.abs(x.astype(np.float64)) * 2.0 ** k >= F16_OVERFLOW).any(axis=0)
    spans = [hot[s:s + span].any() for s in range(0, total, span)]
    return float(np.mean(spans))


def xcd_tile(b, n):
    """gain_kernels.h: workgroup index -> tile"""
    per = n >> 3
    return b if b >= per * 8 else (b & 7) * per + (b >> 3)


def workgroup_tiles(ntiles, wgs):
    """the tiles of every workgroup of k_gain_mix_p2 in the order it takes them (gain_p2.h: vb = b, b + wgs, ...; wgs 0: one each)"""
    wgs = ntiles if wgs <= 0 else min(wgs, ntiles)
    return [[xcd_tile(vb, ntiles) for vb in range(b, ntiles, wgs)] for b in range(wgs)]


def ramps_in_tile(times, t0, t1):
    """ramp segments of a curve (every segment between two different points of these scenes is one) that meet [t0, t1): what
    piece_walk (gain_p2.h) counts as the object's delta pieces of the tile"""
    t = np.asarray(times)
    a, b = t[:-1], t[1:]
    return int(np.sum((a < t1) & (b > t0) & (b > a)))


# per-object capacity of a tile's list: kPieceMaxPerObject = 15 delta pieces in the packed layout (gain_p2.h:79-82: "beyond: the
# exact path"; the lists are sized for it by CurveSet::piece_cap, curves.h:448-452), kPairMaxPerObject = 7 pairs in the paired one
# (gain_p2.h:98-100)
LIST_CAPACITY = {False: 15, True: 7}


def column_tiles(layout, buses):
    """ColumnPlan::make (curves.h:34-48): 16-column tiles per wave of the matrix-core kernels"""
    ncols = n_out(layout) * buses
    return 3 if (ncols + 47) // 48 > 1 else (ncols + 15) // 16


def carried(layout, buses, tile):
    """does k_gain_mix_p2 carry its pipeline through a workgroup's tiles (p2_persistent, gain_p2.h:517: every instantiation but the
    4-wave one — 256-sample tiles — with three column tiles)"""
    return not (tile == 256 and column_tiles(layout, buses) == 3)


# ---- group B / E: the long scenes ------------------------------------------------------------------------------------------------
LONG = dict(m=M, block=512, layout="9+10+3", level=1e-3, burst=1e4,
            cut_block=128, cut=149)  # the cut renders: blocks of 128, cut behind block 149 — sample 19072, 74.5 tiles of 256, 37.25 of 512
BUSY = ((3, 5), (40, 11), (69, 16), (10, 45), (20, 70), (21, 37))  # (object, samples between two curve points)


def long_blocks(tile, cus=CUS):
    """the fewest blocks of 512 of a call on 128 objects that picks its form on the device: ntiles x gsplit >= 2 cus with gsplit = 2
    (any call of fewer than 2 cus tiles), so `cus` tiles"""
    return -(-cus * tile // 512)


def long_calls(cus=CUS):
    """every cutting (a list of (first sample, samples)) a long scene is rendered under: the whole call and the call cut in two
    behind block LONG['cut'] of LONG['cut_block'] samples, for the length of either tile size"""
    out = []
    for tile in (256, 512):
        n, c = long_blocks(tile, cus) * 512, LONG["cut"] * LONG["cut_block"]
        out += [[(0, n)], [(0, c), (c, n - c)]]
    return out


def long_bursts(cus=CUS):
    """(object, first sample) of the bursts of three samples: the first 256-sample tile, the last one of the short (256-sample tiles)
    and of the long (512) call, a busy object alone in its tile, two ordinary objects alone, a busy and an ordinary one together —
    each moved on in steps of 8 until no probe of any cutting reads it"""
    hb, lb = long_blocks(256, cus), long_blocks(512, cus)
    at = lambda share: int(share * hb) * 512
    raw = [(50, 100), (3, at(0.16) + 300), (40, at(0.39) + 40), (77, at(0.39) + 104), (90, at(0.6) + 400), (5, at(0.78) + 10),
           (60, hb * 512 - 150), (61, lb * 512 - 150)]
    calls = [c for cutting in long_calls(cus) for c in cutting]
    out = []
    for obj, s in raw:
        while any(probed_in(obj, s + i, calls) for i in range(3)):
            s += 8
        out.append((obj, s))
    return out


def long_curves(kind, n, total):
    """`pieces`: ADM-like ramp-then-hold (period 700, ramp 150) with the six busy objects of test_piece_list_kernel_vs_oracle;
    `hinge`: always ramping (period = ramp = 240)"""
    if kind == "hinge":
        return scenes.adm_curves(M, n, total, period=240, ramp=240, seed=M)
    curves = scenes.adm_curves(M, n, total, period=700, ramp=150, seed=M)
    rng = np.random.default_rng(M)
    for i, step in BUSY:
        t = np.arange(-40, total + 40, step, dtype=np.int64)
        curves[i] = (t, rng.uniform(0, 1, (len(t), n)).astype(np.float32), rng.uniform(0, 1, (len(t), n)).astype(np.float32))
    return curves


Scene = namedtuple("Scene", "curves x dec delay want block total start")


def _oracle_render(curves, x, n, block, buses, layout):
    import _oracle
    from layouts import LAYOUTS
    if buses == 2:
        dec, delay = _oracle.design_decorrelators(LAYOUTS[layout]), _oracle.compensation_delay()
        o = _oracle.ObjectsRenderer(x.shape[0], n, block, dec, delay)
    else:  # direct bus only: zero decorrelators, no delay => the output is the direct bus exactly
        dec, delay = None, 0
        o = _oracle.ObjectsRenderer(x.shape[0], n, block, np.zeros((n, 1), np.float32), 0)
    zeros = {}
    for m, (t, d, f) in enumerate(curves):
        o.set_points(m, 0, t, d)
        o.set_points(m, 1, t, f if buses == 2 else zeros.setdefault(d.shape, np.zeros_like(d)))
    want = o.process(x)
    want.setflags(write=False)
    return dec, delay, want


@functools.lru_cache(maxsize=None)
def long_inputs(cus, bursts):
    total = long_blocks(512, cus) * 512
    x = (scenes.audio(M, total, seed=23) * np.float32(LONG["level"])).astype(np.float32)
    if bursts:
        for obj, s in long_bursts(cus):
            amp = np.float32(LONG["level"] * LONG["burst"]) * np.array([0.6, 0.7, 0.8], np.float32)
            x[obj, s:s + 3] = np.copysign(amp, x[obj, s:s + 3])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def long_scene(kind, cus=CUS, bursts=True, buses=2, nblocks=None, block=LONG["block"], layout=LONG["layout"]):
    """curves and inputs of the long scene of `cus` blocks of 512 (what the 512-sample tiles need; a call of 256-sample tiles renders
    the first half) and the oracle's render, in blocks of `block`, of its first `nblocks` x 512 samples (all of them by default), made
    once and read-only"""
    n, full = n_out(layout), long_blocks(512, cus) * 512
    total = full if nblocks is None else nblocks * 512
    curves = long_curves(kind, n, full)
    x = long_inputs(cus, bursts)[:, :total]
    dec, delay, want = _oracle_render(curves, x, n, block, buses, layout)
    return Scene(curves, x, dec, delay, want, block, total, 0)


def burst_mask(total, bursts, tile, reach):
    """the samples of a render that no burst reaches: outside the tile of each burst and the `reach` samples behind it (the
    decorrelators' length and the delay)"""
    quiet = np.ones(total, bool)
    for _, s in bursts:
        quiet[s // tile * tile:(s // tile + 1) * tile + reach] = False
    return quiet


# ---- groups C, D: the small scenes (scenes.split_paths_scene's sizes) -----------------------------------------------------------
SP = scenes.SPLIT_PATHS


@functools.lru_cache(maxsize=None)
def small_scene(kind, tile, layout, buses, full_scale):
    """scenes.split_paths_scene without bursts (`f32grid`: every point of every curve on the 512-sample grid and a call of whole
    512-sample tiles, 6 blocks of 256 — what plan_mix asks of the f32 grid kernel), rendered from sample SPLIT_PATHS['start']"""
    n = n_out(layout)
    if kind == "f32grid":
        nblocks = 6
        curves = scenes.dense_curves(M, n, 512, 3, seed=5)
        x = (scenes.audio(M, SP["block"] * nblocks, seed=23) * np.float32(1e-3)).astype(np.float32)
    else:
        nblocks = SP["nblocks"]
        curves, x = scenes.split_paths_scene(kind, n, False, tile)
    if full_scale:
        x = scenes.audio(M, SP["block"] * nblocks, seed=23)
    x.setflags(write=False)
    dec, delay, want = _oracle_render(curves, x, n, SP["block"], buses, layout)
    return Scene(curves, x, dec, delay, want, SP["block"], SP["block"] * nblocks, SP["start"])


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _pieces(tile, pairs, **more):
    return dict({"EARHIP_MFMA": "5", "EARHIP_P2_TILE": str(tile), "EARHIP_P2_PAIRS": str(pairs)}, **more)


def _hinge(tile, **more):
    return dict({"EARHIP_MFMA": "6", "EARHIP_HG_TILE": str(tile)}, **more)


def _grid(tile, **more):
    return dict({"EARHIP_MFMA": "4", "EARHIP_H2_TILE": str(tile)}, **more)


# the split-operand kernels, forced: (name, kernel, tile, list layout, options, curves of the small scenes)
SPLIT = [(f"grid-t{t}", GRID, t, None, _grid(t), "grid") for t in (256, 512)] + \
        [(f"pieces-t{t}-p{p}", PIECES, t, bool(p), _pieces(t, p), "pieces") for t in (256, 512) for p in (0, 1)] + \
        [(f"hinge-t{t}", HINGE, t, False, _hinge(t), "hinge") for t in (256, 512)]
LAYOUTS2 = ("0+5+0", "9+10+3")
XSCALES = (7, 16, 18)       # nothing / some wave spans / every wave span overflows (test_rare_paths_cpu.py holds them to that)
P2_WGS = ("0", "1", "3", "8")
WAYS = ("ostride", "obase", "istride", "ibase")
# ostride  output rows total + 1 floats apart, one bus, GSPLIT = 1
# obase    output rows 4 bytes off a 16-byte boundary, a stride that is a multiple of 4, one bus, GSPLIT = 1
# istride  input rows total + 1 floats apart, aligned outputs, two buses, GSPLIT unset: the objects split over parts
# ibase    input rows 4 bytes off, a stride that is a multiple of 4, one bus, GSPLIT unset


def _build():
    cases = []
    add = cases.append
    lay = LONG["layout"]
    # ---- B (9+10+3: three column tiles, the 256-sample tiles carry nothing; 0+5+0: one column tile, both tile sizes carry)
    for bl in (lay, "0+5+0"):
        for t in (256, 512):
            for p in (0, 1):
                o = _pieces(t, p, EARHIP_TAILCUT="0")
                cr = carried(bl, 2, t)
                add(Case(f"B-pieces-t{t}-p{p}-{bl}-plain", "B", PIECES, t, bl, 2, "plain", bool(p), o, ("pieces", True),
                         dict(gsplit=2, calls="whole", carried=cr)))
                add(Case(f"B-pieces-t{t}-p{p}-{bl}-gsplit1-wide", "B", PIECES, t, bl, 2, "wide", bool(p), dict(o, EARHIP_GSPLIT="1"), ("pieces", True),
                         dict(gsplit=1, calls="whole", carried=cr)))
                add(Case(f"B-pieces-t{t}-p{p}-{bl}-cut-wide", "B", PIECES, t, bl, 2, "wide", bool(p), o, ("pieces", True),
                         dict(gsplit=2, calls="cut", carried=cr)))
    for t in (256, 512):
        add(Case(f"B-hinge-t{t}-{lay}-plain", "B", HINGE, t, lay, 2, "plain", False, _hinge(t, EARHIP_TAILCUT="0"), ("hinge", True),
                 dict(gsplit=2, calls="whole")))
    # ---- C
    for name, kernel, t, paired, o, curves in SPLIT:
        for layout in LAYOUTS2:
            for k in XSCALES:
                add(Case(f"C-{name}-{layout}-xscale{k}-wide", "C", kernel, t, layout, 2, "wide", paired, dict(o, EARHIP_XSCALE=str(k)),
                         (curves, t, layout, 2, True), dict(gsplit=2, k=k)))
    # ---- D
    rows = [("valu-strict", VALU, 256, None, {}, "pieces", ("ostride", "obase", "ibase")),
            ("valu", VALU, 256, None, {"EARHIP_MFMA": "0"}, "pieces", ("istride", "ibase")),
            ("slots", SLOTS, 128, None, {"EARHIP_MFMA": "1"}, "pieces", WAYS),
            ("f32grid", F32GRID, 512, None, {"EARHIP_MFMA": "1"}, "f32grid", WAYS)] + [r + (WAYS,) for r in SPLIT]
    for name, kernel, t, paired, o, curves, ways in rows:
        for layout in LAYOUTS2:
            for way in ways:
                one = way in ("ostride", "obase")
                opts = dict(o, EARHIP_GSPLIT="1") if one else dict(o)
                form = "none" if kernel < GRID else "wide"
                add(Case(f"D-{name}-{layout}-{way}-{form}", "D", kernel, t, layout, 2 if way == "istride" else 1, form, paired, opts,
                         (curves, t, layout, 2 if way == "istride" else 1, False),
                         dict(way=way, strict=name == "valu-strict",  # (gsplit None: more than one — the slot and VALU kernels' own rule)
                              gsplit=1 if one or name == "valu-strict" else 2 if kernel >= F32GRID else None)))
    # ---- E (tile unset: the planner's — 256-sample tiles for the lists of a call this short, 512 for the hinge kernel)
    # One bus of 24 columns is two column tiles: the 4-wave kernel carries its pipeline with P2_WGS 1 (every tile in one workgroup's
    # run) and 8.  P2_WGS unset is the launch's own count, (2 CUs / gsplit) & ~7 workgroups (launch_pieces, api_core.hip:363) — as many
    # as this call has tiles: a workgroup per tile, nothing carried; the row pins the default launch, not the carried state.
    for p in (0, 1):
        for wgs in ("1", "8", None):
            o = {"EARHIP_MFMA": "5", "EARHIP_P2_PAIRS": str(p), "EARHIP_P2_WGS": wgs, "EARHIP_TAILCUT": "0"}
            add(Case(f"E-pieces-t256-p{p}-wgs{wgs or 'auto'}-{lay}-plain", "E", PIECES, 256, lay, 1, "plain", bool(p), o, ("pieces", False),
                     dict(gsplit=2, carried=wgs is not None)))
    add(Case(f"E-hinge-t512-{lay}-wide", "E", HINGE, 512, lay, 1, "wide", False, {"EARHIP_MFMA": "6", "EARHIP_TAILCUT": "0"}, ("hinge", False), dict(gsplit=2)))
    add(Case(f"E-hinge-t256-{lay}-plain", "E", HINGE, 256, lay, 1, "plain", False, _hinge(256, EARHIP_TAILCUT="0"), ("hinge", False), dict(gsplit=2)))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids)
    return cases


CASES = _build()
BY_GROUP = {g: [c for c in CASES if c.group == g] for g in "BCDE"}

# group E: (what, object) — an inf in an ordinary object, a NaN in a busy one (object 3: a point every 5 samples), each at an
# unprobed sample of an interior tile of the call of long_blocks(256) blocks
NON_FINITE = (("inf", 77), ("nan", 3))


def non_finite_sample(obj, cus=CUS):
    total = long_blocks(256, cus) * 512
    s = int(0.47 * long_blocks(256, cus)) * 512 + 300
    while probed_in(obj, s, [(0, total)]):
        s += 8
    return s
