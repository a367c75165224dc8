"""The case table of the extent panner's edges (k_pan_objects_extent, libear_amd/csrc/extent_kernels.h over extent.h), shared by
tests/test_extent_cases_cpu.py (the oracle's two cores against each other, the float64 model, the classification of
the chunks on the host) and tests/test_gpu_extent_edges.py (the device against libear's double core).

The kernel is the only one here that takes a shortcut its reference does not take: libear weighs all 1652 grid points for
every extent; the kernel sorts them into 26 chunks of 64 and classifies each chunk with one dot product (extent_chunk_class):
all points weigh 0 (skipped), all weigh 1 (a precomputed float sum), or the chunk is evaluated point by point.  That is sound
only if r_in and r_out of extent_setup bound the stadium-shaped weight function for every width and height.  A chunk classed
wrongly by 1e-3 rad costs a few points of weight about 5e-3 each: invisible at 1e-5 on an extent that holds hundreds of
weight-1 points, visible near the distance between libear's own float and double cores on an extent of ten points.

Plain Python: nothing here needs a device.  Every case is a set of arrays (az, el, dist, width, height, depth) with gain 1 and
diffuse 0, a name and what it claims.  Groups:
  1  sweeps: six directions x five height rules x widths 0 .. 360 in steps of 0.25 degrees (43,230 positions a layout: the
     oracle's two cores take 4 to 7 s a layout together).  Every chunk crosses both of its thresholds somewhere along each
     sweep.  tests/cpp/extent_host.cpp walks the same sweeps at 0.05 without the oracle.
  2  thresholds placed on purpose, at distances 1 and 0.5: the 10-degree blend, one dimension 0, no extent at a distance under
     1, is_circular at 1e-6 rad, the interpolation knots at 90, 180 and 360 degrees, 400 degrees.
  3  distance and depth: the near pass clamped at distance 0, the origin (where the direction is +y).
  4  poles: either side of the 1e-5 rule, where the azimuth decides the frame, with extents that are not circular.
  5  the widest layout the library takes (WIDE: 32 channels, 22 loudspeakers, LFE channels inside the list), against
     tests/extent_model.py.  A layout of 30 loudspeakers (TOO_WIDE) is refused: kMaxLayoutSpeakers is 22.
  6  batch structure: calls of 1, 3, 5, 127 and 129 positions in which every other position has no extent at distance 1, and one
     call of 2^18 + 5 positions (two batches of launch_objects).

The bar: per group and layout, e_lib is the worst distance (Eigen's isApprox measure per row) of libear's float core from its
double core over the group's positions, computed by reference() in the same run; the device's worst distance from the
double core is held to F x e_lib.  F = 1.5: the device adds the same float terms in another order (the suite's neighbouring
bars are 1.25 for the gain kernels and 1.5 for the block convolver).  E_LIB_MAX keeps a group from loosening its own bar."""
import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name group claim az el dist width height depth")

F = 1.5
E_LIB_MAX = 2e-6
E_LIB_MAX_SWEEP = 1.25e-6
SWEEP_STEP = 0.25
SWEEP_LAYOUTS = ("0+5+0", "9+10+3", "0+2+0")
EDGE_LAYOUTS = ("0+5+0", "9+10+3")  # (both have an LFE channel inside the list: real_of_full is not the identity)
DIRECTIONS = ((0.0, 0.0), (37.0, 12.0), (-110.0, 45.0), (180.0, -30.0), (10.0, 90.0), (64.0, -88.0))
HEIGHT_RULES = (("equal", lambda w: w), ("zero", lambda w: 0.0 * w), ("half", lambda w: w / 2.0),
                ("double", lambda w: np.minimum(2.0 * w, 360.0)), ("ninety", lambda w: 90.0 + 0.0 * w))


def _case(name, group, claim, rows):
    """rows: (az, el, dist, width, height, depth) each"""
    cols = [np.ascontiguousarray(c, np.float64) for c in np.array(rows, np.float64).reshape(-1, 6).T]
    for c in cols:
        c.setflags(write=False)
    return Case(name, group, claim, *cols)


def sweep_rows(step):
    """group 1 at a step in width: [(direction, rule name, rows)]"""
    widths = np.arange(0.0, 360.0 + step / 2, step)
    out = []
    for az, el in DIRECTIONS:
        for rule, fn in HEIGHT_RULES:
            rows = np.stack([np.full_like(widths, az), np.full_like(widths, el), np.ones_like(widths), widths, fn(widths),
                             np.zeros_like(widths)], axis=1)
            out.append(((az, el), rule, rows))
    return out


def _group1():
    return [_case(f"sweep az {az:g} el {el:g} height {rule}", 1,
                  "every chunk crosses its outside and its inside threshold along the sweep", rows)
            for (az, el), rule, rows in sweep_rows(SWEEP_STEP)]


FEW = ((0.0, 0.0), (37.0, 12.0), (-110.0, 45.0), (64.0, -88.0))


def _placed(name, claim, extents, dists=(1.0, 0.5), depth=0.0):
    rows = [(az, el, d, w, h, depth) for w, h in extents for d in dists for az, el in FEW]
    return _case(name, 2, claim, rows)


def _group2():
    circ = [(base + delta, base) for base in (40.0, 200.0)
            for delta in (1e-7, -1e-7, 5e-5, -5e-5, 1e-4, -1e-4, 2e-4, -2e-4, 1e-3, -1e-3)]
    knots = [v + dv for v in (90.0, 180.0, 360.0) for dv in (-0.01, 0.0, 0.01)]
    return [
        _placed("blend", "width = height around 10 degrees: the share of the spread part reaches 1 at 10 and stays",
                [(v, v) for v in (9.999, 10.0, 10.001)]),
        _placed("one dimension", "(w, 0) and (0, h): the other dimension is raised to half the fade; the frame is rotated for (0, h)",
                [(v, 0.0) for v in (3.0, 10.0, 40.0, 200.0)] + [(0.0, v) for v in (3.0, 10.0, 40.0, 200.0)]),
        _placed("no extent, near", "(0, 0) at a distance under 1 is spread: extent_mod widens it", [(0.0, 0.0)], dists=(0.5, 0.05, 0.9)),
        _placed("circular", "width - height around 40 and 200: is_circular switches at 1e-6 rad of the half sizes (1.15e-4 degrees here); "
                            "the two forms of the weight meet there", circ),
        _placed("knots", "width or height on the knots of the interpolations at 90, 180 and 360 degrees and one hundredth either side",
                [(v, 30.0) for v in knots] + [(30.0, v) for v in knots] + [(v, v) for v in knots]),
        _placed("beyond 360", "the entry points take 400 degrees as the oracle does: the interpolations hold their last value",
                [(400.0, 30.0), (30.0, 400.0), (400.0, 400.0)]),
    ]


DISTANCES = (0.0, 1e-12, 0.05, 0.5, 1.0, 2.0)


def _group3():
    widths = np.arange(0.0, 360.0 + 2.5, 5.0)
    out = []
    for az, el in ((37.0, 12.0), (-110.0, 45.0)):
        for rule, fn in HEIGHT_RULES[:1] + HEIGHT_RULES[2:3]:
            for dist in DISTANCES:
                # (AT the origin a rendering with a point-source share is 0 / 0 in libear: the far pass of depth 3, at distance
                # 1.5, is all spread from a width of 15 on — extent_mod(15, 1.5) = 10.1)
                rows = [(az, el, dist, w, h, dp) for dp in (0.0, 0.1, 1.0, 2.0 * dist, 3.0) for w, h in zip(widths, fn(widths))
                        if not (dist == 0.0 and dp == 3.0 and w < 15.0)]
                out.append(_case(f"az {az:g} el {el:g} height {rule} distance {dist:g}", 3,
                                 "depth renders a near and a far pass (the second job's weighting); the near pass clamps at "
                                 "distance 0; at the origin the direction is +y", rows))
    return out


def _group4():
    els = [s * v for v in (90.0, 90.0 - 1e-6, 90.0 - 1e-4) for s in (1.0, -1.0)]
    rows = [(az, el, 1.0, w, h, 0.0) for w, h in ((120.0, 20.0), (20.0, 120.0)) for el in els for az in (0.0, 45.0, 180.0)]
    return [_case("poles", 4, "within 1e-5 degrees of a pole the azimuth is taken as 0: it decides the frame of an extent that is "
                              "not circular", rows)]


@functools.lru_cache(maxsize=None)
def cases(group):
    return tuple({1: _group1, 2: _group2, 3: _group3, 4: _group4}[group]())


def layouts_of(group):
    return SWEEP_LAYOUTS if group == 1 else EDGE_LAYOUTS


def columns(cs):
    """the cases' arrays end to end -> dict of az, el, dist, width, height, depth"""
    return {k: np.concatenate([getattr(c, k) for c in cs]) for k in Case._fields[3:]}


def rel(a, b):
    """Eigen's isApprox measure per row: |a - b| / min(|a|, |b|)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.minimum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1))
    return np.linalg.norm(a - b, axis=1) / np.maximum(den, 1e-30)


Reference = namedtuple("Reference", "want e_lib worst_at")


def references(layout, v):
    """libear's double core at the positions v (columns()), and how far its float core is from it"""
    import _oracle
    o = _oracle.PolarExtent(layout)
    xyz = _oracle.cart(v["az"], v["el"], v["dist"])
    want = o.handle(xyz, v["width"], v["height"], v["depth"], which=1)
    lib = o.handle(xyz, v["width"], v["height"], v["depth"], which=0)
    want.setflags(write=False)
    e = rel(lib, want)
    return Reference(want, float(e.max()), int(e.argmax()))


@functools.lru_cache(maxsize=None)
def reference(group, layout):
    """computed once per group and layout, shared by every test that needs it, never written to"""
    return references(layout, columns(cases(group)))


def real_columns(layout):
    from layouts import LAYOUTS
    return [i for i, nm in enumerate(LAYOUTS[layout]) if not nm.startswith("LFE")]


# ---- group 5 ------------------------------------------------------------------------------------------------------------------------
def _wide(n_speakers_wanted):
    """rings of loudspeakers on three layers and one overhead, from the definitions of tests/custom_layout_model.py, with LFE
    channels inside the list up to 32 channels"""
    import custom_layout_model as model
    rings = {22: (model._ring("M", 36, 0), model._ring("U", 60, 35), model._ring("B", 72, -30)),
             30: (model._ring("M", 30, 0), model._ring("U", 40, 35), model._ring("B", 45, -30))}[n_speakers_wanted]
    speakers = rings[0] + rings[1] + rings[2] + [("T+000", 0.0, 90.0, False)]
    assert len(speakers) == n_speakers_wanted
    n_lfe = 32 - len(speakers)
    at = np.linspace(1, len(speakers) - 1, n_lfe).astype(int)  # (after which loudspeaker an LFE channel stands)
    out = []
    for k, ch in enumerate(speakers):
        out.append(ch)
        out += [(f"LFE{j + 1}", 45.0, -30.0, True) for j in np.flatnonzero(at == k + 1)]
    assert len(out) == 32 and not out[0][3] and not out[-1][3]
    return out


WIDE = _wide(22)      # the most loudspeakers a defined layout may have (kMaxLayoutSpeakers)
TOO_WIDE = _wide(30)  # refused: NOT_IMPLEMENTED


@functools.lru_cache(maxsize=None)
def wide_positions():
    """group 5: a coarse width sweep at two directions, two depths, and the directions of WIDE's loudspeakers (64 positions)"""
    rows = []
    for w in (0.0, 2.0, 4.0, 8.0, 10.0, 12.0, 20.0, 35.0, 45.0, 60.0, 90.0, 135.0, 180.0, 270.0, 300.0, 360.0):
        rows += [(37.0, 12.0, 1.0, w, w / 2.0, 0.0), (-110.0, 45.0, 0.7, w / 3.0, w, 0.0)]
    for dp in (0.3, 1.5):
        for w, h in ((0.0, 0.0), (15.0, 40.0), (90.0, 30.0), (200.0, 200.0), (5.0, 5.0)):
            rows.append((64.0, -20.0, 0.6, w, h, dp))
    for name, az, el, lfe in WIDE:
        if not lfe:
            rows.append((az, el, 1.0, 25.0, 12.0, 0.0) if len(rows) % 2 else (az, el, 1.0, 8.0, 8.0, 0.4))
    return _case("wide layout", 5, "32 channels: lane s carries output s up to the layout's last loudspeaker, and extent_write takes "
                                   "channel c's value from lane real_of_full[c], which is not c", rows)


# ---- group 6 ------------------------------------------------------------------------------------------------------------------------
CALL_SIZES = (1, 3, 5, 127, 129)


def small_call(n):
    """n positions, every other one with no extent at distance 1: the job index is not the position, and the last workgroup of
    four waves is part empty"""
    rng = np.random.default_rng(600 + n)
    az, el = rng.uniform(-180.0, 180.0, n), rng.uniform(-90.0, 90.0, n)
    spread = np.arange(n) % 2 == 0
    w, h = np.where(spread, rng.uniform(0.0, 120.0, n), 0.0), np.where(spread, rng.uniform(0.0, 120.0, n), 0.0)
    dist = np.where(spread, rng.choice([0.5, 1.0, 1.5], n), 1.0)
    depth = np.where(spread & (np.arange(n) % 4 == 0), 0.4, 0.0)
    return _case(f"call of {n}", 6, "jobs and positions are counted apart", np.stack([az, el, dist, w, h, depth], axis=1))


BATCH = 1 << 18  # kExtentBatch of launch_objects


def large_call():
    """2^18 + 5 positions with cheap extents (a handful of boundary chunks each): the second batch of launch_objects has
    batch-relative job positions, offset arrays and a job buffer used before"""
    rng = np.random.default_rng(66)
    n = BATCH + 5
    az, el = rng.uniform(-180.0, 180.0, n), np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n)))
    w, h = rng.uniform(0.0, 30.0, n), rng.uniform(0.0, 30.0, n)
    dist = rng.choice([0.5, 1.0, 2.0], n)
    depth = np.where(rng.uniform(0, 1, n) < 0.25, 0.5, 0.0)
    return _case("call of 2^18 + 5", 6, "the second iteration of the batch loop", np.stack([az, el, dist, w, h, depth], axis=1))
