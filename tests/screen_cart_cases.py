"""Inputs and the independent model of include/earhip.h group V (screenRef scaling and screenEdgeLock of Cartesian positions),
shared by tests/test_screen_cart_cpu.py and tests/test_gpu_screen_cart.py.

The model is tests/conv_model.py's point conversion to polar, tests/screen_model.py's scale and lock, conv_model's conversion
back: neither shares code with libear_amd/csrc.  The composition is well conditioned over the whole sweep (on 200,000 positions
of `batch` and the screen pairs below, the models alone: every finite position converts with status 0, outputs stay finite,
equal screens reproduce the input within 5e-11, and a 1e-12 perturbation of the input moves the output by at most 13e-12), so
the bar against the model is the conversion's own margin, LIBEAR_MARGIN = 1e-6 of tests/test_conversion.py, absolute."""
import numpy as np

import conv_model as CM
import screen_model as SM

ATOL = 1e-6  # LIBEAR_MARGIN of tests/test_conversion.py

# (reference, reproduction), as tests/test_gpu_screen.py pairs them; None: the default reference / no reproduction screen
PAIRS = ((None, SM.SCREEN_30), (SM.CART, SM.POLAR_15), (SM.OTHERS[0], SM.OTHERS[2]), (SM.POLAR_15, None))

# every combination of (screen_ref, lock_horizontal, lock_vertical) with a flag set
COMBOS = [(r, h, v) for r in (0, 1) for h in (0, 1, 2) for v in (0, 1, 2)][1:]


def _fixed_points():
    p = [(0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)]
    p += [(x, y, z) for x in (1.0, -1.0) for y in (1.0, -1.0) for z in (1.0, -1.0)]
    p += [(x, y, 0.0) for x in (1.0, -1.0) for y in (1.0, -1.0)]
    p += [(-0.0, 1.0, 0.0), (0.5, -0.0, 0.25), (-0.0, -0.0, -0.0), (0.3, 0.4, -0.0), (-0.0, -0.0, 0.75)]
    # either side of the conversion's 1e-10 centre rule
    p += [(1e-300, 1.0, 0.0), (0.0, -1.0, 1e-12), (5e-11, 5e-11, 0.5), (2e-10, 0.0, 0.5)]
    # converted azimuth exactly 0, -+30, -+110 and 180 (the sector seams), off the unit cube and off the horizontal plane
    p += [(0.0, 0.5, 0.3), (0.5, 0.5, 0.3), (-0.5, 0.5, -0.3), (1.5, -1.5, 0.25), (-1.5, -1.5, -2.0), (0.0, -0.75, 0.1)]
    # converted direction a reference screen's edge (corners and edge centres), by the model's conversion
    for s in (SM.DEFAULT, SM.CART, SM.OTHERS[0], SM.POLAR_15):
        left, right, bottom, top = SM.edges(s)
        for az, el, d in ((left, bottom, 0.8), (right, top, 1.25), (left, 0.0, 1.0), (0.5 * (left + right), top, 0.6)):
            (x, y, z), _ = CM.point_polar_to_cart(az, el, d)
            p.append((float(x), float(y), float(z)))
    return np.array(p)


FIXED = _fixed_points()


def batch(n, seed, invalid=False):
    """n seeded positions -> x, y, z (float64), screen_ref, lock_h, lock_v (uint8), bad (bool: what the stage refuses when it
    has a reproduction screen).  The batch starts with FIXED, every one of them flagged; the others are uniform in [-2, 2]^3,
    a third of them with no flag set, and a fifth of those hold NaN, an infinity or -0.0, which is nobody's business.
    invalid: every 23rd flagged element behind FIXED is one the stage refuses."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-2.0, 2.0, (n, 3))
    k = min(n, len(FIXED))
    xyz[:k] = FIXED[:k]
    combo = np.array(COMBOS)[rng.integers(0, len(COMBOS), n)]
    combo[:k] = np.array(COMBOS)[(np.arange(k) + seed) % len(COMBOS)]
    plain = rng.uniform(0, 1, n) < 1.0 / 3.0
    plain[:k] = False
    combo[plain] = 0
    ref, lh, lv = (np.ascontiguousarray(combo[:, j], np.uint8) for j in range(3))
    odd = np.flatnonzero(plain & (rng.uniform(0, 1, n) < 0.2))
    for j, i in enumerate(odd):
        xyz[i, j % 3] = (np.nan, np.inf, -np.inf, -0.0)[j % 4]
    bad = np.zeros(n, bool)
    if invalid:
        chosen = np.flatnonzero(~plain)
        chosen = chosen[chosen >= k][::23]
        bad[chosen] = True
        for j, i in enumerate(chosen):
            kind = j % 6
            if kind < 4:
                xyz[i, j % 3] = (np.nan, np.inf, -np.inf, np.nan)[kind]
            elif kind == 4:
                lh[i] = 3
            else:
                lv[i] = 200
    x, y, z = (np.ascontiguousarray(xyz[:, j]) for j in range(3))
    return x, y, z, ref, lh, lv, bad


def flagged(n, ref, lh, lv):
    """which elements have a flag set, a None array standing for what NULL means"""
    f = np.ones(n, bool) if ref is None else ref != 0
    for a in (lh, lv):
        if a is not None:
            f = f | (a != 0)
    return f


def finite(x, y, z):
    """the batch for a call with screen_ref NULL, where every element is flagged: the oddities of unflagged ones replaced"""
    return tuple(np.where(np.isfinite(a), a, 0.625) for a in (x, y, z))


def model(x, y, z, reproduction, reference=None, ref=None, lh=None, lv=None):
    """-> (x, y, z) of the independent model; unflagged elements, and all without a reproduction screen, are the inputs"""
    x, y, z = (np.asarray(a, np.float64) for a in (x, y, z))
    if reproduction is None:
        return x, y, z
    f = flagged(x.size, ref, lh, lv)
    (az, el, d), st = CM.point_cart_to_polar(np.where(f, x, 0.5), np.where(f, y, 0.5), np.where(f, z, 0.5))
    assert (st == 0).all()
    az, el = SM.apply(az, el, reproduction, reference, ref, lh, lv)
    (mx, my, mz), st = CM.point_polar_to_cart(az, el, d)
    assert (st == 0).all()
    return np.where(f, mx, x), np.where(f, my, y), np.where(f, mz, z)
