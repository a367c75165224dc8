"""ear::conversion through the host forms of earhip group K (capi.to_polar / capi.to_cartesian): no GPU needed.

libear's own cases (tests/conversion_tests.cpp) at its margin of 1e-6, a seeded sweep of 2^17 positions and extents
against the independent numpy restatement (tests/conv_model.py), the error cases and the pointer cases of the C ABI.
The wrapper semantics of toPolar / toCartesian are checked by the drop-in program (test_dropin_conversion.py)."""
import ctypes as C
import time

import numpy as np
import pytest

import conv_model as M
from libear_amd import capi

LIBEAR_MARGIN = 1e-6


# --- libear's own cases ---------------------------------------------------------------------------------------------

def test_conversion_reference():
    (p, e) = capi.to_cartesian([10.0], [20.0], [0.3], [40.0], [50.0], [0.6])
    np.testing.assert_allclose(np.ravel(p), [-0.08972503721988338, 0.3, 0.1732050807568877], rtol=0, atol=LIBEAR_MARGIN)
    np.testing.assert_allclose(np.ravel(e), [0.35166171614357594, 0.4470181645863707, 0.5762749096794243], rtol=0,
                               atol=LIBEAR_MARGIN)
    (p, e) = capi.to_polar([0.9], [0.8], [0.1], [0.3], [0.5], [0.4])
    np.testing.assert_allclose(np.ravel(p), [-34.85107611658391, 4.226794497273273, 0.9000000000000001], rtol=0,
                               atol=LIBEAR_MARGIN)
    np.testing.assert_allclose(np.ravel(e), [76.50724453298275, 104.9708107421662, 0.1756348204517474], rtol=0,
                               atol=LIBEAR_MARGIN)


def test_conversion_cartesian_polar_loop():
    az, el, d = np.meshgrid([0.0, -10.0, 10.0, 90.0, -90.0, 150.0, -150.0], [0.0, -10.0, 10.0, -45.0, 45.0, -90.0, 90.0],
                            [0.5, 1.0], indexing="ij")
    az, el, d = az.ravel(), el.ravel(), d.ravel()
    assert az.size == 7 * 7 * 2
    x, y, z = capi.to_cartesian(az, el, d)
    az2, el2, d2 = capi.to_polar(x, y, z)
    # libear's check_polar_equal compares the azimuth only where |el| < 90 - 1e6, i.e. never; here it is compared
    # wherever it is defined (away from the poles)
    off_pole = np.abs(el) < 90.0
    np.testing.assert_allclose(az2[off_pole], az[off_pole], rtol=0, atol=LIBEAR_MARGIN)
    np.testing.assert_allclose(el2, el, rtol=0, atol=LIBEAR_MARGIN)
    np.testing.assert_allclose(d2, d, rtol=0, atol=LIBEAR_MARGIN)


def test_conversion_poles():
    for sign in (-1.0, 1.0):
        for d in (0.5, 1.0, 2.0):
            np.testing.assert_allclose(np.ravel(capi.to_cartesian([0.0], [sign * 90.0], [d])), [0.0, 0.0, sign * d],
                                       rtol=0, atol=LIBEAR_MARGIN)
            np.testing.assert_allclose(np.ravel(capi.to_polar([0.0], [0.0], [sign * d])), [0.0, sign * 90.0, d],
                                       rtol=0, atol=LIBEAR_MARGIN)


def test_conversion_centre():
    az, el = np.meshgrid([-90.0, 0.0, 90.0], [-90.0, 0.0, 90.0])
    x, y, z = capi.to_cartesian(az.ravel(), el.ravel(), np.zeros(9))
    np.testing.assert_allclose(np.stack([x, y, z]), 0.0, rtol=0, atol=LIBEAR_MARGIN)
    assert abs(capi.to_polar([0.0], [0.0], [0.0])[2][0]) <= LIBEAR_MARGIN


@pytest.mark.parametrize("az,el,cart_whd", [(0.0, 0.0, "whd"), (90.0, 0.0, "dhw"), (-90.0, 0.0, "dhw"),
                                            (180.0, 0.0, "whd"), (0.0, 90.0, "wdh"), (0.0, -90.0, "wdh")])
def test_conversion_whd_mapping(az, el, cart_whd):
    def axis(ext):
        return "whd"[int(np.argmax([v[0] for v in ext]))]
    for polar_axis, cart_axis in zip("whd", cart_whd):
        _, ext = capi.to_cartesian([az], [el], [1.0], [20.0 if polar_axis == "w" else 0.0],
                                   [20.0 if polar_axis == "h" else 0.0], [0.2 if polar_axis == "d" else 0.0])
        assert axis(ext) == cart_axis
        pos = capi.to_cartesian([az], [el], [1.0])
        _, ext = capi.to_polar(*pos, [0.1 if cart_axis == "w" else 0.0], [0.1 if cart_axis == "h" else 0.0],
                               [0.1 if cart_axis == "d" else 0.0])
        assert axis(ext) == polar_axis


# --- seeded sweep against the model ---------------------------------------------------------------------------------

N_SWEEP = 1 << 17
SPECIAL_AZ = [3600.25, -3600.25, 1e6 + 0.1, -1e6 - 0.1, 180.0, -180.0, 360.0, -360.0, 540.0, 720.0, -0.0, 0.0,
              -30.0, -110.0, 110.0, 30.0, 2.0 ** 40, -(2.0 ** 40)]
SPECIAL_EL = [30.0, -30.0, 90.0, -90.0, 100.0, -100.0, 0.0, 45.0]

# Points where asin / acos are evaluated at +-1, whose slope there turns one ulp of difference in a sine or cosine
# into ~1e-6 degrees: Cartesian extents of exactly 1 (and 0) along the axes, at the poles and the cardinal
# directions, where a size of the rotated extent comes out at 1 or at 1 - 1 ulp.  Only these use libear's margin.
DEGENERATE_POS = [(0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0),
                  (0.0, 0.0, -1.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0)]
DEGENERATE_EXT = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 0.0),
                  (0.5, 1.0, 0.0)]


def polar_sweep(n=N_SWEEP, seed=2127):
    """(az, el, dist, width, height, depth) [n]: random polar metadata with the edges mixed in"""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-720.0, 720.0, n)
    az[: n // 8] = rng.choice(SPECIAL_AZ, n // 8) + rng.choice([0.0, 0.0, 1e-9, -1e-9], n // 8)
    az[n // 8: n // 4] = rng.uniform(-1e7, 1e7, n // 8)
    el = rng.uniform(-95.0, 95.0, n)
    el[n // 4: n // 4 + n // 8] = rng.choice(SPECIAL_EL, n // 8)
    dist = rng.uniform(0.0, 2.0, n)
    dist[rng.random(n) < 0.05] = 0.0
    w, h = rng.uniform(0.0, 360.0, n), rng.uniform(0.0, 360.0, n)
    for a in (w, h):
        sel = rng.random(n) < 0.15
        a[sel] = rng.choice([0.0, 180.0, 360.0], sel.sum())
    d = rng.uniform(0.0, 1.0, n)
    d[rng.random(n) < 0.1] = 0.0
    return az, el, dist, w, h, d


def cart_sweep(n=N_SWEEP, seed=2051):
    """(x, y, z, width, height, depth) [n]: random Cartesian metadata (extents below 1: no asin / acos at +-1),
    with the axes, the origin and the poles mixed in"""
    rng = np.random.default_rng(seed)
    x, y, z = (rng.uniform(-1.5, 1.5, n) for _ in range(3))
    sel = rng.random(n) < 0.1
    for a in (x, y, z):
        a[sel] = rng.choice([0.0, 1.0, -1.0, 1e-11, 0.5], sel.sum())
    w, h, d = (rng.uniform(0.0, 0.999, n) for _ in range(3))
    for a in (w, h, d):
        a[rng.random(n) < 0.1] = 0.0
    return x, y, z, w, h, d


def degenerate_cart():
    pts = [p + e for p in DEGENERATE_POS for e in DEGENERATE_EXT]
    return tuple(np.array(v) for v in zip(*pts))


def assert_close(got, want, atol, what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.flatnonzero(np.isnan(got) != np.isnan(want))[:8])
    with np.errstate(invalid="ignore"):
        err = np.where(np.isnan(want), 0.0, np.abs(got - want))
    bad = np.flatnonzero(err > atol)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]], err.max())


def test_polar_to_cartesian_sweep_matches_model():
    az, el, dist, w, h, d = polar_sweep()
    (mp, me, st) = M.extent_polar_to_cart(az, el, dist, w, h, d)
    assert (st == M.OK).all()  # |az| <= 2^40: every element converts
    (p, e) = capi.to_cartesian(az, el, dist, w, h, d)
    scale = np.maximum(1.0, dist)
    for k, name in enumerate("xyz"):
        assert_close(p[k], mp[k], 1e-12 * scale, name)
    for k, name in enumerate(("width", "height", "depth")):
        assert_close(e[k], me[k], 1e-9, name)
    # the point form gives the same positions, bit for bit
    for a, b in zip(capi.to_cartesian(az, el, dist), p):
        assert np.array_equal(a, b, equal_nan=True)


def test_cartesian_to_polar_sweep_matches_model():
    x, y, z, w, h, d = cart_sweep()
    (mp, me, st) = M.extent_cart_to_polar(x, y, z, w, h, d)
    assert (st == M.OK).all()
    (p, e) = capi.to_polar(x, y, z, w, h, d)
    scale = np.maximum(1.0, p[2])
    for k, name in enumerate(("azimuth", "elevation", "distance")):
        assert_close(p[k], mp[k], 1e-12 * scale, name)
    for k, name in enumerate(("width", "height", "depth")):
        assert_close(e[k], me[k], 1e-9, name)


def test_degenerate_points_within_libear_margin():
    x, y, z, w, h, d = degenerate_cart()
    (mp, me, _) = M.extent_cart_to_polar(x, y, z, w, h, d)
    (p, e) = capi.to_polar(x, y, z, w, h, d)
    for k in range(3):
        assert_close(p[k], mp[k], 1e-12 * np.maximum(1.0, p[2]), "position")
        assert_close(e[k], me[k], LIBEAR_MARGIN, "extent")


def libear_reduce(x, lo):
    """libear's relativeAngle loop, literally (terminates for the moderate values it is used on here)"""
    while x - 360.0 >= lo:
        x -= 360.0
    while x < lo:
        x += 360.0
    return x


@pytest.mark.parametrize("az", [3600.25, -3600.25, 1e6 + 0.1, -1e6 - 0.1, 720.0, -720.0, 1e5 + 1e-7])
def test_bounded_reduction_equals_libear_loops(az):
    """fmod-based reduction: the same value as libear's loops, so the point form gives what it gives for the
    reduced azimuth, bit for bit (the extent part evaluates sin / cos of the azimuth as given, as libear does)"""
    r = libear_reduce(az, -180.0)
    got = capi.to_cartesian([az], [20.0], [1.0])
    want = capi.to_cartesian([r], [20.0], [1.0])
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


# --- errors ---------------------------------------------------------------------------------------------------------

def test_nan_azimuth_is_internal_error_naming_the_index():
    with pytest.raises(capi.InternalError) as e:
        capi.to_cartesian([0.0, 10.0, 20.0, np.nan], [0.0] * 4, [1.0] * 4)
    assert "element 3" in str(e.value) and "sector" in str(e.value)
    with pytest.raises(capi.InternalError) as e:
        capi.to_polar([1.0, np.nan], [0.0, 1.0], [0.0, 0.0])
    assert "element 1" in str(e.value)


@pytest.mark.parametrize("az", [np.inf, -np.inf, 2.0 ** 40 * 1.5, -1e300, np.nextafter(2.0 ** 40, np.inf)])
def test_infinite_or_huge_azimuth_is_invalid_argument_and_returns_promptly(az):
    t0 = time.monotonic()
    with pytest.raises(capi.InvalidArgument) as e:
        capi.to_cartesian([0.0, az], [0.0, 0.0], [1.0, 1.0], [10.0, 10.0], [0.0, 0.0], [0.0, 0.0])
    assert time.monotonic() - t0 < 1.0
    assert "element 1" in str(e.value)


def test_largest_accepted_azimuth_converts():
    for az in (2.0 ** 40, -(2.0 ** 40)):
        (p, _), ((mp, _, st)) = capi.to_cartesian([az], [0.0], [1.0], [10.0], [0.0], [0.0]), \
            M.extent_polar_to_cart(np.array([az]), 0.0, 1.0, 10.0, 0.0, 0.0)
        assert st[0] == M.OK and np.isfinite(p[0][0])


def test_cartesian_infinities_propagate_nan_as_libear():
    x = np.array([np.inf, -np.inf, 0.5, 0.5, np.inf, 0.0])
    y = np.array([1.0, 0.5, np.inf, 0.5, np.inf, 0.0])
    z = np.array([0.0, 0.0, 0.0, np.inf, 0.0, -np.inf])
    w = np.full(6, 0.2)
    (p, e) = capi.to_polar(x, y, z, w, w, w)
    (mp, me, st) = M.extent_cart_to_polar(x, y, z, w, w, w)
    assert (st == M.OK).all()
    assert np.isnan(p[0]).any()
    for k in range(3):
        assert np.array_equal(np.isnan(p[k]), np.isnan(mp[k]))
        assert np.array_equal(np.isnan(e[k]), np.isnan(me[k]))
        assert_close(p[k], mp[k], 1e-9, "position")


# --- pointer cases --------------------------------------------------------------------------------------------------

def _call(fn, n, ins, ext_in, outs, ext_out):
    f64 = C.POINTER(C.c_double)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(f64)
    return fn(C.c_size_t(n), *[ptr(a) for a in ins], *[ptr(a) for a in ext_in], *[ptr(a) for a in outs],
              *[ptr(a) for a in ext_out])


@pytest.mark.parametrize("direction", ["to_polar", "to_cartesian"])
def test_in_place_equals_separate_buffers(direction):
    lib = capi.load()
    fn = getattr(lib, "earhip_conversion_" + direction)
    src = cart_sweep(4096, 7) if direction == "to_polar" else polar_sweep(4096, 7)
    sep_out = [np.empty(4096) for _ in range(6)]
    assert _call(fn, 4096, src[:3], src[3:], sep_out[:3], sep_out[3:]) == capi.OK
    arrs = [a.copy() for a in src]
    assert _call(fn, 4096, arrs[:3], arrs[3:], arrs[:3], arrs[3:]) == capi.OK
    for a, b in zip(arrs, sep_out):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("direction", ["to_polar", "to_cartesian"])
def test_null_extents_equal_point_forms(direction):
    lib = capi.load()
    fn = getattr(lib, "earhip_conversion_" + direction)
    src = cart_sweep(4096, 9) if direction == "to_polar" else polar_sweep(4096, 9)
    point = [np.empty(4096) for _ in range(3)]
    assert _call(fn, 4096, src[:3], [None] * 3, point, [None] * 3) == capi.OK
    full = [np.empty(4096) for _ in range(6)]
    assert _call(fn, 4096, src[:3], [None] * 3, full[:3], full[3:]) == capi.OK  # extents in: NULL means 0
    zeros = [np.zeros(4096) for _ in range(3)]
    full0 = [np.empty(4096) for _ in range(6)]
    assert _call(fn, 4096, src[:3], zeros, full0[:3], full0[3:]) == capi.OK
    for a, b, c in zip(point, full[:3], full0[:3]):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
    for a, b in zip(full[3:], full0[3:]):
        assert np.array_equal(a, b, equal_nan=True)


def test_null_positions_and_partial_extent_outputs_are_refused():
    lib = capi.load()
    a = [np.zeros(4) for _ in range(6)]
    assert _call(lib.earhip_conversion_to_polar, 4, [a[0], None, a[2]], [None] * 3, a[3:], [None] * 3) \
        == capi.INVALID_ARGUMENT
    assert _call(lib.earhip_conversion_to_polar, 4, a[:3], [None] * 3, a[3:], [a[0], None, None]) \
        == capi.INVALID_ARGUMENT
    assert _call(lib.earhip_conversion_to_polar, 0, a[:3], [None] * 3, a[3:], [None] * 3) == capi.OK
