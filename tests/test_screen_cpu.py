"""The host forms of include/earhip.h group R (screenRef scaling and screenEdgeLock), without a device: known edges and
scalings, the results that are exact, earhip_screen_apply against the model of tests/screen_model.py, every refusal, the
bindings, and the shared core (libear_amd/csrc/screen.h) on the CPU under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import screen_model as M
from libear_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_screen(s):
    if s is None:
        return None
    if "x" in s:
        return capi.Screen.cart(s["aspect"], s["x"], s["y"], s["z"], s["width_x"])
    return capi.Screen.polar(s["aspect"], s["az"], s["el"], s["dist"], s["width"])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


KNOWN_EDGES = (
    (M.DEFAULT, (29.0, -29.0, -17.29708889245067, 17.29708889245067)),
    (M.POLAR_15, (0.283559454529715, -40.283559454529716, -3.639039283545732, 23.63903928354573)),
    (M.CART, (26.56505117707799, -26.56505117707799, -15.689992929083877, 15.689992929083877)),
    (M.SCREEN_30, (15.0, -15.0, -8.560644163419065, 8.560644163419065)),
)


@pytest.mark.parametrize("screen,want", KNOWN_EDGES)
def test_known_edges(screen, want):
    got = capi.screen_edges(c_screen(screen))
    assert np.max(np.abs(np.array(got) - np.array(want))) <= 1e-10, got
    assert np.max(np.abs(np.array(M.edges(screen)) - np.array(want))) <= 1e-10


def test_default_screen():
    s = capi.screen_default()
    assert (s.cartesian, s.aspect_ratio, s.azimuth, s.elevation, s.distance, s.width_azimuth) == (0, 1.78, 0.0, 0.0, 1.0, 58.0)
    assert capi.screen_edges(s) == capi.screen_edges(c_screen(M.DEFAULT))
    for s in M.ALL:  # the model's screens are ones the stage accepts
        left, right, bottom, top = capi.screen_edges(c_screen(s))
        assert -180 < right < left < 180 and -90 < bottom < top < 90


KNOWN_SCALINGS = (
    (M.DEFAULT, M.SCREEN_30, (90.0, 45.0), (81.65562913907284, 39.59251346586589)),
    (M.DEFAULT, M.SCREEN_30, (14.5, -8.0), (7.5, -3.9593456293817697)),
    (M.DEFAULT, M.SCREEN_30, (-100.0, -50.0), (-92.58278145695364, -45.1933453029919)),
    (M.DEFAULT, M.POLAR_15, (0.0, 0.0), (-20.0, 10.0)),
    (M.DEFAULT, M.POLAR_15, (90.0, 45.0), (72.88424073448789, 48.92539670353921)),
    (M.CART, M.DEFAULT, (90.0, 45.0), (91.42826256823597, 45.97321102772186)),
)


@pytest.mark.parametrize("ref,rep,src,want", KNOWN_SCALINGS)
def test_known_scalings(ref, rep, src, want):
    az, el = capi.screen_apply([src[0]], [src[1]], c_screen(rep), c_screen(ref))
    assert abs(az[0] - want[0]) <= 1e-10 and abs(el[0] - want[1]) <= 1e-10, (az[0], el[0])
    # a NULL reference is the default screen
    if ref is M.DEFAULT:
        az2, el2 = capi.screen_apply([src[0]], [src[1]], c_screen(rep))
        assert az2[0] == az[0] and el2[0] == el[0]


def test_exact_results():
    for ref, rep in ((M.DEFAULT, M.SCREEN_30), (M.CART, M.POLAR_15), (M.OTHERS[0], M.OTHERS[1])):
        cr, cp = c_screen(ref), c_screen(rep)
        rl, rr, rb, rt = capi.screen_edges(cr)
        pl, pr, pb, pt = capi.screen_edges(cp)
        # the seam and the poles map to themselves
        az, el = capi.screen_apply([180.0, -180.0, 180.0, -180.0], [90.0, -90.0, -90.0, 90.0], cp, cr)
        assert az.tolist() == [180.0, -180.0, 180.0, -180.0] and el.tolist() == [90.0, -90.0, -90.0, 90.0]
        # a reference edge maps to the reproduction edge
        az, el = capi.screen_apply([rl, rr], [rb, rt], cp, cr)
        assert az.tolist() == [pl, pr] and el.tolist() == [pb, pt]
        # a locked component equals the reproduction edge, scaled or not; the other component is untouched or scaled
        src_az, src_el = np.array([12.25, -70.0, 400.0, 5.0]), np.array([3.0, -30.0, 60.0, 1.0])
        for ref_flag in (0, 1):
            az, el = capi.screen_apply(src_az, src_el, cp, cr, ref_flag, [1, 2, 0, 0], [0, 0, 1, 2])
            assert az[:2].tolist() == [pl, pr] and el[2:].tolist() == [pb, pt]
            if ref_flag:
                saz, sel = capi.screen_apply(src_az, src_el, cp, cr)
                assert np.array_equal(bits(az[2:]), bits(saz[2:])) and np.array_equal(bits(el[:2]), bits(sel[:2]))
            else:  # not even reduced: 400 stays 400
                assert np.array_equal(bits(az[2:]), bits(src_az[2:])) and np.array_equal(bits(el[:2]), bits(src_el[:2]))
    # untouched elements keep their bits, whatever they hold
    odd = np.array([np.nan, np.inf, 1e300, -0.0, 389.0])
    odd_el = np.array([-np.inf, 1234.0, np.nan, -0.0, 91.0])
    az, el = capi.screen_apply(odd, odd_el, c_screen(M.SCREEN_30), None, 0)
    assert np.array_equal(bits(az), bits(odd)) and np.array_equal(bits(el), bits(odd_el))
    # no reproduction screen: copies, flags or not
    az, el = capi.screen_apply(odd, odd_el, None, None, 1, 1, 2)
    assert np.array_equal(bits(az), bits(odd)) and np.array_equal(bits(el), bits(odd_el))
    # an azimuth of 389 scales as 29; so does one a thousand turns on
    az, el = capi.screen_apply([389.0, 29.0, 29.0 - 360000.0, 29.0 - 360.0], [0.0] * 4, c_screen(M.SCREEN_30))
    assert az[0] == az[1] == az[2] == az[3] and abs(az[0] - 15.0) <= 1e-10
    az, el = capi.screen_apply([372.0, 12.0, -348.0], [0.0] * 3, c_screen(M.SCREEN_30))
    assert az[0] == az[1] == az[2] and 0.0 < az[0] < 15.0


def test_host_form_matches_the_model():
    """4,096 seeded elements over pairs of screens, flags and locks.  Bound: 1e-12 degrees absolute, derived: the host form
    and np.interp differ by roundings of values no larger than 180, whose spacing is 2.9e-14."""
    n = 4096
    az, el, ref, lh, lv, _ = M.mixed_batch(n, seed=7331)
    pairs = [(a, b) for a in M.ALL for b in M.ALL][::3]
    worst = 0.0
    for k, (r, p) in enumerate(pairs):
        sl = slice(k * n // len(pairs), (k + 1) * n // len(pairs))
        got = capi.screen_apply(az[sl], el[sl], c_screen(p), c_screen(r), ref[sl], lh[sl], lv[sl])
        want = M.apply(az[sl], el[sl], p, r, ref[sl], lh[sl], lv[sl])
        for g, w in zip(got, want):
            assert np.array_equal(np.isnan(g), np.isnan(w))
            same = bits(g) == bits(w)
            with np.errstate(invalid="ignore"):
                err = np.where(same, 0.0, np.abs(g - w))
            worst = max(worst, float(np.nanmax(err)))
    print(f"host form vs model: worst difference {worst:.3e} degrees over {len(pairs)} screen pairs")
    assert worst <= 1e-12


def refused(fn, *words):
    with pytest.raises(capi.InvalidArgument) as e:
        fn()
    assert e.value.code == capi.INVALID_ARGUMENT
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refused_screens():
    P = capi.Screen.polar
    bad = (
        (P(1.78, 170.0, 0.0, 1.0, 58.0), "edges"),          # across the rear seam
        (P(1.78, -170.0, 0.0, 1.0, 58.0), "edges"),
        (P(0.0, 0.0, 0.0, 1.0, 58.0), "aspect_ratio"),
        (P(-1.78, 0.0, 0.0, 1.0, 58.0), "aspect_ratio"),
        (P(1.78, 0.0, 0.0, 1.0, 180.0), "width_azimuth"),
        (P(1.78, 0.0, 0.0, 1.0, 0.0), "width_azimuth"),
        (P(1.78, 0.0, 0.0, 0.0, 58.0), "distance"),
        (P(1.78, 0.0, 91.0, 1.0, 58.0), "elevation"),
        (P(float("nan"), 0.0, 0.0, 1.0, 58.0), "aspect_ratio"),
        (P(1.78, float("nan"), 0.0, 1.0, 58.0), "azimuth"),
        (P(1.78, 0.0, 0.0, float("inf"), 58.0), "distance"),
        (P(1.78, 0.0, 0.0, 1.0, float("nan")), "width_azimuth"),
        (capi.Screen.cart(1.78, 0.0, 1.0, 0.0, 0.0), "width_x"),
        (capi.Screen.cart(1.78, 0.0, 1.0, 0.0, -1.0), "width_x"),
        (capi.Screen.cart(1.78, 0.0, float("nan"), 0.0, 1.0), "y"),
        (capi.Screen.cart(1.78, -1.0, -0.2, 0.0, 1.0), "edges"),  # left of and behind the listener: right > left
    )
    good = c_screen(M.SCREEN_30)
    for s, field in bad:
        refused(lambda: capi.screen_edges(s), field)
        refused(lambda: capi.screen_apply([0.0], [0.0], s), "reproduction", field)
        refused(lambda: capi.screen_apply([0.0], [0.0], good, s), "reference", field)
        refused(lambda: capi.screen_apply([0.0], [0.0], None, s), "reference", field)
    # the fields of the other kind are not read
    s = capi.Screen.polar(1.78, 0.0, 0.0, 1.0, 58.0)
    s.x = s.width_x = float("nan")
    assert capi.screen_edges(s) == capi.screen_edges(capi.screen_default())


def test_refused_elements_are_named_and_the_elements_before_them_written():
    lib = capi.load()
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    rep = c_screen(M.SCREEN_30)
    base_az, base_el = np.array([14.5, 29.0, -100.0, 50.0, 60.0]), np.array([-8.0, 0.0, -50.0, 5.0, 6.0])
    want = capi.screen_apply(base_az, base_el, rep)
    cases = (("az", float("inf")), ("az", float("-inf")), ("az", float("nan")), ("az", 2.0 ** 40 * 1.5), ("el", 90.0000001),
             ("el", -91.0), ("el", float("nan")), ("lh", 3), ("lv", 3), ("lv", 255))
    for where, value in cases:
        az, el = base_az.copy(), base_el.copy()
        lh, lv = np.zeros(5, np.uint8), np.zeros(5, np.uint8)
        {"az": az, "el": el, "lh": lh, "lv": lv}[where][3] = value
        refused(lambda: capi.screen_apply(az, el, rep, None, None, lh, lv), "element 3")
        out_az, out_el = np.full(5, -1000.0), np.full(5, -2000.0)
        rc = lib.earhip_screen_apply(None, C.byref(rep), C.c_size_t(5), az.ctypes.data_as(dp), el.ctypes.data_as(dp), None,
                                     lh.ctypes.data_as(bp), lv.ctypes.data_as(bp), out_az.ctypes.data_as(dp),
                                     out_el.ctypes.data_as(dp))
        assert rc == capi.INVALID_ARGUMENT and b"element 3" in lib.earhip_last_error()
        assert np.array_equal(out_az[:3], want[0][:3]) and np.array_equal(out_el[:3], want[1][:3])
        assert out_az[3:].tolist() == [-1000.0] * 2 and out_el[3:].tolist() == [-2000.0] * 2
    # the same values in an element with no flag set are nobody's business
    az, el = base_az.copy(), base_el.copy()
    az[3], el[3] = float("inf"), 500.0
    flags = np.array([1, 1, 1, 0, 1], np.uint8)
    got = capi.screen_apply(az, el, rep, None, flags)
    assert got[0][3] == float("inf") and got[1][3] == 500.0 and got[0][4] == capi.screen_apply([60.0], [6.0], rep)[0][0]
    # 2^40 itself is accepted
    capi.screen_apply([2.0 ** 40], [0.0], rep)
    # NULL arrays, too many elements; n == 0 needs no arrays
    one = np.zeros(1)
    p = one.ctypes.data_as(dp)
    assert lib.earhip_screen_apply(None, C.byref(rep), C.c_size_t(1), None, p, None, None, None, p, p) == capi.INVALID_ARGUMENT
    assert lib.earhip_screen_apply(None, C.byref(rep), C.c_size_t(1), p, p, None, None, None, p, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_screen_apply(None, C.byref(rep), C.c_size_t(1 << 31), p, p, None, None, None, p, p) == capi.INVALID_ARGUMENT
    assert lib.earhip_screen_apply(None, C.byref(rep), C.c_size_t(0), None, None, None, None, None, None, None) == capi.OK
    assert lib.earhip_screen_apply_device(None, None, C.byref(rep), C.c_size_t(0), None, None, None, None, None, None, None,
                                          None) == capi.INVALID_ARGUMENT
    assert lib.earhip_screen_default(None) == capi.INVALID_ARGUMENT
    assert lib.earhip_screen_edges(None, None) == capi.INVALID_ARGUMENT


def test_in_place():
    rep = c_screen(M.POLAR_15)
    az, el, ref, lh, lv, _ = M.mixed_batch(300, seed=5)
    want = capi.screen_apply(az, el, rep, None, ref, lh, lv)
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    a, e = az.copy(), el.copy()
    rc = capi.load().earhip_screen_apply(None, C.byref(rep), C.c_size_t(300), a.ctypes.data_as(dp), e.ctypes.data_as(dp),
                                         ref.ctypes.data_as(bp), lh.ctypes.data_as(bp), lv.ctypes.data_as(bp),
                                         a.ctypes.data_as(dp), e.ctypes.data_as(dp))
    assert rc == capi.OK
    assert np.array_equal(bits(a), bits(want[0])) and np.array_equal(bits(e), bits(want[1]))


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    lib = capi.load()
    for name in ("earhip_screen_default", "earhip_screen_edges", "earhip_screen_apply", "earhip_screen_apply_device"):
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert hasattr(lib, name), name
    assert re.search(r"^typedef struct earhip_screen \{", header, flags=re.M)
    for name in ("screen_default", "screen_edges", "screen_apply", "screen_apply_device"):
        assert callable(getattr(capi, name))
    hpp = open(os.path.join(ROOT, "libear_amd", "host", "ear", "hip_screen.hpp")).read()
    assert "class ScreenHandler" in hpp


def test_segment_choice_at_every_breakpoint(tmp_path):
    """libear_amd/csrc/screen.h on the host, under ASan + UBSan: the segment chosen at and next to every breakpoint, the clamps
    at 180 and 90, the reduction of the azimuth (tests/cpp/test_screen_core.cpp)"""
    exe = tmp_path / "test_screen_core"
    src = os.path.join(ROOT, "tests", "cpp", "test_screen_core.cpp")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "libear_amd", "csrc"),
                    src, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0 and re.search(r"^\d+ checked, 0 failed$", res.stdout, flags=re.M), res.stdout
