"""The host form of include/earhip.h group V (screenRef scaling and screenEdgeLock of Cartesian positions), without a device:
bit for bit against the three host entry points it fuses, against the independent model of tests/screen_cart_cases.py, the
results that are exact, edges and locks seen through the conversion back to polar, every refusal, in place, the bindings, and
the shared core (libear_amd/csrc/screen_cart.h) as a program of its own."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import screen_cart_cases as K
import screen_model as M
from libear_amd import capi
from test_screen_cpu import bits, c_screen, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 257, 4099)
DP, BP = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)


def null_variants(ref, lh, lv):
    return ((ref, lh, lv), (None, lh, lv), (ref, None, lv), (ref, lh, None), (None, None, None))


def sweep():
    """every size, screen pair and NULL-array variant -> (x, y, z), (reference, reproduction), (ref, lh, lv)"""
    for n in SIZES:
        x, y, z, ref, lh, lv, _ = K.batch(n, seed=2000 + n)
        for pair in K.PAIRS:
            for flags in null_variants(ref, lh, lv):
                # with screen_ref NULL every element is scaled: the batch's untouched oddities would be refused
                yield (x, y, z) if flags[0] is not None else K.finite(x, y, z), pair, flags


def chain(pos, rs, ps, flags):
    """the three host entry points the stage fuses"""
    az, el, d = capi.to_polar(*pos)
    az, el = capi.screen_apply(az, el, ps, rs, *flags)
    return capi.to_cartesian(az, el, d)


def test_host_form_has_the_bits_of_the_chained_host_entry_points():
    calls = compared = 0
    for pos, (r, p), flags in sweep():
        rs, ps = c_screen(r), c_screen(p)
        got = capi.screen_apply_cartesian(*pos, ps, rs, *flags)
        f = K.flagged(pos[0].size, *flags)
        # (the chain converts the unflagged elements too, NaN among them, which its first stage refuses: leave them out)
        want = chain([a[f] for a in pos], rs, ps, [None if a is None else a[f] for a in flags])
        if p is None:  # no reproduction screen: the stage copies, where the chain still converts there and back
            want = [a[f] for a in pos]
        for g, w in zip(got, want):
            assert np.array_equal(bits(g[f]), bits(w)), (pos[0].size, np.flatnonzero(bits(g[f]) != bits(w))[:4])
        calls += 1
        compared += int(f.sum())
    assert calls == len(SIZES) * len(K.PAIRS) * 5 and compared > 50000


def test_host_form_matches_the_model():
    worst = 0.0
    for pos, (r, p), flags in sweep():
        got = capi.screen_apply_cartesian(*pos, c_screen(p), c_screen(r), *flags)
        want = K.model(*pos, p, r, *flags)
        for g, w in zip(got, want):
            assert np.array_equal(np.isnan(g), np.isnan(w))
            with np.errstate(invalid="ignore"):
                err = np.where(bits(g) == bits(w), 0.0, np.abs(g - w))
            worst = max(worst, float(np.nanmax(err)))
    print(f"host form vs model: worst difference {worst:.3e}")
    assert worst <= K.ATOL


def test_exact_results():
    x, y, z, ref, lh, lv, _ = K.batch(4099, seed=77)
    plain = ~K.flagged(4099, ref, lh, lv)
    held = np.concatenate([a[plain] for a in (x, y, z)])
    assert 1000 < plain.sum() < 1700 and np.isnan(held).any() and np.isinf(held).any()
    assert (bits(held) == bits([-0.0])[0]).any()
    for r, p in K.PAIRS:
        rs, ps = c_screen(r), c_screen(p)
        # unflagged elements keep their bits, whatever they hold
        got = capi.screen_apply_cartesian(x, y, z, ps, rs, ref, lh, lv)
        for g, a in zip(got, (x, y, z)):
            assert np.array_equal(bits(g[plain]), bits(a[plain]))
        # no reproduction screen: the whole batch keeps its bits, flags (and lock codes no screen would take) or not
        for flags in ((ref, lh, lv), (None, None, None), (None, np.full(4099, 3, np.uint8), lv)):
            got = capi.screen_apply_cartesian(x, y, z, None, rs, *flags)
            for g, a in zip(got, (x, y, z)):
                assert np.array_equal(bits(g), bits(a))
        # the flagged origin stays the origin under every combination of flags
        for combo in K.COMBOS:
            got = capi.screen_apply_cartesian([0.0, -0.0], [0.0, -0.0], [0.0, 0.0], ps, rs, *combo)
            assert all(g[0] == 0.0 and g[1] == 0.0 for g in got), (combo, got)
        # a flagged position on the z axis stays on it and keeps z: the poles map to themselves (|z| >= 1e-10: below that
        # the conversion calls it the origin)
        zs = np.array([1.0, -1.0, 0.3, -2.0, 1e-9, 1.7, -1e-10, 1.7e308])
        zero = np.zeros(zs.size)
        for h in (0, 1, 2):
            gx, gy, gz = capi.screen_apply_cartesian(zero, zero, zs, ps, rs, 1, h, 0)
            assert (gx == 0.0).all() and (gy == 0.0).all() and np.array_equal(bits(gz), bits(zs)), (h, gx, gy, gz)


def _angle_apart(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b)) % 360.0
    return np.minimum(d, 360.0 - d)


def test_reference_edges_land_on_reproduction_edges():
    for r, p in K.PAIRS[:3] + ((M.OTHERS[1], M.DEFAULT),):
        rs, ps = c_screen(r), c_screen(p)
        left, right, bottom, top = capi.screen_edges(rs if rs is not None else capi.screen_default())
        p_left, p_right, p_bottom, p_top = capi.screen_edges(ps)
        az, el, want_az, want_el = [left, right] * 2, [bottom, top] * 2, [p_left, p_right] * 2, [p_bottom, p_top] * 2
        d = np.array([0.7, 0.7, 1.3, 1.3])
        got = capi.screen_apply_cartesian(*capi.to_cartesian(az, el, d), ps, rs)
        g_az, g_el, g_d = capi.to_polar(*got)
        assert _angle_apart(g_az, want_az).max() <= 1e-6 and np.abs(g_el - want_el).max() <= 1e-6, (g_az, g_el)
        assert np.abs(g_d - d).max() <= 1e-6


def test_locks_alone_and_together_with_and_without_screen_ref():
    rng = np.random.default_rng(404)
    n = 60
    x, y, z = rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(-1.0, 1.0, n)
    x = np.where(np.maximum(np.abs(x), np.abs(y)) < 0.3, 1.1, x)  # well off the z axis, where the azimuth is lost
    for r, p in K.PAIRS[:3]:
        rs, ps = c_screen(r), c_screen(p)
        p_left, p_right, p_bottom, p_top = capi.screen_edges(ps)
        for ref in (0, 1):
            # the unlocked run: the scaled position, or (no flag at all) the input
            free_az, free_el, free_d = capi.to_polar(*capi.screen_apply_cartesian(x, y, z, ps, rs, ref, 0, 0))
            if ref == 0:
                assert np.array_equal(bits(free_az), bits(capi.to_polar(x, y, z)[0]))
            for h in (0, 1, 2):
                for v in (0, 1, 2):
                    if h == 0 and v == 0:
                        continue
                    az, el, d = capi.to_polar(*capi.screen_apply_cartesian(x, y, z, ps, rs, ref, h, v))
                    want_az = free_az if h == 0 else np.full(n, (p_left, p_right)[h - 1])
                    want_el = free_el if v == 0 else np.full(n, (p_bottom, p_top)[v - 1])
                    assert _angle_apart(az, want_az).max() <= 1e-6, (ref, h, v, _angle_apart(az, want_az).max())
                    assert np.abs(el - want_el).max() <= 1e-6, (ref, h, v, np.abs(el - want_el).max())
                    assert np.abs(d - free_d).max() <= 1e-6


def _raw(rep, x, y, z, ref, lh, lv, out, reference=None, n=None):
    def p(a, t=DP):
        return None if a is None else a.ctypes.data_as(t)
    return capi.load().earhip_screen_apply_cartesian(
        None if reference is None else C.byref(reference), None if rep is None else C.byref(rep),
        C.c_size_t(x.size if n is None else n), p(x), p(y), p(z), p(ref, BP), p(lh, BP), p(lv, BP), *[p(a) for a in out])


def test_refused_elements_are_named_and_the_elements_before_them_written():
    lib = capi.load()
    n = 1500
    x, y, z, ref, lh, lv, bad = K.batch(n, seed=99, invalid=True)
    assert bad.sum() >= 12
    rep = c_screen(M.SCREEN_30)
    ok = ~bad
    want = capi.screen_apply_cartesian(x[ok], y[ok], z[ok], rep, None, ref[ok], lh[ok], lv[ok])
    for i in np.flatnonzero(bad):
        # the accepted elements before it, it, and the 40 elements after it
        idx = np.concatenate([np.flatnonzero(ok[:i]), np.arange(i, min(i + 41, n))])
        k = int(ok[:i].sum())
        args = [np.ascontiguousarray(a[idx]) for a in (x, y, z, ref, lh, lv)]
        refused(lambda: capi.screen_apply_cartesian(*args[:3], rep, None, *args[3:]), f"element {k}:")
        out = [np.full(idx.size, -1000.0 - j) for j in range(3)]
        assert _raw(rep, *args, out) == capi.INVALID_ARGUMENT and f"element {k}:".encode() in lib.earhip_last_error()
        for j in range(3):
            assert np.array_equal(bits(out[j][:k]), bits(want[j][:k])) and (out[j][k:] == -1000.0 - j).all()
    # the same values in an element with no flag set are nobody's business; neither is anything without a reproduction screen
    got = capi.screen_apply_cartesian([0.5, np.inf, 0.5], [0.5, np.nan, 0.5], [0.1, -np.inf, 0.1], rep, None, [1, 0, 1])
    assert got[0][1] == np.inf and np.isnan(got[1][1]) and got[2][1] == -np.inf and got[0][0] == got[0][2]
    capi.screen_apply_cartesian([np.nan], [0.0], [0.0], None, None, 1, 3, 3)
    # the largest coordinates are finite, and so is what becomes of them
    assert all(np.isfinite(g).all() for g in capi.screen_apply_cartesian([1.7e308, -1e308], [-1.7e308, 1e308], [1e308, 1.7e308], rep))
    # NULL arrays, too many elements; n == 0 needs no arrays
    one = np.zeros(1)
    for missing in range(6):
        arrays = [None if j == missing else one for j in range(6)]
        assert _raw(rep, *arrays[:3], None, None, None, arrays[3:], n=1) == capi.INVALID_ARGUMENT
    assert _raw(rep, one, one, one, None, None, None, [one] * 3, n=1 << 31) == capi.INVALID_ARGUMENT
    assert _raw(rep, None, None, None, None, None, None, [None] * 3, n=0) == capi.OK
    assert lib.earhip_screen_apply_cartesian_device(None, None, C.byref(rep), C.c_size_t(0), *[None] * 10) == capi.INVALID_ARGUMENT


def test_refused_screens_give_the_messages_of_the_polar_stage():
    P = capi.Screen.polar
    bad = ((P(1.78, 170.0, 0.0, 1.0, 58.0), "edges"), (P(0.0, 0.0, 0.0, 1.0, 58.0), "aspect_ratio"),
           (P(1.78, 0.0, 0.0, 1.0, 180.0), "width_azimuth"), (P(1.78, 0.0, 0.0, 0.0, 58.0), "distance"),
           (P(1.78, 0.0, 91.0, 1.0, 58.0), "elevation"), (P(1.78, float("nan"), 0.0, 1.0, 58.0), "azimuth"),
           (capi.Screen.cart(1.78, 0.0, 1.0, 0.0, 0.0), "width_x"), (capi.Screen.cart(1.78, 0.0, float("nan"), 0.0, 1.0), "y"),
           (capi.Screen.cart(1.78, -1.0, -0.2, 0.0, 1.0), "edges"))
    good = c_screen(M.SCREEN_30)

    def message(fn):
        with pytest.raises(capi.InvalidArgument) as e:
            fn()
        return str(e.value)
    for s, field in bad:
        for rep, reference, role in ((s, None, "reproduction"), (good, s, "reference"), (None, s, "reference")):
            text = message(lambda: capi.screen_apply_cartesian([0.0], [1.0], [0.0], rep, reference))
            assert role in text and field in text
            assert text == message(lambda: capi.screen_apply([0.0], [0.0], rep, reference))
            # before any element is looked at, and with no element at all
            assert text == message(lambda: capi.screen_apply_cartesian(np.zeros(0), np.zeros(0), np.zeros(0), rep, reference))


def test_in_place():
    x, y, z, ref, lh, lv, _ = K.batch(300, seed=5)
    for r, p in K.PAIRS:
        rs, ps = c_screen(r), c_screen(p)
        want = capi.screen_apply_cartesian(x, y, z, ps, rs, ref, lh, lv)
        io = [x.copy(), y.copy(), z.copy()]
        assert _raw(ps, *io, ref, lh, lv, io, reference=rs) == capi.OK
        for g, w in zip(io, want):
            assert np.array_equal(bits(g), bits(w))


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    exports = open(os.path.join(ROOT, "libear_amd", "csrc", "exports.map")).read()
    lib = capi.load()
    assert re.search(r"global:\s*earhip_\*;", exports)  # every earhip_ symbol is exported, no other
    for name in ("earhip_screen_apply_cartesian", "earhip_screen_apply_cartesian_device"):
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert hasattr(lib, name), name
    for name in ("screen_apply_cartesian", "screen_apply_cartesian_device"):
        assert callable(getattr(capi, name))
    hpp = open(os.path.join(ROOT, "libear_amd", "host", "ear", "hip_screen.hpp")).read()
    assert len(re.findall(r"\bapply_cartesian\(", hpp)) >= 2


def test_core_on_the_fixed_points(tmp_path):
    """libear_amd/csrc/screen_cart.h on the host, as a program of its own (tests/cpp/test_screen_cart_core.cpp): apply_cart_one
    on the fixed points, the pass-through of an unflagged NaN, the refusal codes"""
    exe = tmp_path / "test_screen_cart_core"
    src = os.path.join(ROOT, "tests", "cpp", "test_screen_cart_core.cpp")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "libear_amd", "csrc"), src, "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0 and re.search(r"^\d+ checked, 0 failed$", res.stdout, flags=re.M), res.stdout
