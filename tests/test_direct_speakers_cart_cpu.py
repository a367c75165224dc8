"""DirectSpeakers with Cartesian positions and screenEdgeLock (earhip group X; capi.DirectSpeakers.calculate_screen), the host
logic: calculators created without a context, so every channel that stops before the point source panner is computed on any
machine, against tests/ds_cart_model.py (a numpy restatement of the group's header comment).  Rows the model places are
one-hot or silent, so they are compared exactly.  The panned channels are in tests/test_gpu_direct_speakers_cart.py.
"""
import ctypes as C

import numpy as np
import pytest

import conv_model
import ds_cart_model
import ds_model
import screen_model
from ds_cart_model import SCREEN, atmos_bed, c_screen
from libear_amd import capi

CUSTOM = [("Left", 35.0, 0.0), ("Right", -35.0, 0.0), ("Mid", 0.0, 0.0), ("Sub", 20.0, -25.0, True), ("BackL", 125.0, 0.0),
          ("BackR", -125.0, 0.0)]


def names(layout):
    return [c[0] for c in capi.layout_channels(layout)]


def one_hot(layout, channel):
    pv = np.zeros(len(names(layout)), np.float32)
    pv[names(layout).index(channel)] = 1.0
    return pv


def placed(model, mds):
    """the channels the model places without the panner"""
    return [md for md in mds if model.one_screen(md)[0] is not None]


def moved(layout, seed):
    return ds_cart_model.moved(capi.layout_channels(layout), seed)


@pytest.mark.parametrize("layout", capi.layout_names() + ["custom"])
def test_cartesian_positions(layout):
    if layout == "custom":
        layout = "ds cart six"
        capi.define_layout(layout, CUSTOM)
    ch = capi.layout_channels(layout)
    az, el = np.array([c[1] for c in ch]), np.array([c[2] for c in ch])
    real = moved(layout, 5)
    for positions in (None, real):
        ds = capi.DirectSpeakers(None, layout, positions=positions)
        nominal, r = ds.cartesian_positions()
        ds.close()
        (x, y, z), st = conv_model.point_polar_to_cart(az, el, 1.0)
        assert not st.any() and np.max(np.abs(nominal - np.stack([x, y, z], -1))) <= 1e-12
        (x, y, z), st = conv_model.point_polar_to_cart(*(positions or (az, el)), 1.0)
        assert not st.any() and np.max(np.abs(r - np.stack([x, y, z], -1))) <= 1e-12


def test_corners_of_0_5_0():
    ds = capi.DirectSpeakers(None, "0+5+0")
    nominal, _ = ds.cartesian_positions()
    ds.close()
    n = names("0+5+0")
    for name, want in (("M+030", (-1, 1, 0)), ("M-030", (1, 1, 0)), ("M+110", (-1, -1, 0)), ("M-110", (1, -1, 0)),
                       ("M+000", (0, 1, 0))):
        assert np.max(np.abs(nominal[n.index(name)] - np.array(want, float))) <= 1e-12, name


def test_atmos_bed_on_0_5_0():
    layout = "0+5+0"
    ds = capi.DirectSpeakers(None, layout)
    model = ds_cart_model.Model(capi.layout_channels(layout))
    mds = atmos_bed()
    want = {"RC_L": "M+030", "RC_R": "M-030", "RC_C": "M+000", "RC_Lrs": "M+110", "RC_Rrs": "M-110", "RC_LFE": "LFE1"}
    for md in mds:
        label = md["speakerLabels"][0]
        g, w, _ = model.one_screen(md)
        if label in want:
            got, gw = ds.calculate_screen([md])
            assert np.array_equal(got[0], one_hot(layout, want[label])), label
            assert np.array_equal(g, got[0])
            # (RC_LFE is no LFE label, so the frequency and the label disagree, as libear would report it)
            assert [int(c) for c in gw[0] if c] == w == ([capi.FREQ_SPEAKERLABEL_LFE_MISMATCH] if label == "RC_LFE" else [])
        else:
            assert g is None, label
            with pytest.raises(capi.InvalidArgument, match="point source panner"):
                ds.calculate_screen([md])
    assert sum(model.one_screen(md)[0] is None for md in mds) == 4
    ds.close()


@pytest.mark.parametrize("layout,move", [("0+5+0", False), ("4+7+0", False), ("9+10+3", False), ("9+10+3", True)])
def test_random_batches_match_the_model(layout, move):
    real = moved(layout, 11) if move else None
    subst = {"foo": "M+030"}
    ds = capi.DirectSpeakers(None, layout, subst, positions=real)
    model = ds_cart_model.Model(capi.layout_channels(layout), subst, real)
    mds = placed(model, ds_cart_model.random_metadata(model, 1536, 23))[:512]
    assert len(mds) == 512 and sum("X" in md for md in mds) > 200
    got, gw = ds.calculate_screen(mds)
    want, ww, rows = model.calculate_screen(mds, None)
    assert not rows
    assert np.array_equal(got, want) and np.array_equal(gw, ww)
    # one-hot rows from the bounds test are among them, not only labels and LFE
    assert sum(1 for md, g in zip(mds, got) if "X" in md and not md.get("speakerLabels") and g.any()) > 50
    ds.close()


def test_bounds_one_candidate_and_tolerance_edges():
    layout = "0+5+0"
    ds = capi.DirectSpeakers(None, layout)
    model = ds_cart_model.Model(capi.layout_channels(layout))

    def calc(md):
        g, _, _ = model.one_screen(md)
        got = ds.calculate_screen([md])[0][0]
        assert g is not None and np.array_equal(got, g)
        return got
    # a position off every loudspeaker, bounds that reach exactly one
    assert np.array_equal(calc({"X": -0.8, "Y": 0.9, "Z": 0.0, "XMin": -1.0, "YMax": 1.0}), one_hot(layout, "M+030"))
    # M+000 at (0, 1, 0): 1e-6 inside and 1e-6 outside each of the six tolerances
    base = {"X": 0.4, "Y": 0.6, "Z": 0.3, "XMin": -0.5, "XMax": 0.5, "YMin": 0.5, "YMax": 1.5, "ZMin": -0.5, "ZMax": 0.5}
    assert np.array_equal(calc(base), one_hot(layout, "M+000"))
    q = {"X": 0.0, "Y": 1.0, "Z": 0.0}
    for axis in "XYZ":
        for key, sign in ((axis + "Min", 1.0), (axis + "Max", -1.0)):
            inside = dict(base, **{key: q[axis] + sign * (1e-5 - 1e-6)})
            assert np.array_equal(calc(inside), one_hot(layout, "M+000")), key
            outside = dict(base, **{key: q[axis] + sign * (1e-5 + 1e-6)})
            assert model.one_screen(outside)[0] is None
            with pytest.raises(capi.InvalidArgument, match="point source panner"):
                ds.calculate_screen([outside])
    ds.close()


def test_bounds_several_candidates_nearest_and_tie():
    layout = "0+5+0"
    ds = capi.DirectSpeakers(None, layout)
    model = ds_cart_model.Model(capi.layout_channels(layout))
    # the two rear loudspeakers at (-+1, -1, 0) are the candidates; the position decides
    wide = {"Y": -1.0, "Z": 0.0, "XMin": -1.0, "XMax": 1.0}
    md = dict(wide, X=0.3)
    assert np.array_equal(ds.calculate_screen([md])[0][0], one_hot(layout, "M-110"))
    assert np.array_equal(model.one_screen(md)[0], one_hot(layout, "M-110"))
    md = dict(wide, X=-0.3)
    assert np.array_equal(ds.calculate_screen([md])[0][0], one_hot(layout, "M+110"))
    # the distances differ by 2 X: 1e-6 beyond the 1e-5 of the tie rule, and 1e-6 short of it
    clear = dict(wide, X=(1e-5 + 1e-6) / 2)
    assert np.array_equal(ds.calculate_screen([clear])[0][0], one_hot(layout, "M-110"))
    assert np.array_equal(model.one_screen(clear)[0], one_hot(layout, "M-110"))
    tie = dict(wide, X=(1e-5 - 1e-6) / 2)
    assert model.one_screen(tie)[0] is None
    with pytest.raises(capi.InvalidArgument, match="point source panner"):
        ds.calculate_screen([tie])
    ds.close()
    # moved loudspeakers: the bounds look at the nominal positions, the distances at the real ones
    ch = capi.layout_channels(layout)
    az, el = np.array([c[1] for c in ch]), np.array([c[2] for c in ch])
    az[names(layout).index("M+110")] = 60.0  # on the left wall now, farther from the position below than M-110
    ds = capi.DirectSpeakers(None, layout, positions=(az, el))
    model = ds_cart_model.Model(ch, None, (az, el))
    md = dict(wide, X=-0.3)
    assert np.array_equal(ds.calculate_screen([md])[0][0], one_hot(layout, "M-110"))
    assert np.array_equal(model.one_screen(md)[0], one_hot(layout, "M-110"))
    ds.close()


def test_bounds_respect_the_lfe_type():
    layout = "9+10+3"
    ds = capi.DirectSpeakers(None, layout)
    model = ds_cart_model.Model(capi.layout_channels(layout))
    nominal, _ = ds.cartesian_positions()
    n = names(layout)
    lfe2 = nominal[n.index("LFE2")]
    at = {"X": float(lfe2[0]), "Y": float(lfe2[1]), "Z": float(lfe2[2])}
    # an LFE channel on LFE2's position finds LFE2, not LFE1 (where step 6 would send it) ...
    g, w = ds.calculate_screen([dict(at, lowPass=100.0)])
    assert np.array_equal(g[0], one_hot(layout, "LFE2")) and not w.any()
    assert np.array_equal(model.one_screen(dict(at, lowPass=100.0))[0], g[0])
    # ... bounds around everything make it ambiguous only among the LFEs, and a far LFE falls through to LFE1
    box = {"XMin": -2.0, "XMax": 2.0, "YMin": -2.0, "YMax": 2.0, "ZMin": -2.0, "ZMax": 2.0}
    g, _ = ds.calculate_screen([dict(at, lowPass=100.0, **box)])
    assert np.array_equal(g[0], one_hot(layout, "LFE2"))
    g, _ = ds.calculate_screen([{"X": 0.0, "Y": -1.0, "Z": 1.0, "lowPass": 100.0}])
    assert np.array_equal(g[0], one_hot(layout, "LFE1"))
    # a full-range channel on the same position sees no LFE: B-045 stands there too
    assert np.array_equal(ds.calculate_screen([at])[0][0], one_hot(layout, "B-045"))
    assert np.array_equal(model.one_screen(at)[0], one_hot(layout, "B-045"))
    # and a layout without LFE1 is silent
    ds2 = capi.DirectSpeakers(None, "0+2+0")
    g, _ = ds2.calculate_screen([{"X": 0.0, "Y": 1.0, "Z": 0.0, "lowPass": 100.0}])
    assert not g.any()
    ds.close()
    ds2.close()


def _replace_polar(mds, screen):
    out = []
    for md in mds:
        h, v = ds_cart_model.lock_codes(md)
        az, el = capi.screen_apply([md.get("azimuth", 0.0)], [md.get("elevation", 0.0)], screen, None, [0], [h], [v])
        md = {k: val for k, val in md.items() if k != "screenEdgeLock"}
        out.append(dict(md, azimuth=float(az[0]), elevation=float(el[0])))
    return out


def _replace_cart(mds, screen):
    out = []
    for md in mds:
        h, v = ds_cart_model.lock_codes(md)
        x, y, z = capi.screen_apply_cartesian([md["X"]], [md.get("Y", 1.0)], [md.get("Z", 0.0)], screen, None, [0], [h], [v])
        md = {k: val for k, val in md.items() if k != "screenEdgeLock"}
        out.append(dict(md, X=float(x[0]), Y=float(y[0]), Z=float(z[0])))
    return out


def _locked_batch(layout, cartesian, n=1200):
    model = ds_cart_model.Model(capi.layout_channels(layout), None, None, SCREEN)
    mds = ds_cart_model.random_metadata(model, n, 41, cartesian=1.0 if cartesian else 0.0, lock=0.8)
    mds = [md for md in placed(model, mds) if ("X" in md) == cartesian]
    assert sum("screenEdgeLock" in md for md in mds) > 100
    return model, mds


@pytest.mark.parametrize("layout", ["0+5+0", "9+10+3"])
def test_lock_polar_is_the_screen_stage_then_no_lock(layout):
    model, mds = _locked_batch(layout, False)
    screen = c_screen(SCREEN)
    ds = capi.DirectSpeakers(None, layout)
    got, gw = ds.calculate_screen(mds, screen)
    plain, pw = ds.calculate_screen(_replace_polar(mds, screen), screen)
    assert np.array_equal(got, plain) and np.array_equal(gw, pw)
    want, ww, _ = model.calculate_screen(mds, None)
    assert np.array_equal(got, want) and np.array_equal(gw, ww)
    # the lock matters: without it other loudspeakers are found
    unlocked = [{k: v for k, v in md.items() if k != "screenEdgeLock"} for md in mds]
    other = ds_cart_model.Model(capi.layout_channels(layout)).calculate_screen(unlocked, None)[0]
    assert not np.array_equal(other, want)
    ds.close()


@pytest.mark.parametrize("layout", ["0+5+0", "9+10+3"])
def test_lock_cartesian_is_the_screen_stage_then_no_lock(layout):
    model, mds = _locked_batch(layout, True)
    screen = c_screen(SCREEN)
    ds = capi.DirectSpeakers(None, layout)
    got, gw = ds.calculate_screen(mds, screen)
    plain, pw = ds.calculate_screen(_replace_cart(mds, screen), screen)
    assert np.array_equal(got, plain) and np.array_equal(gw, pw)
    want, ww, _ = model.calculate_screen(mds, None)
    assert np.array_equal(got, want) and np.array_equal(gw, ww)
    ds.close()


def test_present_bounds_are_kept_and_absent_ones_follow_the_lock():
    layout = "0+5+0"
    screen = c_screen(SCREEN)
    left, right, bottom, top = capi.screen_edges(screen)
    assert 36.0 < left < 38.0 and -22.0 < right < -20.0
    ds = capi.DirectSpeakers(None, layout)
    # polar: M+030 is 7 degrees inside the left edge.  An absent azimuthMin follows the locked azimuth (37): not found;
    # a present azimuthMin of 25 stays 25 under the lock: found
    lock = {"screenEdgeLock": {"horizontal": "left"}}
    with pytest.raises(capi.InvalidArgument, match="point source panner"):
        ds.calculate_screen([dict(lock, azimuth=28.0)], screen)
    g, _ = ds.calculate_screen([dict(lock, azimuth=28.0, azimuthMin=25.0)], screen)
    assert np.array_equal(g[0], one_hot(layout, "M+030"))
    # ... and a present azimuthMax of 31 stays 31 although the position has moved beyond it: M+030 is still the one within
    g, _ = ds.calculate_screen([dict(lock, azimuth=28.0, azimuthMin=25.0, azimuthMax=31.0)], screen)
    assert np.array_equal(g[0], one_hot(layout, "M+030"))
    # Cartesian: locked to the right edge, the position lands between M+000 at (0, 1, 0) and M-030 at (1, 1, 0)
    lock = {"screenEdgeLock": {"horizontal": "right"}}
    x, y, z = capi.screen_apply_cartesian([0.1], [1.0], [0.0], screen, None, [0], [2], [0])
    assert 0.5 < x[0] < 0.9 and abs(y[0] - 1.0) < 1e-12 and abs(z[0]) < 1e-12
    cart = dict(lock, X=0.1, Y=1.0, Z=0.0)
    with pytest.raises(capi.InvalidArgument, match="point source panner"):
        ds.calculate_screen([cart], screen)                      # absent bounds: the locked point, no loudspeaker there
    g, _ = ds.calculate_screen([dict(cart, XMax=1.0)], screen)   # XMax kept, XMin absent = the locked x: M-030 alone
    assert np.array_equal(g[0], one_hot(layout, "M-030"))
    g, _ = ds.calculate_screen([dict(cart, XMin=-0.2, XMax=0.2)], screen)  # both kept, the locked x outside them: M+000
    assert np.array_equal(g[0], one_hot(layout, "M+000"))
    g, _ = ds.calculate_screen([dict(cart, XMin=-0.2)], screen)  # XMin kept, XMax follows the lock: M+000 again, not M-030
    assert np.array_equal(g[0], one_hot(layout, "M+000"))
    ds.close()


def test_a_lock_without_a_screen_changes_nothing():
    layout = "4+7+0"
    model, polar = _locked_batch(layout, False, 600)
    _, cart = _locked_batch(layout, True, 600)
    plain_model = ds_cart_model.Model(capi.layout_channels(layout))
    mds = [md for md in polar + cart if plain_model.one_screen(md)[0] is not None]
    assert len(mds) > 300 and sum("screenEdgeLock" in md for md in mds) > 100
    unlocked = [{k: v for k, v in md.items() if k != "screenEdgeLock"} for md in mds]
    ds = capi.DirectSpeakers(None, layout)
    got, gw = ds.calculate_screen(mds)
    want, ww = ds.calculate_screen(unlocked)
    assert np.array_equal(got, want) and np.array_equal(gw, ww)
    ds.close()


@pytest.mark.parametrize("layout", ["0+5+0", "4+5+0", "9+10+3"])
def test_no_cartesian_and_no_lock_is_the_old_entry_point(layout):
    subst = {"foo": "M+030"}
    ds = capi.DirectSpeakers(None, layout, subst)
    model = ds_model.Model(capi.layout_channels(layout), subst)
    mds = [md for md in ds_model.random_metadata(capi.layout_channels(layout), 1500, 3) if model.one(md)[0] is not None]
    assert len(mds) > 500
    want, ww = ds.calculate(mds)
    for screen in (None, c_screen(SCREEN)):
        got, gw = ds.calculate_screen(mds, screen)
        assert np.array_equal(got, want) and np.array_equal(gw, ww)
    ds.close()


def test_refusals_name_the_channel():
    layout = "4+5+0"
    ds = capi.DirectSpeakers(None, layout)
    screen = c_screen(SCREEN)
    ok = {"speakerLabels": ["M+000"]}
    nan, inf = float("nan"), float("inf")
    bad = [{"X": nan}, {"X": 0.0, "Y": inf}, {"X": 0.0, "Z": -inf}, {"X": 0.0, "XMin": nan}, {"X": 0.0, "ZMax": inf},
           {"X": 0.0, "YMin": -inf}, {"screenEdgeLock": {"horizontal": 3}}, {"X": 0.0, "screenEdgeLock": {"vertical": 3}},
           {"azimuth": 15.0}, {"X": 0.3, "Y": 0.3, "Z": 0.1}]
    for md in bad:
        for scr in (None, screen):
            with pytest.raises(capi.InvalidArgument, match=r"metadata\[2\]"):
                ds.calculate_screen([ok, {"speakerLabels": ["LFE1"]}, md, ok], scr)
            assert list(ds.last_warnings[1]) == [capi.FREQ_SPEAKERLABEL_LFE_MISMATCH, 0] and not ds.last_warnings[3].any()
            with pytest.raises(capi.InvalidArgument) as e:
                ds.calculate_screen([md], scr)
            assert "metadata[" not in str(e.value)
    # group R's checks of a polar position, under a lock and a screen only
    for md in ({"azimuth": nan}, {"elevation": 91.0}, {"azimuth": 2.0 ** 41}):
        locked = dict(md, screenEdgeLock={"vertical": "top"} if "azimuth" in md else {"horizontal": "left"})
        with pytest.raises(capi.InvalidArgument, match=r"metadata\[1\]"):
            ds.calculate_screen([ok, locked], screen)
    # an unknown lock string never reaches the library
    with pytest.raises(capi.InvalidArgument, match=r"metadata\[1\]"):
        ds.calculate_screen([ok, {"screenEdgeLock": {"horizontal": "top"}}], screen)
    # warnings raised before a refusal come back with it
    with pytest.raises(capi.InvalidArgument):
        ds.calculate_screen([{"X": nan, "lowPass": 300.0}])
    assert list(ds.last_warnings[0]) == [capi.FREQ_NOT_LFE, 0]
    # a Cartesian element without the cart array
    keep = []
    md = (capi.DSMetadata * 2)(ds._struct(ok, keep), ds._struct(ok, keep))
    md[1].cartesian = 1
    gains, warnings = np.zeros((2, ds.n_out), np.float32), np.zeros((2, 2), np.int32)
    rc = capi.load().earhip_direct_speakers_calculate_screen(ds.h, None, C.c_size_t(2), md, None,
                                                             gains.ctypes.data_as(C.POINTER(C.c_float)),
                                                             warnings.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == capi.INVALID_ARGUMENT and "metadata[1]" in capi.load().earhip_last_error().decode()
    # a reproduction screen group R refuses
    with pytest.raises(capi.InvalidArgument, match="screen"):
        ds.calculate_screen([ok], capi.Screen.polar(1.78, 170.0, 0.0, 1.0, 58.0))
    # the refusals of group I that stay
    for scr in (None, screen):
        with pytest.raises(capi.NotImplementedInLibear, match="AP_0001000f"):
            ds.calculate_screen([{"audioPackFormatID": "AP_0001000f", "speakerLabels": ["M+000"], "X": 0.0}], scr)
        with pytest.raises(capi.AdmError):
            ds.calculate_screen([{"audioPackFormatID": "AP_00010002", "X": 0.0}], scr)
    g, w = ds.calculate_screen([])
    assert g.shape == (0, 10) and w.shape == (0, 2)
    ds.close()


def test_a_loudspeaker_position_the_conversion_refuses():
    """a calculator created with a real azimuth beyond 2^40 (finite, so create takes it): group K's conversion returns a code
    for it, so every Cartesian element that reaches step 5a is refused, the message naming the element and the code, and so
    is cartesian_positions; labelled channels and polar channels without a lock are served as by calculate"""
    layout = "0+5+0"
    ch = capi.layout_channels(layout)
    az, el = np.array([c[1] for c in ch]), np.array([c[2] for c in ch])
    az[names(layout).index("M-110")] = 2.0 ** 41
    ds = capi.DirectSpeakers(None, layout, positions=(az, el))
    ok = {"speakerLabels": ["M+000"]}
    for scr in (None, c_screen(SCREEN)):
        with pytest.raises(capi.InvalidArgument, match=r"metadata\[1\]: .*Cartesian form.*returned code 1"):
            ds.calculate_screen([ok, {"X": 0.0}], scr)
        with pytest.raises(capi.InvalidArgument, match=r"^a loudspeaker position.*returned code 1"):
            ds.calculate_screen([{"X": -1.0, "Y": 1.0, "Z": 0.0, "lowPass": 100.0}], scr)
        # the element's own refusals come first
        with pytest.raises(capi.InvalidArgument, match="must be finite"):
            ds.calculate_screen([{"X": float("nan")}], scr)
    with pytest.raises(capi.InvalidArgument, match="returned code 1"):
        ds.cartesian_positions()
    # a label places a Cartesian channel before its position is looked at; polar channels never meet the table
    model = ds_model.Model(ch, None, (az, el))
    polar = [md for md in ds_model.random_metadata(ch, 600, 7) if model.one(md)[0] is not None]
    mds = polar + [{"speakerLabels": ["M+110"], "X": 0.0}, {"speakerLabels": ["LFE1"], "X": 0.5, "lowPass": 80.0}]
    got, gw = ds.calculate_screen(mds, c_screen(SCREEN))
    want, ww = ds.calculate(polar)
    assert len(polar) > 200 and np.array_equal(got[:len(polar)], want) and np.array_equal(gw[:len(polar)], ww)
    assert np.array_equal(got[-2], one_hot(layout, "M+110")) and np.array_equal(got[-1], one_hot(layout, "LFE1"))
    ds.close()


def test_positions_up_to_the_largest_double_convert_and_are_panned():
    """finite coordinates, however large or small, pass the finite check and group K's conversion gives them a finite
    direction (the library guards the launch against any other): they reach the panner like any position, here its refusal
    without a context; as an LFE they never reach the conversion"""
    ds = capi.DirectSpeakers(None, "0+5+0")
    ok = {"speakerLabels": ["M+000"]}
    big = float(np.finfo(np.float64).max)
    for x, y, z in ((1e308, 1e308, 0.0), (-big, big, big), (big, -big, -1e300), (-1.5e308, 1e308, 1e300), (5e-324, 0.0, 0.0)):
        pos = {"X": x, "Y": y, "Z": z}
        az, el, _ = capi.to_polar([x], [y], [z])[:3]
        assert np.isfinite(az).all() and np.isfinite(el).all()
        with pytest.raises(capi.InvalidArgument, match=r"metadata\[1\]: a channel needs the point source panner"):
            ds.calculate_screen([ok, pos])
        g, _ = ds.calculate_screen([dict(pos, lowPass=100.0)])
        assert np.array_equal(g[0], one_hot("0+5+0", "LFE1"))
    ds.close()


def test_the_old_entry_point_still_refuses():
    """beside tests/test_direct_speakers.py::test_not_implemented: calculate is libear's, refusals included"""
    ds = capi.DirectSpeakers(None, "4+7+0")
    for md in ({"cartesian": True}, {"screenEdgeLock": {"horizontal": "left"}}, {"screenEdgeLock": {"vertical": "top"}}):
        with pytest.raises(capi.NotImplementedInLibear):
            ds.calculate([md])
    # the keys of calculate_screen do not make calculate Cartesian
    g, _ = ds.calculate([{"X": 0.0, "Y": 1.0, "Z": 0.0, "speakerLabels": ["M+030"]}])
    assert g[0].any()
    ds.close()


def test_a_labelled_channel_never_has_its_position_looked_at():
    ds = capi.DirectSpeakers(None, "0+5+0")
    nan = float("nan")
    g, _ = ds.calculate_screen([{"speakerLabels": ["M+110"], "X": nan, "XMin": nan, "screenEdgeLock": {"horizontal": 7}}],
                               c_screen(SCREEN))
    assert np.array_equal(g[0], one_hot("0+5+0", "M+110"))
    ds.close()


def test_the_model_keeps_its_distance_from_every_decision():
    """what makes exact comparison sound: the generator refuses a case within 1e-9 of a decision, and sees one"""
    model = ds_cart_model.Model(capi.layout_channels("0+5+0"))
    model.margins = []
    model.one_screen({"X": 0.0, "Y": 1.0, "Z": 0.0, "XMax": -1e-5 + 1e-12})
    assert min(model.margins) < ds_cart_model.MARGIN
    model.margins = []
    model.one_screen({"X": 0.0, "Y": 1.0, "Z": 0.0, "XMax": -1e-5 + 1e-6})
    assert min(model.margins) >= 1e-7
    assert screen_model.edges(SCREEN)[0] > screen_model.edges(SCREEN)[1]
