"""ear::GainCalculatorDirectSpeakers through the C ABI (earhip group I, DirectSpeakers; capi.DirectSpeakers).

The reference's own cases (tests/gain_calculator_direct_speakers_tests.cpp) restated with their expected gains.
The label, LFE, substitution, bounds, error and warning logic is host code: a calculator created without a context
runs it on any machine, as long as no channel reaches the point source panner.  The cases that do are marked gpu
and compared with the pinned oracle panner (oracle/panner_oracle.hpp) at 1e-6.

One documented difference from libear: the mapping rules of the common-definitions packs (AP_0001xxxx) are not
carried, and such a channel is refused (NotImplementedInLibear, naming the pack).
"""
import numpy as np
import pytest

import ds_model
from libear_amd import capi

URN0, URN1 = ds_model.URN0, "urn:itu:bs:2051:1:speaker:"


def names(layout, without_lfe=False):
    return [c[0] for c in capi.layout_channels(layout) if not (without_lfe and c[3])]


def direct_pv(layout, channel):
    pv = np.zeros(len(names(layout)), np.float32)
    pv[names(layout).index(channel)] = 1.0
    return pv


def calc(ds, md):
    g, w = ds.calculate([md])
    return g[0], [int(c) for c in w[0] if c]


def test_speaker_label():
    ds = capi.DirectSpeakers(None, "4+5+0")
    for prefix in ("", URN0, URN1):
        assert np.array_equal(calc(ds, {"speakerLabels": [prefix + "M+000"]})[0], direct_pv("4+5+0", "M+000"))
        assert np.array_equal(calc(ds, {"speakerLabels": [prefix + "M+030"]})[0], direct_pv("4+5+0", "M+030"))
        # missing channels are ignored
        assert np.array_equal(calc(ds, {"speakerLabels": [prefix + "M+030", prefix + "B+000"]})[0],
                              direct_pv("4+5+0", "M+030"))
        assert np.array_equal(calc(ds, {"speakerLabels": [prefix + "B+000", prefix + "M+030"]})[0],
                              direct_pv("4+5+0", "M+030"))
        # matching more than one channel picks the first
        assert np.array_equal(calc(ds, {"speakerLabels": [prefix + "M+000", prefix + "M+030"]})[0],
                              direct_pv("4+5+0", "M+000"))
        assert np.array_equal(calc(ds, {"speakerLabels": [prefix + "M+030", prefix + "M+000"]})[0],
                              direct_pv("4+5+0", "M+030"))
    ds.close()


def test_speaker_label_additional_substitutions():
    ds = capi.DirectSpeakers(None, "4+5+0", {"foo": "M+030"})
    assert np.array_equal(calc(ds, {"speakerLabels": ["foo"]})[0], direct_pv("4+5+0", "M+030"))
    ds.close()
    # a substitution is keyed by the label as written, and does not replace a default (std::map::insert)
    ds = capi.DirectSpeakers(None, "4+5+0", {"LFE": "M+000", URN0 + "bar": "M-030"})
    assert np.array_equal(calc(ds, {"speakerLabels": ["LFE"]})[0], direct_pv("4+5+0", "LFE1"))
    assert np.array_equal(calc(ds, {"speakerLabels": [URN0 + "bar"]})[0], direct_pv("4+5+0", "M-030"))
    assert np.array_equal(calc(ds, {"speakerLabels": ["LFER"]})[0], direct_pv("4+5+0", "LFE1"))
    ds.close()


def test_one_lfe_out():
    ds = capi.DirectSpeakers(None, "4+5+0")
    assert np.array_equal(calc(ds, {"speakerLabels": ["LFE1"]})[0], direct_pv("4+5+0", "LFE1"))
    assert np.array_equal(calc(ds, {"speakerLabels": ["LFE2"]})[0], direct_pv("4+5+0", "LFE1"))
    ds.close()


def test_two_lfe_out():
    ds = capi.DirectSpeakers(None, "9+10+3")
    assert np.array_equal(calc(ds, {"speakerLabels": ["LFE1"]})[0], direct_pv("9+10+3", "LFE1"))
    assert np.array_equal(calc(ds, {"speakerLabels": ["LFER"]})[0], direct_pv("9+10+3", "LFE2"))
    ds.close()


def test_no_lfe_out():
    ds = capi.DirectSpeakers(None, "0+2+0")
    assert not calc(ds, {"speakerLabels": ["LFE1"]})[0].any()
    assert not calc(ds, {"speakerLabels": ["LFE2"]})[0].any()
    ds.close()


def test_lfe_just_frequency():
    ds = capi.DirectSpeakers(None, "4+5+0")
    assert np.array_equal(calc(ds, {"lowPass": 100.0})[0], direct_pv("4+5+0", "LFE1"))
    g, w = calc(ds, {"lowPass": 100.0, "speakerLabels": ["LFE1"]})
    assert np.array_equal(g, direct_pv("4+5+0", "LFE1")) and w == []
    ds.close()


def test_dist_bounds_polar_direct():
    """the assertions of test_dist_bounds_polar whose result is one loudspeaker (all of them: the gpu test below)"""
    ds = capi.DirectSpeakers(None, "9+10+3")
    pv = lambda ch: direct_pv("9+10+3", ch)  # noqa: E731
    assert np.array_equal(calc(ds, {"azimuth": 15.0, "azimuthMin": 0.0})[0], pv("M+000"))
    assert np.array_equal(calc(ds, {"azimuth": 15.0, "azimuthMax": 30.0})[0], pv("M+030"))
    assert np.array_equal(calc(ds, {"azimuth": 14.0, "azimuthMin": 0.0, "azimuthMax": 30.0})[0], pv("M+000"))
    assert np.array_equal(calc(ds, {"elevation": 15.0, "elevationMin": 0.0})[0], pv("M+000"))
    assert np.array_equal(calc(ds, {"elevation": 15.0, "elevationMax": 30.0})[0], pv("U+000"))
    assert np.array_equal(calc(ds, {"elevation": 14.0, "elevationMin": 0.0, "elevationMax": 30.0})[0], pv("M+000"))
    # pole loudspeakers are found even when the azimuth range excludes 0
    assert np.array_equal(calc(ds, {"azimuth": 15.0, "elevation": 90.0, "azimuthMin": 10.0, "azimuthMax": 20.0})[0],
                          pv("T+000"))
    # distance bounds: the loudspeakers stand at distance 1
    assert np.array_equal(calc(ds, {"distance": 0.5, "distanceMax": 1.0})[0], pv("M+000"))
    # without a context, a channel that needs the panner is refused rather than left silent
    with pytest.raises(capi.InvalidArgument):
        ds.calculate([{"azimuth": 15.0}])
    ds.close()


@pytest.mark.gpu
def test_dist_bounds_polar():
    """every assertion of the reference's test_dist_bounds_polar; the point-source-panner results against the
    oracle panner and the closed form (half way between two loudspeakers: sqrt(0.5) on each)"""
    from _hip import ctx
    layout = "9+10+3"
    ds = capi.DirectSpeakers(ctx(), layout)
    psp = ds_model.oracle_psp(layout)
    pv = lambda ch: direct_pv(layout, ch)  # noqa: E731
    n = names(layout)
    horiz = np.zeros(len(n))
    horiz[[n.index("M+000"), n.index("M+030")]] = np.sqrt(0.5)
    vert = np.zeros(len(n))
    vert[[n.index("M+000"), n.index("U+000")]] = np.sqrt(0.5)

    def check_psp(md, closed):
        g = calc(ds, md)[0]
        want = psp(np.array([md.get("azimuth", 0.0)]), np.array([md.get("elevation", 0.0)]))[0]
        assert np.max(np.abs(g - want)) <= 1e-6
        assert np.max(np.abs(g - closed)) <= 1e-6
    check_psp({"azimuth": 15.0}, horiz)
    assert np.array_equal(calc(ds, {"azimuth": 15.0, "azimuthMin": 0.0})[0], pv("M+000"))
    assert np.array_equal(calc(ds, {"azimuth": 15.0, "azimuthMax": 30.0})[0], pv("M+030"))
    check_psp({"azimuth": 15.0, "azimuthMin": 0.0, "azimuthMax": 30.0}, horiz)
    assert np.array_equal(calc(ds, {"azimuth": 14.0, "azimuthMin": 0.0, "azimuthMax": 30.0})[0], pv("M+000"))
    check_psp({"elevation": 15.0}, vert)
    assert np.array_equal(calc(ds, {"elevation": 15.0, "elevationMin": 0.0})[0], pv("M+000"))
    assert np.array_equal(calc(ds, {"elevation": 15.0, "elevationMax": 30.0})[0], pv("U+000"))
    check_psp({"elevation": 15.0, "elevationMin": 0.0, "elevationMax": 30.0}, vert)
    assert np.array_equal(calc(ds, {"elevation": 14.0, "elevationMin": 0.0, "elevationMax": 30.0})[0], pv("M+000"))
    assert np.array_equal(calc(ds, {"azimuth": 15.0, "elevation": 90.0, "azimuthMin": 10.0, "azimuthMax": 20.0})[0],
                          pv("T+000"))
    assert ds.missed() == 0
    ds.close()


def test_mapping_rules_are_refused():
    """the reference's `mapping` cases: a common-definitions pack is refused, the pack named"""
    ds = capi.DirectSpeakers(None, "4+5+0")
    for pos, label in (((135.0, 0.0), "M+135"), ((180.0, 30.0), "U+180")):
        md = {"audioPackFormatID": "AP_0001000f", "azimuth": pos[0], "elevation": pos[1],
              "speakerLabels": [URN0 + label]}
        with pytest.raises(capi.NotImplementedInLibear, match="AP_0001000f"):
            ds.calculate([md])
    ds.close()


def test_mapping_per_input_is_refused():
    """the reference's `mapping_per_input` cases: refused even where a label would match"""
    ds = capi.DirectSpeakers(None, "4+5+0")
    for pack in ("AP_00010009", "AP_00010017"):
        md = {"audioPackFormatID": pack, "azimuth": 90.0, "speakerLabels": [URN0 + "M+090"]}
        with pytest.raises(capi.NotImplementedInLibear, match=pack):
            ds.calculate([md])
        with pytest.raises(capi.NotImplementedInLibear, match=pack):
            ds.calculate([{"audioPackFormatID": pack, "speakerLabels": [URN0 + "M+030"]}])
    ds.close()


def test_other_packs_follow_the_labels():
    """a pack ID outside the common definitions (AP_00020001, a custom pack) falls through to label matching"""
    ds = capi.DirectSpeakers(None, "4+5+0")
    for pack in ("AP_00020001", "AP_00011001x", "AP_0001000"):
        g, w = calc(ds, {"audioPackFormatID": pack, "speakerLabels": [URN0 + "M-110"]})
        assert np.array_equal(g, direct_pv("4+5+0", "M-110")) and w == []
    ds.close()


@pytest.mark.parametrize("case", ["screenEdgeLock horizontal", "screenEdgeLock vertical", "cartesian positions"])
def test_not_implemented(case):
    ds = capi.DirectSpeakers(None, "4+7+0")
    md = {"screenEdgeLock horizontal": {"screenEdgeLock": {"horizontal": "left"}},
          "screenEdgeLock vertical": {"screenEdgeLock": {"vertical": "top"}},
          "cartesian positions": {"cartesian": True}}[case]
    with pytest.raises(capi.NotImplementedInLibear):
        ds.calculate([md])
    ds.close()


def test_adm_errors():
    ds = capi.DirectSpeakers(None, "4+7+0")
    with pytest.raises(capi.AdmError):
        ds.calculate([{"audioPackFormatID": "AP_00010002"}])
    # before the refusal of a Cartesian position, as in libear
    with pytest.raises(capi.AdmError):
        ds.calculate([{"audioPackFormatID": "AP_00010002", "cartesian": True}])
    ds.close()


def test_warnings():
    """exact codes, once each; libear raises them before its own refusals"""
    ds = capi.DirectSpeakers(None, "4+7+0")
    g, w = calc(ds, {"lowPass": 300.0, "speakerLabels": ["M+000"]})
    assert w == [capi.FREQ_NOT_LFE] and np.array_equal(g, direct_pv("4+7+0", "M+000"))
    assert calc(ds, {"highPass": 20.0, "speakerLabels": ["M+000"]})[1] == [capi.FREQ_NOT_LFE]
    assert calc(ds, {"lowPass": 100.0, "highPass": 20.0, "speakerLabels": ["M+000"]})[1] == [capi.FREQ_NOT_LFE]
    g, w = calc(ds, {"lowPass": 100.0, "speakerLabels": ["M+000"]})
    assert w == [capi.FREQ_SPEAKERLABEL_LFE_MISMATCH] and np.array_equal(g, direct_pv("4+7+0", "LFE1"))
    assert calc(ds, {"speakerLabels": ["LFE1"]})[1] == [capi.FREQ_SPEAKERLABEL_LFE_MISMATCH]
    # both: the frequency is not an LFE's, the label is
    assert calc(ds, {"lowPass": 300.0, "speakerLabels": ["LFE"]})[1] == [capi.FREQ_NOT_LFE,
                                                                          capi.FREQ_SPEAKERLABEL_LFE_MISMATCH]
    # no labels: no mismatch to report
    assert calc(ds, {"lowPass": 300.0, "azimuth": 30.0})[1] == [capi.FREQ_NOT_LFE]
    assert calc(ds, {"lowPass": 200.0, "speakerLabels": ["LFE1"]})[1] == []
    # raised before a refusal, and returned with it
    with pytest.raises(capi.NotImplementedInLibear):
        ds.calculate([{"lowPass": 300.0, "speakerLabels": ["M+000"], "audioPackFormatID": "AP_00010003"}])
    assert list(ds.last_warnings[0]) == [capi.FREQ_NOT_LFE, 0]
    ds.close()


def test_batch_errors_name_the_channel():
    ds = capi.DirectSpeakers(None, "4+5+0")
    with pytest.raises(capi.NotImplementedInLibear, match=r"metadata\[2\]"):
        ds.calculate([{"speakerLabels": ["M+000"]}, {"speakerLabels": ["LFE1"]}, {"cartesian": True}])
    assert list(ds.last_warnings[1]) == [capi.FREQ_SPEAKERLABEL_LFE_MISMATCH, 0]
    g, w = ds.calculate([])
    assert g.shape == (0, 10) and w.shape == (0, 2)
    ds.close()


def test_create_errors():
    with pytest.raises(capi.UnknownLayout):
        capi.DirectSpeakers(None, "5+5+5")
    with pytest.raises(capi.InvalidArgument):
        capi.DirectSpeakers(None, "4+5+0", positions=(np.zeros(3), np.zeros(3)))


@pytest.mark.parametrize("layout", ["0+5+0", "4+5+0", "9+10+3", "3+7+0", "4+9+0"])
def test_host_logic_matches_the_numpy_restatement(layout):
    """random channels that stop before the panner: the library and ds_model agree on every gain and warning"""
    subst = {"foo": "M+030"}
    ds = capi.DirectSpeakers(None, layout, subst)
    model = ds_model.Model(capi.layout_channels(layout), subst)
    mds = [md for md in ds_model.random_metadata(capi.layout_channels(layout), 3000, 3) if model.one(md)[0] is not None]
    assert len(mds) > 1000
    got, gw = ds.calculate(mds)
    want, ww = model.calculate(mds, psp=None)
    assert np.array_equal(got, want) and np.array_equal(gw, ww)
    ds.close()
