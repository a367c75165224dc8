"""The host tables behind channelLock and zoneExclusion of the Objects gain producer (libearhip group I:
earhip_objects_lock_priority, earhip_objects_excluded_channels, earhip_objects_zone_downmix) against tests/objects_model.py
and the literal answers of the header's specification, and the value checks of the host form.  No device is needed."""
import numpy as np
import pytest

import objects_model as om
from layouts import LAYOUTS


def names_mask(layout, pred):
    return sum(1 << i for i, nm in enumerate(LAYOUTS[layout]) if not nm.startswith("LFE") and pred(nm))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_lock_priority_equals_the_model(layout):
    from libear_amd import capi
    got = capi.objects_lock_priority(layout)
    assert got == om.lock_priority(layout)
    assert sorted(got) == [i for i, nm in enumerate(LAYOUTS[layout]) if not nm.startswith("LFE")]


def test_lock_priority_literal_orders():
    from libear_amd import capi
    want = {"0+5+0": "M+000 M-030 M+030 M-110 M+110",
            "9+10+3": "M+000 M-030 M+030 M-060 M+060 M-090 M+090 M-135 M+135 M+180 B+000 B-045 B+045 U+000 U-045 U+045 "
                      "U-090 U+090 U-135 U+135 U+180 T+000"}
    for layout, order in want.items():
        assert [LAYOUTS[layout][i] for i in capi.objects_lock_priority(layout)] == order.split()


def masks_of(layout):
    """the empty and the full set, every single loudspeaker, each layer, everything behind, 50 random masks"""
    from libear_amd import capi
    chans = capi.layout_channels(layout)
    real = [i for i, c in enumerate(chans) if not c[3]]
    out = [0, sum(1 << i for i in real)] + [1 << i for i in real]
    for lo, hi in ((-91, -10), (-10, 10), (10, 60), (60, 91)):
        out.append(sum(1 << i for i in real if lo <= chans[i][2] < hi))
    out.append(sum(1 << i for i in real if abs(chans[i][1]) > 90.0))
    rng = np.random.default_rng(sum(map(ord, layout)))
    out += [int(m) for m in rng.integers(0, 1 << len(chans), 50)]
    return out


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_zone_downmix_equals_the_model(layout):
    from libear_amd import capi
    n = len(LAYOUTS[layout])
    masks = masks_of(layout)
    assert np.array_equal(capi.objects_zone_downmix(layout, masks[0]), np.eye(n))
    assert np.array_equal(capi.objects_zone_downmix(layout, masks[1]), np.eye(n))
    for mask in masks:
        got = capi.objects_zone_downmix(layout, mask)
        assert np.max(np.abs(got - om.zone_downmix(layout, mask))) <= 1e-15, mask
        assert np.max(np.abs(got.sum(axis=1) - 1.0)) <= 1e-15, mask
        full = all(mask >> i & 1 for i, nm in enumerate(LAYOUTS[layout]) if not nm.startswith("LFE"))
        for i, nm in enumerate(LAYOUTS[layout]):
            if nm.startswith("LFE"):
                assert got[i, i] == 1.0 and got[i].sum() == 1.0 and got[:, i].sum() == 1.0
            elif mask >> i & 1 and not full:
                assert not got[:, i].any()


def test_zone_groups_of_9_10_3_literal():
    """the groups of a loudspeaker read off a chain of exclusions: exclude it, see where its row goes, exclude that too, ..."""
    from libear_amd import capi
    layout = "9+10+3"
    names = LAYOUTS[layout]

    def chain(name, n):
        mask, groups = 1 << names.index(name), [{name}]
        for _ in range(n):
            row = capi.objects_zone_downmix(layout, mask)[names.index(name)]
            to = {names[j] for j in np.nonzero(row)[0]}
            assert np.allclose(row[row > 0], 1.0 / len(to), rtol=0, atol=1e-15)
            groups.append(to)
            mask |= sum(1 << names.index(t) for t in to)
        return groups
    assert chain("M+000", 5) == [{"M+000"}, {"M+030", "M-030"}, {"M+060", "M-060"}, {"M+090", "M-090"}, {"M+135", "M-135"},
                                 {"M+180"}]
    assert chain("T+000", 4) == [{"T+000"}, {"U+090", "U-090"}, {"U+045", "U-045", "U+135", "U-135"}, {"U+000", "U+180"},
                                 {"M+090", "M-090"}]
    assert chain("U+045", 3) == [{"U+045"}, {"U+000"}, {"U-045"}, {"U+090"}]


def test_excluded_channels():
    from libear_amd import capi
    layout = "9+10+3"
    names = LAYOUTS[layout]
    every = names_mask(layout, lambda nm: True)

    def both(zones):
        keys = {"min_azimuth": "minAzimuth", "max_azimuth": "maxAzimuth", "min_elevation": "minElevation",
                "max_elevation": "maxElevation", "min_x": "minX", "max_x": "maxX", "min_y": "minY", "max_y": "maxY",
                "min_z": "minZ", "max_z": "maxZ"}
        got = capi.objects_excluded_channels(layout, zones)
        assert got == om.excluded_channels(layout, [{keys[k]: v for k, v in z.items()} for z in zones])
        return {names[i] for i in range(len(names)) if got >> i & 1}
    band = dict(min_elevation=-90.0, max_elevation=90.0)
    # the full circle
    assert both([dict(min_azimuth=-180.0, max_azimuth=180.0, **band)]) == {names[i] for i in range(len(names)) if every >> i & 1}
    # through +-180 (edges on M+135's far side and short of M-135); the pole is in whatever the azimuths are
    assert both([dict(min_azimuth=150.0, max_azimuth=-150.0, **band)]) == {"M+180", "U+180", "T+000"}
    assert both([dict(min_azimuth=150.0, max_azimuth=-150.0, min_elevation=-10.0, max_elevation=10.0)]) == {"M+180"}
    # one azimuth exactly on a loudspeaker (and the degenerate range is not the full circle)
    assert both([dict(min_azimuth=60.0, max_azimuth=60.0, min_elevation=-5.0, max_elevation=5.0)]) == {"M+060"}
    assert both([dict(min_azimuth=-135.0, max_azimuth=-135.0, min_elevation=0.0, max_elevation=30.0)]) == {"M-135", "U-135"}
    # an elevation band that holds the top loudspeaker, whatever its azimuth bounds
    assert both([dict(min_azimuth=100.0, max_azimuth=101.0, min_elevation=80.0, max_elevation=90.0)]) == {"T+000"}
    # a Cartesian box: everything behind
    box = dict(min_x=-1.0, max_x=1.0, min_y=-1.0, max_y=-1e-3, min_z=-1.0, max_z=1.0)
    assert both([box]) == {"M+135", "M-135", "M+180", "U+135", "U-135", "U+180"}
    # a union of two
    assert both([box, dict(min_azimuth=-1.0, max_azimuth=1.0, min_elevation=-35.0, max_elevation=-25.0)]) == \
        {"M+135", "M-135", "M+180", "U+135", "U-135", "U+180", "B+000"}
    assert both([]) == set()
    # other layouts against the model
    for other in sorted(LAYOUTS):
        zones = [dict(min_azimuth=100.0, max_azimuth=-100.0, min_elevation=-90.0, max_elevation=90.0)]
        want = om.excluded_channels(other, [dict(minAzimuth=100.0, maxAzimuth=-100.0, minElevation=-90.0, maxElevation=90.0)])
        assert capi.objects_excluded_channels(other, zones) == want


def test_host_form_refuses_values_outside_their_ranges():
    """the values are looked at before anything else, so a NULL panner shows the messages without a device"""
    import ctypes as C
    from libear_amd import capi
    lib = capi.load()
    f64 = C.POINTER(C.c_double)

    def call(n=3, divergence=None, lock_max=None, az_range=None):
        def opt(v):
            return None if v is None else capi._ptr(np.ascontiguousarray(v, np.float64), f64)
        zeros = np.zeros(n)
        out = np.zeros((n, 24), np.float32)
        capi.check(lib.earhip_panner_calculate_objects(
            None, C.c_size_t(n), opt(zeros), opt(zeros), None, None, None, None, None, None, None, opt(lock_max), opt(divergence),
            opt(az_range), None, capi._ptr(out), capi._ptr(out)))
    for bad in (-0.1, 1.5, np.nan):
        with pytest.raises(capi.InvalidArgument, match=r"divergence\[1\] must be in \[0, 1\]"):
            call(divergence=[0.0, bad, 1.0])
    for bad in (-1e-9, np.nan):
        with pytest.raises(capi.InvalidArgument, match=r"lock_max_distance\[2\] must not be negative or NaN"):
            call(lock_max=[0.0, np.inf, bad])
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(capi.InvalidArgument, match=r"azimuth_range\[0\] must be finite"):
            call(az_range=[bad, 45.0, 0.0])
    # valid values get as far as the panner
    with pytest.raises(capi.InvalidArgument, match="panner must not be NULL"):
        call(divergence=[0.0, 0.5, 1.0], lock_max=[0.0, np.inf, 2.0], az_range=[0.0, 45.0, 90.0])
    with pytest.raises(capi.InvalidArgument, match=r"bit set beyond the layout's 6 channels"):
        capi.objects_zone_downmix("0+5+0", 1 << 6)
    with pytest.raises(capi.UnknownLayout):
        capi.objects_lock_priority("1+2+3")
