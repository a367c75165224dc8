"""Loudspeaker layouts of the caller's own (include/earhip.h group H: earhip_layout_define / _kind / _hull) without a
device: the hull header on the CPU (tests/cpp/test_hull.cpp, also under ASan + UBSan), the registry through the C ABI,
the three layouts of tests/custom_layout_model.py against scipy's hull, and the model itself against the oracle's point
source panner on two BS.2051 layouts — which is what lets the GPU tests use it as the reference for defined layouts."""
import os
import subprocess

import numpy as np
import pytest

import _oracle
import custom_layout_model as model
from layouts import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libear_amd", "csrc")
TABLED = [name for name in sorted(LAYOUTS) if name != "0+2+0"]


def test_hull_header_on_cpu(tmp_path):
    """libear_amd/csrc/layout_registry.h: the hull of every tabled layout's nominal augmented set == its facet table"""
    exe = tmp_path / "test_hull"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_hull.cpp"),
                    "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0 and "all checks passed" in res.stdout, res.stdout


def test_hull_header_under_sanitizers(tmp_path):
    exe = tmp_path / "test_hull_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_hull.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0 and "all checks passed" in res.stdout, res.stdout


def define_all():
    from libear_amd import capi
    for name, (channels, *_) in model.CUSTOM.items():
        capi.define_layout(name, channels)


def test_define_kind_hull_round_trip():
    from libear_amd import capi
    assert capi.layout_kind("4+5+0") == 1 and capi.layout_kind("never defined") == 0
    channels = [("L", 30.0, 0.0), ("R", -30.0, 0.0, False), ("Sub", 0.0, -20.0, True), ("Ls", 110.0, 0.0, False, (100.0, 120.0), (0.0, 15.0)),
                ("Rs", -110.0, 0.0, False, (-120.0, -100.0), (0.0, 15.0))]
    capi.define_layout("round trip", channels)
    assert capi.layout_kind("round trip") == 2
    assert capi.layout_channels("round trip") == [("L", 30.0, 0.0, False), ("R", -30.0, 0.0, False), ("Sub", 0.0, -20.0, True),
                                                  ("Ls", 110.0, 0.0, False), ("Rs", -110.0, 0.0, False)]
    assert capi.layout_channel_ranges("round trip") == [((30.0, 30.0), (0.0, 0.0)), ((-30.0, -30.0), (0.0, 0.0)), ((0.0, 0.0), (-20.0, -20.0)),
                                                        ((100.0, 120.0), (0.0, 15.0)), ((-120.0, -100.0), (0.0, 15.0))]
    xyz, mix_to, n_virtual, facets = capi.layout_hull("round trip")
    # 4 loudspeakers, 4 below, 4 above, 2 virtual; the Sub (channel 2) is no vertex
    assert len(xyz) == 14 and n_virtual == 2 and list(mix_to) == [0, 1, 3, 4] * 3 + [-1, -1]
    assert np.allclose(xyz[:4], model.cart([30, -30, 110, -110], [0, 0, 0, 0]), atol=1e-15)
    assert np.array_equal(xyz[-2:], [[0, 0, -1], [0, 0, 1]])
    want_xyz, want_mix, _ = model.augment([c + (False,) if len(c) == 3 else c for c in channels])
    assert np.allclose(xyz, want_xyz, atol=1e-15) and [m if m < 0 else [0, 1, 3, 4][m] for m in want_mix] == list(mix_to)
    assert sorted(facets) == sorted(model.convex_hull(want_xyz))
    # the list of BS.2051 layouts is what it was
    assert capi.layout_names() == list(LAYOUTS)


def test_redefinition_and_refusals():
    from libear_amd import capi
    body = [("A", 0.0, 0.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0)]
    capi.define_layout("three", body)
    capi.define_layout("three", list(body))  # bit-identical: nothing happens
    assert capi.layout_kind("three") == 2
    for other in ([("A", 0.0, 0.0), ("B", 120.0, 0.0), ("C", -120.0, 1e-9)], body + [("D", 180.0, 0.0)],
                  [("A", 0.0, 0.0), ("B", 120.0, 0.0), ("c", -120.0, 0.0)], [("A", 0.0, 0.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0, True)],
                  [("A", 0.0, 0.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0, False, (-130.0, -110.0), (0.0, 0.0))]):
        with pytest.raises(capi.InvalidArgument, match="already defined"):
            capi.define_layout("three", other)
    assert capi.layout_channels("three") == [c + (False,) for c in body]
    refused = {
        "a BS.2051 name": ("4+5+0", body),
        "an empty name": ("", body),
        "a name of 64 characters": ("n" * 64, body),
        "no channel": ("r0", []),
        "duplicate channel names": ("r1", [("A", 0.0, 0.0), ("B", 120.0, 0.0), ("A", -120.0, 0.0)]),
        "an empty channel name": ("r2", [("", 0.0, 0.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0)]),
        "a channel name of 32 characters": ("r3", [("c" * 32, 0.0, 0.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0)]),
        "a NaN azimuth": ("r4", [("A", float("nan"), 0.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0)]),
        "an infinite elevation": ("r5", [("A", 0.0, float("inf")), ("B", 120.0, 0.0), ("C", -120.0, 0.0)]),
        "an elevation of 91": ("r6", [("A", 0.0, 91.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0)]),
        "an azimuth of 181": ("r7", [("A", 181.0, 0.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0)]),
        "33 channels": ("r8", [(f"S{k}", -170.0 + 10.0 * k, 0.0, k >= 20) for k in range(33)]),
        "only LFE channels": ("r9", [("LFE1", 45.0, -30.0, True)]),
        "a non-finite range": ("r10", [("A", 0.0, 0.0, False, (0.0, float("nan")), (0.0, 0.0)), ("B", 120.0, 0.0), ("C", -120.0, 0.0)]),
    }
    for what, (name, channels) in refused.items():
        with pytest.raises(capi.InvalidArgument):
            capi.define_layout(name, channels)
            pytest.fail(what + " was accepted")
        if name not in LAYOUTS:
            assert capi.layout_kind(name) == 0, what
    assert len(("n" * 63).encode()) == 63
    capi.define_layout("n" * 63, body)  # (63 characters and a channel name of 31 are allowed)
    capi.define_layout("names of 31", [("c" * 31, 0.0, 0.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0)])
    # two loudspeakers in one direction: three augmented vertices on a line
    with pytest.raises(capi.InvalidArgument, match="collinear"):
        capi.define_layout("twice", [("A", 0.0, 0.0), ("B", 120.0, 0.0), ("C", -120.0, 0.0), ("D", 120.0, 0.0)])
    assert capi.layout_kind("twice") == 0
    # more loudspeakers than the objects kernels' tables hold, and more around a virtual loudspeaker than an n-gon holds
    with pytest.raises(capi.NotImplementedInLibear):
        capi.define_layout("23 loudspeakers", [(f"S{k}", -170.0 + 15.0 * k, 0.0) for k in range(23)])
    with pytest.raises(capi.NotImplementedInLibear, match="around a virtual loudspeaker"):
        capi.define_layout("ring of 18", [(f"S{k}", -170.0 + 20.0 * k, 0.0) for k in range(18)])
    # a name that was never defined is unknown to every entry point that takes a name
    for call in (lambda: capi.layout_channels("7+7+7"), lambda: capi.layout_hull("7+7+7"), lambda: capi.objects_lock_priority("7+7+7"),
                 lambda: capi.design_decorrelators_for_layout("7+7+7"), lambda: capi.loudness_layout_weights("7+7+7"),
                 lambda: capi.DirectSpeakers(None, "7+7+7")):
        with pytest.raises(capi.UnknownLayout, match=r"unknown layout: 7\+7\+7"):
            call()


@pytest.mark.parametrize("name", TABLED)
def test_hull_of_a_bs2051_layout_is_its_table(name):
    """earhip_layout_hull of a BS.2051 layout returns the table; a copy defined under another name gets the same facets
    from the hull, as sets of sets"""
    from libear_amd import capi
    ranges = capi.layout_channel_ranges(name)
    capi.define_layout("copy:" + name, [c + r for c, r in zip(capi.layout_channels(name), ranges)])
    xyz, mix_to, n_virtual, facets = capi.layout_hull(name)
    cxyz, cmix_to, cn_virtual, cfacets = capi.layout_hull("copy:" + name)
    assert np.array_equal(xyz, cxyz) and np.array_equal(mix_to, cmix_to) and n_virtual == cn_virtual
    assert set(facets) == set(cfacets) and len(facets) == len(cfacets) == len(set(cfacets))
    assert capi.layout_channels("copy:" + name) == capi.layout_channels(name)
    assert capi.layout_channel_ranges("copy:" + name) == ranges


def test_stereo_has_no_hull_of_its_own():
    from libear_amd import capi
    with pytest.raises(capi.InvalidArgument):
        capi.layout_hull("0+2+0")


@pytest.mark.parametrize("name", sorted(model.CUSTOM))
def test_three_new_layouts(name):
    from scipy.spatial import ConvexHull
    from libear_amd import capi
    define_all()
    channels, n_facets, n_quads, n_triangles, rings, n_simplices = model.CUSTOM[name]
    n_real = sum(1 for c in channels if not c[3])
    xyz, mix_to, n_virtual, facets = capi.layout_hull(name)
    assert (n_real, len(xyz) - n_real - n_virtual, n_virtual) == {"2+7+0": (9, 9, 2), "6+9+0": (15, 9, 2), "dome": (21, 12, 1)}[name]
    assert len(facets) == n_facets and [len(f) for f in facets].count(4) == n_quads and [len(f) for f in facets].count(3) == n_triangles
    virt = range(len(xyz) - n_virtual, len(xyz))
    assert [len({v for f in facets if vv in f for v in f} - {vv}) for vv in virt] == rings
    assert sorted(facets) == sorted(model.Panner(channels).facets)
    # scipy triangulates every facet: as many simplices as the facets have triangles, each inside one facet
    simplices = ConvexHull(xyz).simplices
    assert sum(len(f) - 2 for f in facets) == len(simplices) == n_simplices
    for s in simplices:
        assert sum(set(int(v) for v in s) <= set(f) for f in facets) == 1, s
    # the entry points that take a layout name answer for a defined one
    order = capi.objects_lock_priority(name)
    full_index = [i for i, c in enumerate(channels) if not c[3]]
    assert sorted(order) == full_index
    el = {i: channels[i][2] for i in full_index}
    assert [abs(el[i]) for i in order] == sorted(abs(el[i]) for i in order)
    n = len(channels)
    mask = 1 << full_index[0] | 1 << full_index[3]
    D = capi.objects_zone_downmix(name, mask)
    assert D.shape == (n, n) and np.allclose(D[full_index].sum(axis=1), 1.0) and not D[:, [full_index[0], full_index[3]]].any()
    assert np.array_equal(capi.objects_zone_downmix(name, 0), np.eye(n))
    assert capi.objects_excluded_channels(name, [dict(min_azimuth=-180, max_azimuth=180, min_elevation=20, max_elevation=90)]) == \
        sum(1 << i for i in full_index if el[i] >= 20)
    weights = capi.loudness_layout_weights(name)
    assert len(weights) == n and all(w == 0.0 for w, c in zip(weights, channels) if c[3]) and \
        all(w in (1.0, 1.41) for w, c in zip(weights, channels) if not c[3])
    for without_lfe in (False, True):
        names = [c[0] for c in channels if not (without_lfe and c[3])]
        dec = capi.design_decorrelators_for_layout(name, without_lfe)
        assert dec.shape == (len(names), 512) and np.array_equal(dec, capi.design_decorrelators(names))
    ds = capi.DirectSpeakers(None, name)
    gains, _ = ds.calculate([{"speakerLabels": [channels[2][0]]}, {"speakerLabels": ["LFE1"], "lowPass": 120.0}])
    ds.close()
    assert ds.n_out == n and gains[0].argmax() == 2 and gains[0].sum() == 1.0
    assert gains[1].sum() == (1.0 if any(c[0] == "LFE1" for c in channels) else 0.0)


@pytest.fixture(scope="module")
def design_directions():
    return _oracle.tdesign_points()[np.linspace(0, 5199, 2000).astype(int)]


@pytest.mark.parametrize("name", ["4+5+0", "9+10+3"])
def test_model_equals_the_oracle_panner(name, design_directions):
    """tests/custom_layout_model.py, given nothing but a layout's channels, reproduces the oracle's point source panner
    (which reads the facet TABLE) within 1e-12 on 2,000 directions of the t-design plus every loudspeaker direction"""
    from libear_amd import capi
    channels = capi.layout_channels(name)
    speakers = model.cart([c[1] for c in channels if not c[3]], [c[2] for c in channels if not c[3]])
    directions = np.vstack([design_directions, speakers])
    want, want_missed = _oracle.GainCalculatorObjects(name).psp(directions)
    got, missed = model.Panner(channels).pan(directions)
    assert want_missed == 0 and not missed.any()
    print(f"{name}: largest difference between the model and the oracle {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(got[-len(speakers):] - np.eye(len(speakers))).max() <= 1e-12


def test_model_equals_the_oracle_panner_at_real_positions(design_directions):
    """... and with loudspeakers off their nominal positions (the geometry follows the real ones).  The model takes the
    facets in the table's order here, as the oracle does, so that the same region answers on a shared edge.  The bound is
    1e-9, not the 1e-12 of the nominal positions: moved loudspeakers make quads that are not flat, whose two coordinates
    are roots of a quadratic solved with the textbook formula; its b^2 - 4ac cancels, so a root carries an error of about
    2^-53 (b^2 + 4|ac|) / |b^2 - 4ac|, which is 1e-13 to 1e-11 for quads bent by a few degrees, and the two sides order
    their sums differently.  1e-9 stays three digits under the 1e-6 the GPU tests ask of the device against this model."""
    from libear_amd import capi
    channels = capi.layout_channels("4+5+0")
    rng = np.random.default_rng(5)
    az = np.array([c[1] for c in channels]) + rng.uniform(-3, 3, len(channels))
    el = np.array([c[2] for c in channels]) + rng.uniform(-3, 3, len(channels))
    want, want_missed = _oracle.GainCalculatorObjects("4+5+0", (az, el)).psp(design_directions)
    table = capi.layout_hull("4+5+0")[3]
    assert sorted(table) == sorted(model.Panner(channels).facets)
    got, missed = model.Panner(channels, (az, el), table).pan(design_directions)
    print(f"largest difference at real positions {np.abs(got - want).max():.3e}")
    assert want_missed == 0 and not missed.any() and np.abs(got - want).max() <= 1e-9


def test_symbols_are_declared_and_bound():
    from libear_amd import capi
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    lib = capi.load()
    for sym in ("earhip_layout_define", "earhip_layout_kind", "earhip_layout_hull", "earhip_panner_self_check"):
        assert sym + "(" in header and hasattr(lib, sym), sym
    assert all(hasattr(capi, f) for f in ("define_layout", "layout_kind", "layout_hull")) and hasattr(capi.Panner, "self_check")
