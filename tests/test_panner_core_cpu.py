"""The Objects gain producer's own point source panner without a device: libear_amd/csrc/panner.h — the region builder, the
region walk and the stereo downmix that the device kernels run, and a layout's lock and zone tables — compiled by plain g++
under ASan and UBSan (tests/cpp/panner_host.cpp) and held to the oracle's panner, to tests/custom_layout_model.py on a
defined layout, and to the C ABI's host entry points.  The cases and the bounds are those tests/test_custom_layout_cpu.py
asks of the Python model: 1e-12 at nominal positions, 1e-9 at real ones (the reason is written there).

Measured (x86-64, glibc, -ffp-contract=off): 0 against the oracle in all four oracle cases, the pow of 0+2+0 included — the
same bits; the defined 2+7+0 against the numpy model 8.9e-16 at nominal and 6.7e-15 at real positions."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import _oracle
import custom_layout_model as model
from layouts import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("panner_host") / "panner_host"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "panner_host.cpp"), "-o", str(path)], check=True)
    return str(path)


@pytest.fixture(scope="module")
def design_directions():
    return _oracle.tdesign_points()[np.linspace(0, 5199, 2000).astype(int)]


def run(exe, tmp_path, name, defined=None, positions=None, facets=None, directions=(), masks=(), zones=()):
    """-> (status, text) when the set-up refuses, else a dict of what the program computed"""
    from libear_amd import capi
    directions = np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
    flat = [v for f in facets for v in (len(f),) + tuple(f)] + [0] if facets is not None else []
    zs = (capi.ExclusionZone * max(len(zones), 1))()
    for z, given in zip(zs, zones):
        z.cartesian = int(any(k.endswith(("_x", "_y", "_z")) for k in given))
        for k, v in given.items():
            setattr(z, k, float(v))
    blob = struct.pack("<6i64s", len(defined or []), int(positions is not None), len(flat), len(directions), len(masks), len(zones),
                       name.encode())
    for ch in defined or []:
        blob += struct.pack("<32sddii", ch[0].encode(), float(ch[1]), float(ch[2]), int(len(ch) > 3 and ch[3]), 0)
    if positions is not None:
        blob += np.asarray(positions[0], np.float64).tobytes() + np.asarray(positions[1], np.float64).tobytes()
    blob += np.asarray(flat, np.int32).tobytes() + directions.tobytes() + np.asarray(masks, np.uint32).tobytes()
    blob += bytes(zs)[:C.sizeof(capi.ExclusionZone) * len(zones)]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([exe, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout
    out = dst.read_bytes()
    status, text_len = struct.unpack_from("<2i", out)
    if status != 0:
        return status, out[8:8 + text_len].decode()
    at = 8 + text_len
    n_pv, n_regions, n_speakers, _ = struct.unpack_from("<4i", out, at)
    at += 16
    n, n_dirs = len(defined) if defined else len(LAYOUTS[name]), len(directions)
    pv = np.frombuffer(out, np.float64, n_dirs * n_pv, at).reshape(n_dirs, n_pv)
    at += pv.nbytes
    missed = np.frombuffer(out, np.uint8, n_dirs, at).astype(bool)
    at += n_dirs
    lock_order = np.frombuffer(out, np.int32, n_speakers, at).tolist()
    at += 4 * n_speakers
    excluded, = struct.unpack_from("<I", out, at)
    downmix = np.frombuffer(out, np.float64, len(masks) * n * n, at + 4).reshape(len(masks), n, n)
    assert at + 4 + downmix.nbytes == len(out)
    return dict(pv=pv, missed=missed, n_regions=n_regions, lock_order=lock_order, excluded=excluded, downmix=downmix)


def speakers_of(name):
    from libear_amd import capi
    channels = capi.layout_channels(name)
    return model.cart([c[1] for c in channels if not c[3]], [c[2] for c in channels if not c[3]])


def moved(channels):
    """the positions of test_model_equals_the_oracle_panner_at_real_positions: seed 5, +-3 degrees"""
    rng = np.random.default_rng(5)
    az = np.array([c[1] for c in channels]) + rng.uniform(-3, 3, len(channels))
    el = np.array([c[2] for c in channels]) + rng.uniform(-3, 3, len(channels))
    return az, el


@pytest.mark.parametrize("name", ["4+5+0", "9+10+3"])
def test_core_equals_the_oracle_panner(exe, tmp_path, name, design_directions):
    speakers = speakers_of(name)
    directions = np.vstack([design_directions, speakers])
    want, want_missed = _oracle.GainCalculatorObjects(name).psp(directions)
    got = run(exe, tmp_path, name, directions=directions)
    print(f"{name}: largest difference between panner.h on the host and the oracle {np.abs(got['pv'] - want).max():.3e}")
    assert want_missed == 0 and not got["missed"].any()
    assert np.abs(got["pv"] - want).max() <= 1e-12
    assert np.abs(got["pv"][-len(speakers):] - np.eye(len(speakers))).max() <= 1e-12


def test_stereo_downmix_equals_the_oracle_panner(exe, tmp_path, design_directions):
    """0+2+0: the regions of 0+5+0 and pan_outputs' downmix, whose pow is the one libm call that could differ"""
    directions = np.vstack([design_directions, speakers_of("0+2+0")])
    want, want_missed = _oracle.GainCalculatorObjects("0+2+0").psp(directions)
    got = run(exe, tmp_path, "0+2+0", directions=directions)
    print(f"0+2+0: largest difference between panner.h on the host and the oracle {np.abs(got['pv'] - want).max():.3e}")
    assert got["pv"].shape == want.shape == (len(directions), 2)
    assert want_missed == 0 and not got["missed"].any() and np.abs(got["pv"] - want).max() <= 1e-12


def test_core_equals_the_oracle_panner_at_real_positions(exe, tmp_path, design_directions):
    from libear_amd import capi
    az, el = moved(capi.layout_channels("4+5+0"))
    want, want_missed = _oracle.GainCalculatorObjects("4+5+0", (az, el)).psp(design_directions)
    got = run(exe, tmp_path, "4+5+0", positions=(az, el), directions=design_directions)
    print(f"4+5+0 at real positions: largest difference {np.abs(got['pv'] - want).max():.3e}")
    assert want_missed == 0 and not got["missed"].any() and np.abs(got["pv"] - want).max() <= 1e-9


def test_core_equals_the_model_on_a_defined_layout(exe, tmp_path, design_directions):
    """2+7+0 of tests/custom_layout_model.py with the facet list the library made of it, nominal and moved"""
    from libear_amd import capi
    channels = model.CUSTOM["2+7+0"][0]
    capi.define_layout("2+7+0", channels)
    table = capi.layout_hull("2+7+0")[3]
    speakers = model.cart([c[1] for c in channels if not c[3]], [c[2] for c in channels if not c[3]])
    directions = np.vstack([design_directions, speakers])
    for positions, bound in ((None, 1e-12), (moved(channels), 1e-9)):
        want, want_missed = model.Panner(channels, positions, table).pan(directions if positions is None else design_directions)
        got = run(exe, tmp_path, "2+7+0", defined=channels, positions=positions, facets=table,
                  directions=directions if positions is None else design_directions)
        print(f"2+7+0 {'nominal' if positions is None else 'moved'}: largest difference {np.abs(got['pv'] - want).max():.3e}")
        assert not want_missed.any() and not got["missed"].any() and np.abs(got["pv"] - want).max() <= bound
        assert got["n_regions"] == len(model.Panner(channels, positions, table).regions)
    # without a facet list the program triangulates as earhip_layout_define does: the same regions, the same bits
    own = run(exe, tmp_path, "2+7+0", defined=channels, directions=directions)
    given = run(exe, tmp_path, "2+7+0", defined=channels, facets=table, directions=directions)
    assert np.array_equal(own["pv"], given["pv"])


def test_refusals_of_the_region_builder(exe, tmp_path):
    """every status and text of build_regions: through earhip_layout_define where a definition reaches it (the same layout
    to the C ABI and to the program), else the literal status and text the C ABI gives on a device"""
    from libear_amd import capi
    base = [("M+000", 0.0, 0.0), ("M+110", 110.0, 0.0), ("M-110", -110.0, 0.0)]
    through_define = {
        "ring of 18 (cpu core)": [(f"S{k}", -170.0 + 20.0 * k, 0.0) for k in range(18)],
        "screen at 30": [("M+SC", 30.0, 0.0), ("M-SC", -30.0, 0.0)] + base,
        "screen at 40": [("M+SC", 40.0, 0.0), ("M-SC", -40.0, 0.0)] + base,
        "screen at 3": [("M+SC", 15.0, 0.0), ("M-SC", -3.0, 0.0)] + base,
        "twice (cpu core)": base + [("D", 110.0, 0.0)],
    }
    seen = set()
    for name, channels in through_define.items():
        with pytest.raises(capi.EarHipError) as info:
            capi.define_layout(name, channels)
        assert run(exe, tmp_path, name, defined=channels) == (info.value.code, str(info.value)), name
        seen.add(str(info.value))
    assert seen == {"more than 16 loudspeakers around a virtual loudspeaker", "collinear points in convex hull",
                    "M+SC or M-SC has azimuth not in the allowed ranges of 5 to 25 and 35 to 60 degrees",
                    "M+SC and M-SC with azimuths wider than 25 degrees are not currently supported"}
    # real positions need a device through the C ABI (tests/test_gpu_panner.py): the texts of libear
    names = LAYOUTS["4+9+0"]
    az, el = (np.array(v, np.float64) for v in zip(*[c[1:3] for c in capi.layout_channels("4+9+0")]))
    for label, sign in (("M+SC", 1.0), ("M-SC", -1.0)):
        for value, want in ((40.0, (capi.NOT_IMPLEMENTED, "M+SC and M-SC with azimuths wider than 25 degrees are not currently supported")),
                            (30.0, (capi.INVALID_ARGUMENT, "M+SC or M-SC has azimuth not in the allowed ranges of 5 to 25 and 35 to 60 degrees"))):
            a = az.copy()
            a[names.index(label)] = sign * value
            assert run(exe, tmp_path, "4+9+0", positions=(a, el)) == want
    # facet lists no hull gives: both virtual loudspeakers in one facet, a ring of two, a facet of five
    table = capi.layout_hull("4+5+0")[3]
    n_vertices = len(capi.layout_hull("4+5+0")[0])
    bottom, top = n_vertices - 2, n_vertices - 1
    assert run(exe, tmp_path, "4+5+0", facets=table + [(0, bottom, top)]) == (capi.INVALID_ARGUMENT, "invalid triangulation")
    assert run(exe, tmp_path, "4+5+0", facets=[(0, 1, bottom)]) == (capi.INVALID_ARGUMENT, "unsupported n-gon size")
    assert run(exe, tmp_path, "4+5+0", facets=table + [(0, 1, 2, 4, 5)]) == \
        (capi.INTERNAL_ERROR, "internal error: facets with more than 4 vertices are not supported")
    assert isinstance(run(exe, tmp_path, "4+5+0", facets=table), dict)


@pytest.mark.parametrize("name", ["4+5+0", "9+10+3", "0+2+0", "2+7+0"])
def test_lock_and_zone_tables_equal_the_c_abi(exe, tmp_path, name):
    from libear_amd import capi
    defined = model.CUSTOM[name][0] if name in model.CUSTOM else None
    if defined:
        capi.define_layout(name, defined)
    channels = capi.layout_channels(name)
    real = [i for i, c in enumerate(channels) if not c[3]]
    rng = np.random.default_rng(sum(map(ord, name)))
    masks = [0, sum(1 << i for i in real)] + [1 << i for i in real] + [int(m) for m in rng.integers(0, 1 << len(channels), 20)]
    zone_sets = [[], [dict(min_azimuth=150.0, max_azimuth=-150.0, min_elevation=-90.0, max_elevation=90.0)],
                 [dict(min_azimuth=-180.0, max_azimuth=180.0, min_elevation=20.0, max_elevation=90.0),
                  dict(min_x=-1.0, max_x=1.0, min_y=-1.0, max_y=-1e-3, min_z=-1.0, max_z=1.0)],
                 [dict(min_azimuth=30.0, max_azimuth=30.0, min_elevation=-5.0, max_elevation=5.0)]]
    for zones in zone_sets:
        got = run(exe, tmp_path, name, defined=defined, masks=masks if zones == [] else (), zones=zones)
        assert got["lock_order"] == capi.objects_lock_priority(name)
        assert got["excluded"] == capi.objects_excluded_channels(name, zones)
        if zones == []:
            for mask, matrix in zip(masks, got["downmix"]):
                assert np.array_equal(matrix, capi.objects_zone_downmix(name, mask)), mask
    assert run(exe, tmp_path, name, defined=defined, masks=[1 << len(channels)]) == \
        (capi.INVALID_ARGUMENT, f"mask has a bit set beyond the layout's {len(channels)} channels")
