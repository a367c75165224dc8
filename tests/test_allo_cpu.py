"""The allocentric (Cartesian) point-source panner's host forms (include/earhip.h group T), without a device: the known answers
of the specification, earhip_allo_calculate against the float64 model of tests/allo_model.py, the loudspeaker table, the
snapping, the refusals and the bindings; and libear_amd/csrc/allo.h alone under ASan + UBSan (tests/cpp/test_allo_core.cpp)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import allo_model as M
from layouts import LAYOUTS
from libear_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2 = np.float32(math.sqrt(0.5))
R8 = np.float32(math.sqrt(0.125))
HALF = np.float32(0.5)

# (layout, position, excluded channel names, {channel name: expected float32}); every other channel is 0
KNOWN = [
    ("0+5+0", (0.0, 1.0, 0.0), (), {"M+000": 1.0}),
    ("0+5+0", (-0.5, 1.0, 0.0), (), {"M+030": R2, "M+000": R2}),
    ("0+5+0", (0.0, 0.0, 0.0), (), {"M+000": R2, "M+110": HALF, "M-110": HALF}),
    ("0+5+0", (0.0, 0.0, 3.0), (), {"M+000": R2, "M+110": HALF, "M-110": HALF}),
    ("0+5+0", (0.0, 1.0, 0.0), ("M+000",), {"M+030": R2, "M-030": R2}),
    ("4+5+0", (0.0, 0.0, 0.5), (), {"M+000": HALF, "M+110": R8, "M-110": R8, "U+030": R8, "U-030": R8, "U+110": R8, "U-110": R8}),
    ("9+10+3", (0.0, 0.0, 1.0), (), {"T+000": 1.0}),
    ("9+10+3", (-1.0, 1.0, 0.0), (), {"M+030": 1.0}),
    ("9+10+3", (0.0, 0.0, 0.0), (), {"M+090": R2, "M-090": R2}),
    ("3+7+0", (0.5, -1.0, 1.0), (), {"UH+180": 1.0}),
    ("3+7+0", (0.0, 0.0, 0.5), (), {"M+090": HALF, "M-090": HALF, "UH+180": HALF, "U+045": R8, "U-045": R8}),
]


def mask_of(layout, names):
    return sum(1 << LAYOUTS[layout].index(n) for n in names)


@pytest.fixture(scope="module")
def handles():
    made = {name: capi.Allo(name) for name in LAYOUTS}
    yield made
    for a in made.values():
        a.close()


@pytest.fixture(scope="module")
def random_batches():
    """per BS.2051 layout: 2000 positions in [-1.3, 1.3]^3 with gains, diffuse values and masks, the special positions last,
    and the model's float64 rows for them — computed once"""
    out = {}
    for k, layout in enumerate(LAYOUTS):
        rng = np.random.default_rng(2127 + k)
        n = 2000
        pos = rng.uniform(-1.3, 1.3, (n, 3))
        pos[-len(M.SPECIAL):] = M.SPECIAL
        gain = rng.uniform(0.05, 2.0, n)
        diffuse = rng.uniform(0.0, 1.0, n)
        nch = len(LAYOUTS[layout])
        mask = rng.integers(0, 1 << nch, n, dtype=np.uint32) & rng.integers(0, 1 << nch, n, dtype=np.uint32)
        mask[::7] = 0
        mask[3::50] = (1 << nch) - 1  # everything excluded: the same as nothing
        model = M.Model(layout)
        out[layout] = (pos, gain, diffuse, mask, model.calculate64(pos[:, 0], pos[:, 1], pos[:, 2], gain, diffuse, mask))
    return out


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_known_answers_are_exact_in_float32(handles, case):
    layout, (x, y, z), excluded, expected = KNOWN[case]
    names = LAYOUTS[layout]
    want = np.zeros(len(names), np.float32)
    for name, v in expected.items():
        want[names.index(name)] = v
    direct, diffuse = handles[layout].calculate(x, y, z, excluded=mask_of(layout, excluded) if excluded else None)
    assert direct.dtype == np.float32 and direct.shape == (1, len(names))
    assert np.array_equal(direct[0], want), (direct[0], want)
    assert np.array_equal(diffuse[0].view(np.uint32), np.zeros(len(names), np.uint32))  # +0 everywhere
    # the throw-away model of the specification agrees
    ok, worst = M.within_one_spacing(direct, M.Model(layout).calculate64(x, y, z, excluded=mask_of(layout, excluded))[0])
    assert ok, worst


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_host_form_is_within_one_float32_spacing_of_the_model(handles, random_batches, layout):
    pos, gain, diffuse, mask, (want_d, want_f) = random_batches[layout]
    direct, diff = handles[layout].calculate(pos[:, 0], pos[:, 1], pos[:, 2], gain, diffuse, mask)
    for got, want, what in ((direct, want_d, "direct"), (diff, want_f, "diffuse")):
        ok, worst = M.within_one_spacing(got, want)
        same = np.mean(got == want.astype(np.float32))
        print(f"{layout} {what}: worst error {worst:.3f} spacings, {100 * same:.2f}% bit-identical to float32(model)")
        assert ok, worst
    power = np.sum(direct.astype(np.float64) ** 2, axis=1) + np.sum(diff.astype(np.float64) ** 2, axis=1)
    assert np.all(np.abs(power - gain ** 2) <= 1e-6 * gain ** 2), np.max(np.abs(power - gain ** 2) / gain ** 2)
    assert np.all(np.count_nonzero(direct, axis=1) <= 8)
    lfe = [c for c, name in enumerate(LAYOUTS[layout]) if M.is_lfe(name)]
    assert np.all(direct[:, lfe].view(np.uint32) == 0) and np.all(diff[:, lfe].view(np.uint32) == 0)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_a_loudspeakers_own_position_gives_the_gain_there_and_zero_elsewhere(handles, layout):
    a = handles[layout]
    xyz = a.positions()
    for c, name in enumerate(LAYOUTS[layout]):
        if M.is_lfe(name):
            assert np.all(np.isnan(xyz[c]))
            continue
        direct, _ = a.calculate(*xyz[c], gain=0.75)
        want = np.zeros(len(xyz), np.float32)
        want[c] = 0.75
        assert np.array_equal(direct[0].view(np.uint32), want.view(np.uint32)), (name, direct[0])


def test_a_mask_that_excludes_every_loudspeaker_equals_no_mask(handles, random_batches):
    for layout in ("0+2+0", "3+7+0", "9+10+3"):
        pos = random_batches[layout][0][:200]
        a = handles[layout]
        nch = len(LAYOUTS[layout])
        none = a.calculate(pos[:, 0], pos[:, 1], pos[:, 2])
        every = a.calculate(pos[:, 0], pos[:, 1], pos[:, 2], excluded=(1 << nch) - 1)
        speakers = a.calculate(pos[:, 0], pos[:, 1], pos[:, 2],
                               excluded=mask_of(layout, [n for n in LAYOUTS[layout] if not M.is_lfe(n)]))
        only_lfe = a.calculate(pos[:, 0], pos[:, 1], pos[:, 2],
                               excluded=mask_of(layout, [n for n in LAYOUTS[layout] if M.is_lfe(n)]))
        for other in (every, speakers, only_lfe):
            assert np.array_equal(none[0].view(np.uint32), other[0].view(np.uint32))


def test_negative_zero_coordinates(handles):
    a = handles["0+5+0"]
    plus = a.calculate([0.0, 0.0], [0.0, 1.0], [0.0, 0.0])
    minus = a.calculate([-0.0, -0.0], [-0.0, 1.0], [-0.0, -0.0])
    assert np.array_equal(plus[0].view(np.uint32), minus[0].view(np.uint32))
    assert np.array_equal(plus[1].view(np.uint32), minus[1].view(np.uint32))


def test_gain_and_diffuse_split(handles):
    a = handles["4+5+0"]
    base, _ = a.calculate(0.3, -0.2, 0.4)
    w = M.Model("4+5+0").weights(0.3, -0.2, 0.4)
    for g, d in ((1.0, 0.0), (0.5, 1.0), (1.7, 0.36), (-0.8, 0.36)):
        direct, diff = a.calculate(0.3, -0.2, 0.4, gain=g, diffuse=d)
        ok, worst = M.within_one_spacing(direct[0], w * g * math.sqrt(1.0 - d))
        assert ok, worst
        ok, worst = M.within_one_spacing(diff[0], w * g * math.sqrt(d))
        assert ok, worst
        if d == 0.0:
            assert np.array_equal(direct, base) and not np.any(diff)
        if d == 1.0:
            assert not np.any(direct) and np.array_equal(diff, (base.astype(np.float64) * g).astype(np.float32))
        if d == 0.36:  # sqrt(0.64) and sqrt(0.36) are within an ulp of 0.8 and 0.6
            assert np.allclose(direct, base * np.float32(g * 0.8), rtol=3e-7, atol=0)
            assert np.allclose(diff, base * np.float32(g * 0.6), rtol=3e-7, atol=0)


def test_table_is_complete_and_mirror_symmetric(handles):
    for layout, names in LAYOUTS.items():
        xyz = handles[layout].positions()
        assert xyz.shape == (len(names), 3)
        want = M.table_positions(layout)
        assert np.array_equal(np.isnan(xyz), np.isnan(want)) and np.array_equal(np.nan_to_num(xyz), np.nan_to_num(want)), layout
        for c, name in enumerate(names):
            if M.is_lfe(name):
                assert np.all(np.isnan(xyz[c])), (layout, name)
                continue
            assert np.all(np.isfinite(xyz[c])) and np.all(np.abs(xyz[c]) <= 1.0), (layout, name)
            if name[1] == "+" and name[-3:] not in ("000", "180"):  # a left loudspeaker and its right twin
                twin = names.index(name.replace("+", "-", 1))
                assert xyz[c, 0] < 0.0 and np.array_equal(xyz[twin], xyz[c] * [-1.0, 1.0, 1.0]), (layout, name)
            elif "-" not in name:
                assert xyz[c, 0] == 0.0, (layout, name)
    # every loudspeaker name of the ten layouts is a key of the data beside layout_table.h
    text = open(os.path.join(ROOT, "libear_amd", "csrc", "allo_table.h")).read()
    keyed = set(re.findall(r'\{(?:nullptr|"[^"]+"), "([^"]+)",', text))
    used = {n for names in LAYOUTS.values() for n in names if not M.is_lfe(n)}
    assert used <= keyed, used - keyed


def test_snapping_joins_5e_7_and_keeps_2e_6_apart():
    names = LAYOUTS["0+5+0"]
    pos = np.array(M.table_positions("0+5+0"))
    pos[names.index("M+030"), 1] = 1.0 + 5e-7   # joins the front row (M+000 and M-030 at y = 1, the group's first value)
    pos[names.index("M+110"), 1] = -1.0 + 2e-6  # a row of its own
    pos[names.index("LFE1")] = [np.inf, np.nan, 7.0]  # ignored
    a = capi.Allo("0+5+0", pos)
    got = a.positions()
    assert got[names.index("M+030"), 1] == 1.0 and got[names.index("M+110"), 1] == -1.0 + 2e-6
    assert np.all(np.isnan(got[names.index("LFE1")]))
    assert np.array_equal(np.nan_to_num(got), np.nan_to_num(M.Model(positions=pos, lfe=[M.is_lfe(n) for n in names]).p))
    # joined: (-0.5, 1, 0) is between M+030 and M+000 alone; the row 2e-6 above the back takes what lies in between
    direct, _ = a.calculate([-0.5, 0.0], [1.0, -1.0 + 1e-6], [0.0, 0.0])
    want = np.zeros(6, np.float32)
    want[[names.index("M+030"), names.index("M+000")]] = R2
    assert np.array_equal(direct[0], want)
    assert direct[1][names.index("M+110")] == R2 and direct[1][names.index("M-110")] == R2
    a.close()
    # the walk measures from the FIRST value of a group: 0, 0.9e-6 and 1.8e-6 are two groups
    pos = np.array(M.table_positions("0+5+0"))
    pos[names.index("M+030"), 2], pos[names.index("M-030"), 2] = 0.9e-6, 1.8e-6
    a = capi.Allo("0+5+0", pos)
    assert a.positions()[names.index("M+030"), 2] == 0.0 and a.positions()[names.index("M-030"), 2] == 1.8e-6
    a.close()


def test_creation_refusals():
    names = LAYOUTS["0+5+0"]
    good = M.table_positions("0+5+0")
    with pytest.raises(capi.UnknownLayout):
        capi.Allo("no such layout")
    with pytest.raises(capi.UnknownLayout):
        capi.Allo("no such layout", good)
    channels, pos = M.dome32()
    capi.define_layout(M.DOME32_NAME, channels)
    with pytest.raises(capi.NotImplementedInLibear):
        capi.Allo(M.DOME32_NAME)  # a defined layout has no table
    dup = good.copy()
    dup[names.index("M+110")] = dup[names.index("M-110")] + [0.0, 5e-7, 0.0]  # the same position after snapping
    with pytest.raises(capi.InvalidArgument) as e:
        capi.Allo("0+5+0", dup)
    assert "M+110" in str(e.value) and "M-110" in str(e.value)
    for bad in (np.nan, np.inf, -np.inf):
        p = good.copy()
        p[names.index("M+000"), 1] = bad
        with pytest.raises(capi.InvalidArgument):
            capi.Allo("0+5+0", p)
    with pytest.raises(capi.InvalidArgument):
        capi.Allo("0+5+0", good[:5])  # n_channels
    with pytest.raises(capi.InvalidArgument):
        capi.Allo("0+5+0", np.vstack([good, good[:1]]))
    lib = capi.load()
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    col = np.ascontiguousarray(good[:, 0])
    assert lib.earhip_allo_create(b"0+5+0", None) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_create(None, C.byref(h)) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_create_positions(b"0+5+0", 6, None, col.ctypes.data_as(dp), col.ctypes.data_as(dp),
                                            C.byref(h)) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_num_channels(None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_positions(None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_destroy(None) == capi.OK


def test_a_32_channel_defined_layout_with_caller_positions():
    channels, pos = M.dome32()
    capi.define_layout(M.DOME32_NAME, channels)
    lfe = [ch[3] for ch in channels]
    a = capi.Allo(M.DOME32_NAME, pos)
    model = M.Model(positions=pos, lfe=lfe)
    assert a.n_out == 32 and np.array_equal(np.nan_to_num(a.positions()), np.nan_to_num(model.p))
    rng = np.random.default_rng(32)
    n = 500
    p = rng.uniform(-1.3, 1.3, (n, 3))
    p[-len(M.SPECIAL):] = M.SPECIAL
    gain, diffuse = rng.uniform(0.05, 2.0, n), rng.uniform(0.0, 1.0, n)
    mask = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    mask[0] = 0xffffffff  # bit 31 is a channel of this layout
    direct, diff = a.calculate(p[:, 0], p[:, 1], p[:, 2], gain, diffuse, mask)
    want_d, want_f = model.calculate64(p[:, 0], p[:, 1], p[:, 2], gain, diffuse, mask)
    for got, want in ((direct, want_d), (diff, want_f)):
        ok, worst = M.within_one_spacing(got, want)
        assert ok, worst
    assert np.all(direct[:, lfe] == 0) and np.all(np.count_nonzero(direct, axis=1) <= 8)
    a.close()


def test_host_form_refusals_name_the_index_and_write_the_rows_before_it(handles):
    a = handles["0+5+0"]
    n, at = 5, 3
    base = dict(x=np.linspace(-1, 1, n), y=np.linspace(1, -1, n), z=np.zeros(n), gain=np.ones(n), diffuse=np.full(n, 0.25),
                excluded=np.zeros(n, np.uint32))
    clean = a.calculate(**base)
    cases = [(k, v) for k in ("x", "y", "z", "gain") for v in (np.nan, np.inf, -np.inf)]
    cases += [("diffuse", v) for v in (np.nan, -1e-9, 1.0000001, np.inf)]
    cases += [("excluded", 1 << 6), ("excluded", 1 << 31)]  # 0+5+0 has 6 channels
    for key, bad in cases:
        args = {k: v.copy() for k, v in base.items()}
        args[key][at] = bad
        with pytest.raises(capi.InvalidArgument) as e:
            a.calculate(**args)
        assert f"element {at}:" in str(e.value), str(e.value)
        for got, want in zip(e.value.partial, clean):
            assert np.array_equal(got[:at].view(np.uint32), want[:at].view(np.uint32)), key
            assert np.all(np.isnan(got[at:])), key  # (the binding's fill: not written)
    # an LFE bit is not beyond the layout: ignored
    ok = a.calculate(**dict(base, excluded=np.full(n, 1 << 3, np.uint32)))
    assert np.array_equal(ok[0], clean[0])
    # NULL pointers and diffuse without diffuse_out, through the C ABI itself
    lib = capi.load()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    v = np.zeros(2)
    out = np.zeros(12, np.float32)
    p, o = v.ctypes.data_as(dp), out.ctypes.data_as(fp)
    assert lib.earhip_allo_calculate(a.h, C.c_size_t(2), p, p, p, None, None, None, o, None) == capi.OK
    assert lib.earhip_allo_calculate(a.h, C.c_size_t(2), p, p, p, None, p, None, o, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_calculate(a.h, C.c_size_t(2), None, p, p, None, None, None, o, o) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_calculate(a.h, C.c_size_t(2), p, p, p, None, None, None, None, o) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_calculate(None, C.c_size_t(2), p, p, p, None, None, None, o, o) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_calculate(a.h, C.c_size_t(1 << 31), p, p, p, None, None, None, o, o) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_calculate(a.h, C.c_size_t(0), None, None, None, None, None, None, None, None) == capi.OK
    assert lib.earhip_allo_calculate_device(None, a.h, C.c_size_t(0), None, None, None, None, None, None, None, None,
                                            None) == capi.INVALID_ARGUMENT


def test_excluded_channels_takes_cartesian_zones_at_the_handles_positions(handles):
    a = handles["9+10+3"]
    names = LAYOUTS["9+10+3"]
    model = M.Model("9+10+3")
    zones = [dict(min_x=-1, max_x=1, min_y=-1, max_y=1, min_z=1, max_z=1),       # the ceiling
             dict(min_x=-1, max_x=-0.5, min_y=0.9, max_y=1, min_z=-1, max_z=0)]  # front left, below and middle
    for zs in ([], zones[:1], zones[1:], zones):
        assert a.excluded_channels(zs) == model.excluded_channels(zs)
    top = {names[c] for c in range(len(names)) if (a.excluded_channels(zones[:1]) >> c) & 1}
    assert top == {n for n in names if n[0] in "UT"}
    # M+030 of 9+10+3 stands at x = -s, outside the second zone; B+045 at x = -1 inside
    second = {names[c] for c in range(len(names)) if (a.excluded_channels(zones[1:]) >> c) & 1}
    assert second == {"B+045"}
    # the bounds are open by 1e-6
    edge = dict(min_x=5e-7, max_x=1, min_y=1, max_y=1, min_z=0, max_z=0)
    assert (a.excluded_channels([edge]) >> names.index("M+000")) & 1
    edge["min_x"] = 2e-6
    assert not (a.excluded_channels([edge]) >> names.index("M+000")) & 1
    with pytest.raises(capi.InvalidArgument) as e:
        a.excluded_channels([zones[0], dict(min_azimuth=-30, max_azimuth=30, min_elevation=-10, max_elevation=10)])
    assert "zone 1" in str(e.value) and "polar" in str(e.value)
    # against caller positions, not nominal ones
    pos = M.table_positions("0+5+0") * 0.5
    b = capi.Allo("0+5+0", pos)
    assert b.excluded_channels([dict(min_x=-0.5, max_x=0.5, min_y=0.5, max_y=0.5, min_z=0, max_z=0)]) == 0b000111
    assert b.excluded_channels([dict(min_x=-1, max_x=1, min_y=1, max_y=1, min_z=0, max_z=0)]) == 0
    b.close()


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    lib = capi.load()
    for name in ("earhip_allo_create", "earhip_allo_create_positions", "earhip_allo_destroy", "earhip_allo_num_channels",
                 "earhip_allo_positions", "earhip_allo_excluded_channels", "earhip_allo_calculate",
                 "earhip_allo_calculate_device"):
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert hasattr(lib, name), name
    assert callable(capi.allo_calculate_device) and callable(capi.Allo.calculate)
    assert "without a reference implementation" in re.sub(r"\s+", " ", header.lower().replace("*", ""))
    hpp = open(os.path.join(ROOT, "libear_amd", "host", "ear", "hip_allo.hpp")).read()
    assert "class AllocentricGainCalculator" in hpp


def test_core_alone_under_asan_and_ubsan(tmp_path):
    """libear_amd/csrc/allo.h compiled by g++ without HIP, as a program of its own under ASan + UBSan
    (tests/cpp/test_allo_core.cpp): the known answers of the specification, and 2 and 32 channels"""
    exe = tmp_path / "test_allo_core"
    src = os.path.join(ROOT, "tests", "cpp", "test_allo_core.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "libear_amd", "csrc"), src, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0 and re.search(r"^\d+ checked, 0 failed$", res.stdout, flags=re.M), res.stdout
