"""The host form of the allocentric panner with extent, channelLock and divergence (earhip_allo_calculate_objects,
include/earhip.h group U), without a device: against the float64 brute-force model of tests/allo_objects_model.py, the bit
rule for plain rows, the power, flat axes, lock ties, maxDistance, divergence edges, every refusal and the bindings; and
libear_amd/csrc/allo_objects.h alone under ASan + UBSan (tests/cpp/test_allo_objects_core.cpp).

The bar is allo_model.within_one_spacing: one float32 spacing at max(|want|, 2^-20) against float32(model).  It is derived,
not measured: every term is positive, the float64 error of a few hundred operations and a few pow calls is below 1e-12
relative, 5 orders under half a float32 spacing, so the single rounding lands on the model's float or its neighbour."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import allo_model as M
import allo_objects_model as OM
from libear_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 0+2+0: y and z flat; 0+5+0: z flat
NAMES = ("0+2+0", "0+5+0", "4+5+1", "3+7+0", "9+10+3", M.DOME32_NAME)


def host(allo, b):
    return allo.calculate_objects(*(b[k] for k in OM.KEYS))


def one(allo, **kw):
    """the direct row of one object, float64"""
    return allo.calculate_objects(kw.pop("x"), kw.pop("y"), kw.pop("z"), **kw)[0][0].astype(np.float64)


@pytest.mark.parametrize("name", NAMES)
def test_host_form_against_the_brute_force_model(name):
    allo, model, _ = OM.handle(name)
    b, (want_d, want_f) = OM.reference(name)
    got_d, got_f = host(allo, b)
    lfe = np.array(model.lfe)
    for what, got, want in (("direct", got_d, want_d), ("diffuse", got_f, want_f)):
        ok, worst = M.within_one_spacing(got, want)
        print(f"{name} {what}: worst error {worst:.3f} spacings over {len(got)} rows")
        assert ok, (what, worst)
        assert np.all(got[:, lfe].view(np.uint32) == 0)
    power = np.sum(got_d.astype(np.float64) ** 2 + got_f.astype(np.float64) ** 2, axis=1)
    assert np.allclose(power, b["gain"] ** 2, rtol=1e-6, atol=0), np.max(np.abs(power / b["gain"] ** 2 - 1))


@pytest.mark.parametrize("name", NAMES)
def test_plain_rows_have_the_bits_of_the_point_source_form(name):
    allo, _, om = OM.handle(name)
    b, _ = OM.reference(name)
    flat_size = {k: b[k].copy() for k in ("width", "depth", "height")}
    s_max = np.max([np.minimum(flat_size[k], 1.0) * (not om.flat[a]) for a, k in enumerate(("width", "depth", "height"))], axis=0)
    is_plain = (b["channel_lock"] == 0) & (b["divergence"] == 0) & (s_max == 0)
    assert np.count_nonzero(is_plain) >= OM.FULL // 4
    got = host(allo, b)
    want = allo.calculate(b["x"], b["y"], b["z"], b["gain"], b["diffuse"], b["excluded"])
    for g, w in zip(got, want):
        assert np.array_equal(g[is_plain].view(np.uint32), w[is_plain].view(np.uint32))
    # every optional array absent: the point-source form's defaults
    bare = allo.calculate_objects(b["x"], b["y"], b["z"])
    want = allo.calculate(b["x"], b["y"], b["z"])
    assert np.array_equal(bare[0].view(np.uint32), want[0].view(np.uint32)) and np.all(bare[1].view(np.uint32) == 0)


def test_a_negative_gain_keeps_plus_zero_where_the_point_source_form_has_it():
    allo, _, _ = OM.handle("4+5+1")
    got = allo.calculate_objects(0.3, 0.2, 0.1, gain=-1.5, diffuse=0.25)
    want = allo.calculate(0.3, 0.2, 0.1, -1.5, 0.25)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_a_size_on_a_flat_axis_changes_nothing():
    allo, _, om = OM.handle("0+5+0")
    assert om.flat == [False, False, True]
    a = allo.calculate_objects(0.3, 0.2, 0.0, width=0.5, depth=0.1)
    b = allo.calculate_objects(0.3, 0.2, 0.0, width=0.5, depth=0.1, height=1.7)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    point = allo.calculate(0.3, 0.2, 0.0)
    only_flat = allo.calculate_objects(0.3, 0.2, 0.0, height=0.5)
    assert np.array_equal(point[0].view(np.uint32), only_flat[0].view(np.uint32))
    allo2, _, om2 = OM.handle("0+2+0")
    assert om2.flat == [False, True, True]
    assert np.array_equal(allo2.calculate_objects(0.3, 0.2, 0.0, depth=1.0, height=1.0)[0].view(np.uint32),
                          allo2.calculate(0.3, 0.2, 0.0)[0].view(np.uint32))


def test_full_extent_spreads_over_every_loudspeaker_and_a_small_one_stays_near_the_point_source():
    allo, model, _ = OM.handle("9+10+3")
    g = one(allo, x=0.0, y=0.0, z=0.0, width=1.7, height=1.7, depth=1.7)
    assert np.all(g[model.real] > 0.01) and np.all(g[[c for c in range(model.n) if model.lfe[c]]] == 0)
    allo, _, _ = OM.handle("0+5+0")
    small = one(allo, x=-1.0, y=1.0, z=0.0, width=0.03)
    point = one(allo, x=-1.0, y=1.0, z=0.0)
    assert abs(small[np.argmax(point)] - 1.0) < 0.1 and not np.array_equal(small, point)


def test_lock_priority_is_the_documented_order():
    for name in NAMES:
        allo, model, om = OM.handle(name)
        assert allo.lock_priority() == om.order and sorted(om.order) == model.real
    allo, model, _ = OM.handle("0+5+0")
    names = [capi.layout_channels("0+5+0")[c][0] for c in allo.lock_priority()]
    assert names == ["M+000", "M+030", "M-030", "M+110", "M-110"]


def test_a_lock_tie_goes_to_the_first_in_the_priority_order():
    allo, model, om = OM.handle("0+5+0")
    # between the two rear loudspeakers nothing else is as near: the tie goes to the left one, first in the order
    rear_l, rear_r = (c for c in om.order if tuple(model.p[c]) in ((-1.0, -1.0, 0.0), (1.0, -1.0, 0.0)))
    assert om.order.index(rear_l) < om.order.index(rear_r)
    g = one(allo, x=0.0, y=-1.0, z=0.0, channel_lock=1)
    assert g[rear_l] == 1.0 and np.count_nonzero(g) == 1
    g = one(allo, x=1e-9, y=-1.0, z=0.0, channel_lock=1)  # off the tie by more than the tolerance: the nearer one
    assert g[rear_r] == 1.0 and np.count_nonzero(g) == 1
    g = one(allo, x=1e-12, y=-1.0, z=0.0, channel_lock=1)  # within 1e-10 of the tie: still the priority order
    assert g[rear_l] == 1.0


def test_max_distance_just_below_and_above_the_nearest_loudspeaker():
    allo, model, om = OM.handle("4+5+1")
    x, y, z = 0.7, 0.6, 0.2
    d = min(math.sqrt((1 / 16) * (x - p[0]) ** 2 + 4 * (y - p[1]) ** 2 + 32 * (z - p[2]) ** 2) for p in model.p[model.real])
    unlocked = one(allo, x=x, y=y, z=z)
    below = one(allo, x=x, y=y, z=z, channel_lock=1, lock_max_distance=d - 1e-9)
    above = one(allo, x=x, y=y, z=z, channel_lock=1, lock_max_distance=d + 1e-9)
    assert np.array_equal(below, unlocked)
    assert np.count_nonzero(above) == 1 and above.max() == 1.0
    assert np.array_equal(one(allo, x=x, y=y, z=z, channel_lock=1, lock_max_distance=0.0), unlocked)
    assert np.array_equal(one(allo, x=x, y=y, z=z, channel_lock=1), above)  # no maxDistance
    assert np.array_equal(one(allo, x=x, y=y, z=z, channel_lock=0, lock_max_distance=d + 1e-9), unlocked)  # no flag


def test_a_lock_onto_an_excluded_loudspeaker():
    allo, model, om = OM.handle("0+5+0")
    centre = om.order[0]  # M+000 at (0, 1, 0)
    g = one(allo, x=0.05, y=0.95, z=0.0, channel_lock=1, excluded=1 << centre)
    want = om.gains(0.05, 0.95, 0.0, lock=True, mask=1 << centre)
    assert g[centre] == 0.0 and np.count_nonzero(g) == 2  # at (0, 1, 0) without M+000: between M+030 and M-030
    ok, _ = M.within_one_spacing(g.astype(np.float32), want)
    assert ok and np.array_equal(g, one(allo, x=0.0, y=1.0, z=0.0, excluded=1 << centre))


def test_divergence_edges():
    allo, _, om = OM.handle("0+5+0")
    # v == 1: the centre position has weight 0
    g = one(allo, x=0.0, y=1.0, z=0.0, divergence=1.0, position_range=1.0)
    assert g[om.order[0]] == 0.0
    assert np.allclose(sorted(g)[-2:], [math.sqrt(0.5)] * 2, rtol=1e-7)
    # r == 0: the undiverged row, to the bar
    for kw in ({}, {"width": 0.5, "depth": 0.2}):
        a = allo.calculate_objects(0.3, 0.2, 0.0, divergence=0.5, position_range=0.0, **kw)[0]
        b = allo.calculate_objects(0.3, 0.2, 0.0, **kw)[0]
        ok, worst = M.within_one_spacing(a, b.astype(np.float64))
        assert ok, worst
    # the side positions are clipped by bracket(), not before
    far = one(allo, x=0.0, y=1.0, z=0.0, divergence=0.5, position_range=5.0)
    edge = one(allo, x=0.0, y=1.0, z=0.0, divergence=0.5, position_range=1.0)
    assert np.array_equal(far, edge)


REFUSED = [("x", np.nan), ("y", np.inf), ("z", -np.inf), ("gain", np.nan), ("gain", np.inf), ("diffuse", -1e-9),
           ("diffuse", 1.0000001), ("diffuse", np.nan), ("width", -1e-9), ("width", np.nan), ("height", np.inf),
           ("depth", -1.0), ("depth", np.nan), ("divergence", -1e-9), ("divergence", 1.0000001), ("divergence", np.nan),
           ("position_range", -1e-9), ("position_range", np.nan), ("position_range", np.inf), ("lock_max_distance", -1e-9),
           ("lock_max_distance", np.nan), ("excluded", 1 << 12)]


@pytest.mark.parametrize("key,value", REFUSED)
def test_each_refusal_names_the_index_and_leaves_the_rows_before_it_written(key, value):
    allo, _, _ = OM.handle("3+7+0")  # 12 channels
    b = OM.last(OM.reference("3+7+0")[0], 24)
    clean = host(allo, b)
    b[key][17] = value
    with pytest.raises(capi.InvalidArgument, match=r"element 17\b") as e:
        host(allo, b)
    for got, want in zip(e.value.partial, clean):
        assert np.array_equal(got[:17].view(np.uint32), want[:17].view(np.uint32))
        assert np.all(np.isnan(got[17:]))


def test_accepted_edges_and_argument_checks():
    allo, _, _ = OM.handle("3+7+0")
    d, f = allo.calculate_objects(0.1, 0.2, 0.3, width=0.0, divergence=1.0, position_range=0.0, lock_max_distance=np.inf,
                                  channel_lock=1, diffuse=1.0)
    assert np.all(d == 0) and np.isclose(np.sum(f.astype(np.float64) ** 2), 1.0, rtol=1e-6)
    lib = capi.load()
    x = np.zeros(1)
    out = np.zeros(12, np.float32)
    p64, pf = C.POINTER(C.c_double), C.POINTER(C.c_float)
    args = [x.ctypes.data_as(p64)] * 3 + [None] * 10
    assert lib.earhip_allo_calculate_objects(allo.h, C.c_size_t(0), *([None] * 15)) == capi.OK  # n == 0: a no-op
    assert lib.earhip_allo_calculate_objects(allo.h, C.c_size_t(1), *args, out.ctypes.data_as(pf), None) == capi.OK
    args[7] = x.ctypes.data_as(p64)  # diffuse without diffuse_out
    assert lib.earhip_allo_calculate_objects(allo.h, C.c_size_t(1), *args, out.ctypes.data_as(pf), None) == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_calculate_objects(None, C.c_size_t(1), *args, out.ctypes.data_as(pf), out.ctypes.data_as(pf)) \
        == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_calculate_objects(allo.h, C.c_size_t(1 << 31), *args, out.ctypes.data_as(pf), out.ctypes.data_as(pf)) \
        == capi.INVALID_ARGUMENT
    assert lib.earhip_allo_lock_priority(allo.h, None) == capi.INVALID_ARGUMENT


def test_header_core_and_model_agree_on_the_constants_and_the_symbols_are_exported():
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    text = re.sub(r"\s+", " ", header.replace("*", ""))
    group_u = text[text.index("(U) Extent, channelLock"):]
    for phrase in ("(1/16) (x - s_c.x)^2 + 4 (y - s_c.y)^2 + 32 (z - s_c.z)^2", "c_j = (2 j - 19) / 19, j = 0 .. 19",
                   "10^(-5.0625 (u^4 - 1))", "maxDistance + 1e-10", "min d + 1e-10", "(|z|, z, -y, |x|, x)",
                   "6 - 8 (s_eff - 0.5)", "min(s_max / 0.2, 1)", "max(size_k, 0.1)", "WITHOUT A REFERENCE IMPLEMENTATION",
                   "THIS PROJECT'S READING"):
        assert phrase in group_u, phrase
    core = open(os.path.join(ROOT, "libear_amd", "csrc", "allo_objects.h")).read()
    for phrase in ("kGrid = 20", "kLockX = 1.0 / 16.0, kLockY = 4.0, kLockZ = 32.0", "kLockTol = 1e-10", "kFallOff = 5.0625",
                   "kMinHalfWidth = 0.1", "kFullExtent = 0.2", "6.0 - 8.0 * (s_eff - 0.5)"):
        assert phrase in core, phrase
    lib = capi.load()
    for name in ("earhip_allo_lock_priority", "earhip_allo_calculate_objects", "earhip_allo_calculate_objects_device"):
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert hasattr(lib, name), name
    assert callable(capi.allo_calculate_objects_device) and callable(capi.Allo.calculate_objects)
    hpp = open(os.path.join(ROOT, "libear_amd", "host", "ear", "hip_allo_objects.hpp")).read()
    assert "class AllocentricObjectsGainCalculator" in hpp


def test_core_alone_under_asan_and_ubsan(tmp_path):
    """libear_amd/csrc/allo_objects.h compiled by g++ without HIP, as a program of its own under ASan + UBSan
    (tests/cpp/test_allo_objects_core.cpp): the factorised core against the triple sum it never forms, 2 and 32 channels"""
    exe = tmp_path / "test_allo_objects_core"
    src = os.path.join(ROOT, "tests", "cpp", "test_allo_objects_core.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-I", os.path.join(ROOT, "libear_amd", "csrc"), src,
                    "-o", str(exe)], check=True)  # (the runtime linked in: the program needs nothing from its environment)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0 and re.search(r"^\d+ checked, 0 failed$", res.stdout, flags=re.M), res.stdout
