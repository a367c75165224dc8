"""The Ambisonic encoder's host forms (include/earhip.h group Q), without a device: the model of tests/hoa_encode_model.py and
earhip_hoa_encode against libear's own hoa::sph_harm, known answers, the addition theorem (independent of any model), the
rotation matrix's defining property, the refusals and the bindings."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
from scipy.special import eval_legendre

import _oracle
import hoa_encode_model as M
from libear_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS = (("N3D", 7), ("SN3D", 7), ("FuMa", 3))


def positions():
    """200 seeded positions, then the poles and the azimuths where a harmonic's factors are exact or the reduction matters"""
    rng = np.random.default_rng(2051)
    az = list(rng.uniform(-180.0, 180.0, 200))
    el = list(np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, 200))))
    for a in (0.0, 90.0, -90.0, 180.0, -180.0, 360.0, 1e6):
        for e in (0.0, 90.0, -90.0, 37.5):
            az.append(a)
            el.append(e)
    return np.array(az), np.array(el)


@pytest.fixture(scope="module")
def reference():
    """libear's sph_harm at the positions, per norm: float64 [n][n_coef] in ACN order, computed once.  The azimuth it is
    given is the exactly reduced one in radians: fmod(az, 360) * pi / 180."""
    az, el = positions()
    r, e = np.fmod(az, 360.0) * (math.pi / 180.0), el * (math.pi / 180.0)
    ref = {}
    for norm, order in NORMS:
        o, d = M.acn(order)
        ref[norm] = np.array([[_oracle.sph_harm(n, m, a, b, norm) for n, m in zip(o, d)] for a, b in zip(r, e)])
    return az, el, ref


@pytest.mark.parametrize("norm,order", NORMS)
def test_model_matches_libear_sph_harm(reference, norm, order):
    az, el, ref = reference
    o, d = M.acn(order)
    got = M.encode64(o, d, az, el, None, norm)
    want = ref[norm]
    err = np.abs(got - want)
    print(f"{norm}: worst |model - sph_harm| = {err.max():.3e}, worst relative {np.max(err / np.maximum(np.abs(want), 1e-300)):.3e}")
    assert np.all(err <= 1e-12 * np.abs(want) + 1e-13)


@pytest.mark.parametrize("norm,order", NORMS)
@pytest.mark.parametrize("with_gain", [False, True])
def test_host_form_is_within_one_float32_spacing_of_libear(reference, norm, order, with_gain):
    az, el, ref = reference
    o, d = M.acn(order)
    gain = np.random.default_rng(5).uniform(0.05, 2.0, az.size) if with_gain else None
    got = capi.hoa_encode(o, d, az, el, gain, norm)
    assert got.dtype == np.float32 and got.shape == (az.size, len(o))
    want = ref[norm] * (gain[:, None] if with_gain else 1.0)
    ok, worst = M.within_one_spacing(got, want)
    same = np.mean(got == want.astype(np.float32))
    print(f"{norm} gain={with_gain}: worst error {worst:.3f} spacings, {100 * same:.2f}% bit-identical to float32(sph_harm * gain)")
    assert ok, worst
    # and against the model
    ok, worst = M.within_one_spacing(got, M.encode64(o, d, az, el, gain, norm))
    assert ok, worst


def test_known_answers():
    for norm, w in (("N3D", 1.0), ("SN3D", 1.0), ("FuMa", 1 / math.sqrt(2))):
        got = capi.hoa_encode([0], [0], [12.0, -170.0], [33.0, -80.0], [1.0, 0.5], norm)
        assert got[0, 0] == np.float32(w) and got[1, 0] == np.float32(0.5 * w)
    o, d = M.acn(1)
    got = capi.hoa_encode(o, d, [90.0], [0.0], None, "N3D")[0].astype(np.float64)
    floor = 2.0 ** -43
    assert got[0] == 1.0
    assert abs(got[1] - math.sqrt(3.0)) <= np.spacing(np.float32(math.sqrt(3.0)))  # Y_1^-1: left
    assert abs(got[2]) <= floor and abs(got[3]) <= floor                           # Y_1^0 (up), Y_1^1 (front)
    # FuMa W X Y Z, a permuted list and a repeated channel
    src = dict(az=[30.0], el=[20.0])
    wxyz = capi.hoa_encode(*M.FUMA_WXYZ, src["az"], src["el"], None, "FuMa")[0]
    x, y, z = M.cart(30.0, 20.0)[[1, 0, 2]] * np.array([1.0, -1.0, 1.0])  # X front, Y left, Z up
    want = np.array([1 / math.sqrt(2), x, y, z])
    assert np.all(np.abs(wxyz - want) <= np.spacing(np.float32(1.0)))
    perm = [3, 0, 2, 0, 1]
    got = capi.hoa_encode([M.FUMA_WXYZ[0][k] for k in perm], [M.FUMA_WXYZ[1][k] for k in perm], src["az"], src["el"], None,
                          "FuMa")[0]
    assert np.array_equal(got, wxyz[perm])
    assert capi.hoa_acn(2)[0].tolist() == M.acn(2)[0] and capi.hoa_acn(2)[1].tolist() == M.acn(2)[1]
    o7, d7 = capi.hoa_acn(7)
    assert len(o7) == 64 and all(n == math.isqrt(k) and m == k - n * n - n for k, (n, m) in enumerate(zip(o7, d7)))


def test_addition_theorem():
    """sum_m Y_nm(a) Y_nm(b) = (2n + 1) P_n(cos gamma) in N3D: no model involved.  Each float32 factor may be one ulp off
    (2^-23 relative) and sum |a b| <= 2n + 1 by Cauchy-Schwarz: the bar is (2n + 1) 2^-22."""
    rng = np.random.default_rng(77)
    az = rng.uniform(-180.0, 180.0, (2, 500))
    el = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, (2, 500))))
    o, d = M.acn(7)
    a = capi.hoa_encode(o, d, az[0], el[0], None, "N3D").astype(np.float64)
    b = capi.hoa_encode(o, d, az[1], el[1], None, "N3D").astype(np.float64)
    cosg = np.clip(np.sum(M.cart(az[0], el[0]) * M.cart(az[1], el[1]), axis=1), -1.0, 1.0)
    o = np.array(o)
    for n in range(8):
        got = np.sum(a[:, o == n] * b[:, o == n], axis=1)
        want = (2 * n + 1) * eval_legendre(n, cosg)
        worst = np.max(np.abs(got - want)) / ((2 * n + 1) * 2.0 ** -22)
        print(f"order {n}: worst error {worst:.3f} of the bar")
        assert worst <= 1.0


def rotations():
    rng = np.random.default_rng(360)
    return [M.random_rotation(rng) for _ in range(3)] + [M.yaw(90.0)]


@pytest.mark.parametrize("norm", ["N3D", "SN3D"])
def test_rotation_matrix_turns_the_encoded_scene(norm):
    o, d = M.acn(7)
    rng = np.random.default_rng(1000)
    az = rng.uniform(-180.0, 180.0, 1000)
    el = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, 1000)))
    e = capi.hoa_encode(o, d, az, el, None, norm).astype(np.float64)
    oo = np.array(o)
    for k, q in enumerate(rotations()):
        R = capi.hoa_rotation_matrix(o, d, q, norm)
        assert R.dtype == np.float32 and R.shape == (64, 64)
        assert np.all(R[oo[:, None] != oo[None, :]] == 0.0)
        if k == 3:  # a pure yaw of 90 degrees: the closed form
            az2, el2 = az + 90.0, el
        else:
            az2, el2 = M.polar(M.cart(az, el) @ q.T)
        want = capi.hoa_encode(o, d, az2, el2, None, norm).astype(np.float64)
        R64 = R.astype(np.float64)
        got = e @ R64.T
        bar = 2.0 ** -22 * (np.abs(e) @ np.abs(R64).T) + 2.0 ** -23 * np.abs(want) + 1e-10
        worst = np.max(np.abs(got - want) / bar)
        print(f"{norm} rotation {k}: worst error {worst:.3f} of the bar")
        assert worst <= 1.0


@pytest.mark.parametrize("norm", ["N3D", "SN3D"])
def test_rotation_matrix_identity_and_composition(norm):
    o, d = M.acn(7)
    ident = capi.hoa_rotation_matrix(o, d, np.eye(3), norm).astype(np.float64)
    assert np.max(np.abs(ident - np.eye(64))) <= 2.0 ** -23
    q1, q2 = rotations()[:2]
    r1, r2, r12 = (capi.hoa_rotation_matrix(o, d, q, norm).astype(np.float64) for q in (q1, q2, q1 @ q2))
    # each entry of r1, r2 and r12 is within 2^-24 relative + 2.4e-11 of the exact matrix: the same form of bound as above
    bar = 2.0 ** -22 * (np.abs(r1) @ np.abs(r2)) + 2.0 ** -23 * np.abs(r12) + 1e-10
    worst = np.max(np.abs(r1 @ r2 - r12) / bar)
    print(f"{norm}: R(q1 q2) vs R(q1) R(q2): worst error {worst:.3f} of the bar")
    assert worst <= 1.0


def test_refusals():
    lib = capi.load()
    ip, dp, fp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float)
    az = np.array([10.0, 20.0, 30.0])
    el = np.zeros(3)
    with pytest.raises(capi.InvalidArgument):
        capi.hoa_encode([], [], az, el)
    with pytest.raises(capi.InvalidArgument):
        capi.hoa_encode([0] * 65, [0] * 65, az, el)
    with pytest.raises(capi.InvalidArgument):
        capi.hoa_encode([8], [0], az, el)
    with pytest.raises(capi.InvalidArgument):
        capi.hoa_encode([1], [2], az, el)
    with pytest.raises(capi.InvalidArgument):
        capi.hoa_encode([1], [-2], az, el)
    with pytest.raises(capi.InvalidArgument):
        capi.hoa_encode([4], [0], az, el, None, "FuMa")
    with pytest.raises(capi.AdmError) as e:
        capi.hoa_encode([0], [0], az, el, None, "foo")
    assert "unknown normalization type: 'foo'" in str(e.value)
    with pytest.raises(capi.AdmError):
        capi.hoa_rotation_matrix([0], [0], np.eye(3), "foo")
    with pytest.raises(capi.InvalidArgument):
        capi.hoa_acn(8)
    with pytest.raises(capi.InvalidArgument):
        capi.hoa_acn(-1)
    # NULL pointers, through the C ABI itself
    one = np.array([0], np.int32)
    out = np.zeros(4, np.float32)
    norm = b"SN3D"
    args = (C.c_size_t(3), az.ctypes.data_as(dp), el.ctypes.data_as(dp), None, out.ctypes.data_as(fp))
    assert lib.earhip_hoa_encode(1, None, one.ctypes.data_as(ip), norm, *args) == capi.INVALID_ARGUMENT
    assert lib.earhip_hoa_encode(1, one.ctypes.data_as(ip), None, norm, *args) == capi.INVALID_ARGUMENT
    assert lib.earhip_hoa_encode(1, one.ctypes.data_as(ip), one.ctypes.data_as(ip), None, *args) == capi.INVALID_ARGUMENT
    assert lib.earhip_hoa_encode(1, one.ctypes.data_as(ip), one.ctypes.data_as(ip), norm, C.c_size_t(3), None,
                                 el.ctypes.data_as(dp), None, out.ctypes.data_as(fp)) == capi.INVALID_ARGUMENT
    assert lib.earhip_hoa_encode(1, one.ctypes.data_as(ip), one.ctypes.data_as(ip), norm, C.c_size_t(3),
                                 az.ctypes.data_as(dp), el.ctypes.data_as(dp), None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_hoa_acn(1, None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_hoa_rotation_matrix(1, one.ctypes.data_as(ip), one.ctypes.data_as(ip), norm, None,
                                          out.ctypes.data_as(fp)) == capi.INVALID_ARGUMENT
    assert lib.earhip_hoa_encode_device(None, 1, one.ctypes.data_as(ip), one.ctypes.data_as(ip), norm, C.c_size_t(0), None,
                                        None, None, None, None) == capi.INVALID_ARGUMENT
    # a bad element is named by its index; the rows before it are written
    for bad, where in ((float("nan"), "az"), (float("inf"), "az"), (90.0000001, "el"), (-91.0, "el"), (float("-inf"), "el"),
                       (float("nan"), "gain"), (float("inf"), "gain")):
        a, b, g = az.copy(), el.copy(), np.ones(3)
        {"az": a, "el": b, "gain": g}[where][2] = bad
        with pytest.raises(capi.InvalidArgument) as e:
            capi.hoa_encode([0, 1], [0, 1], a, b, g)
        assert "element 2" in str(e.value), str(e.value)
    # q: determinant -1, a scaled row, a non-finite entry
    o, d = M.acn(1)
    for q in (np.diag([1.0, 1.0, -1.0]), np.diag([1.0, 1.0 + 1e-6, 1.0]), np.diag([1.0, float("nan"), 1.0])):
        with pytest.raises(capi.InvalidArgument):
            capi.hoa_rotation_matrix(o, d, q)
    capi.hoa_rotation_matrix(o, d, np.eye(3) + 1e-11)  # within the tolerance


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    lib = capi.load()
    for name in ("earhip_hoa_acn", "earhip_hoa_encode", "earhip_hoa_encode_device", "earhip_hoa_rotation_matrix"):
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert hasattr(lib, name), name
    for name in ("hoa_acn", "hoa_encode", "hoa_encode_device", "hoa_rotation_matrix"):
        assert callable(getattr(capi, name))
    hpp = open(os.path.join(ROOT, "libear_amd", "host", "ear", "hip_hoa.hpp")).read()
    assert "class HOAEncoder" in hpp


def test_position_walk_equals_the_single_channel_form_bit_for_bit(tmp_path):
    """libear_amd/csrc/hoa_encode.h on the host, under ASan + UBSan: encode_position (what the host form and the kernel run) gives
    every channel of any list once, with the bits of encode_one / legendre_nm for that channel alone (tests/cpp/test_hoa_core.cpp)"""
    import subprocess
    exe = tmp_path / "test_hoa_core"
    src = os.path.join(ROOT, "tests", "cpp", "test_hoa_core.cpp")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "libear_amd", "csrc"),
                    src, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0 and re.search(r"^\d+ checked, 0 failed$", res.stdout, flags=re.M), res.stdout
