"""The device form of the Ambisonic encoder (earhip_hoa_encode_device, include/earhip.h group Q) on the GPU: against the
float64 model at the tile's edges (n = 1, 63, 64, 65, 4099) and channel counts that do not divide 64, repeatability, bad
elements, the bounds of what it writes, and its rows as the curves of a direct-only renderer (an Ambisonics bus).

Device and host run one core (libear_amd/csrc/hoa_encode.h) and differ only in the math library, so the bar is the host
form's: one float32 spacing at max(|want|, 2^-20) against float32 of the float64 reference (tests/hoa_encode_model.py, which
test_hoa_encode_cpu.py holds to libear's sph_harm within 1e-12)."""
import numpy as np
import pytest

import hoa_encode_model as M
import scenes
from _hip import ctx

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 4099)
SKIP_ONE = ([n for k, n in enumerate(M.acn(3)[0]) if k != 6], [m for k, m in enumerate(M.acn(3)[1]) if k != 6])
LISTS = {"one": ([2], [-1]), "acn1": M.acn(1), "acn3": M.acn(3), "skip15": SKIP_ONE, "fuma_wxyz": M.FUMA_WXYZ, "acn7": M.acn(7)}
NORM = {"fuma_wxyz": "FuMa", "acn7": "N3D"}


def positions(n, seed=9):
    rng = np.random.default_rng(seed)
    az = rng.uniform(-180.0, 180.0, n)
    el = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n)))
    special = [(0.0, 0.0), (90.0, 0.0), (-90.0, 0.0), (180.0, 0.0), (-180.0, 0.0), (360.0, 10.0), (1e6, -20.0), (30.0, 90.0),
               (-75.0, -90.0), (720.5, 45.0)]
    for k, (a, e) in enumerate(special[:max(0, n - 1)]):
        az[-1 - k], el[-1 - k] = a, e
    return az, el, rng.uniform(0.05, 2.0, n)


def _dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def encode_device(orders, degrees, az, el, gain, norm, status=False, guard=0):
    """-> (out [n][n_coef] float32, status or None, the guards' contents)"""
    import torch
    from libear_amd import capi
    n, nc = len(az), len(orders)
    out = torch.full((n * nc + 2 * guard,), 12345.0, dtype=torch.float32, device="cuda")
    st = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device="cuda") if status else None
    ins = [_dev(az), _dev(el), None if gain is None else _dev(gain)]
    torch.cuda.synchronize()
    capi.hoa_encode_device(ctx(), n, *ins, out.data_ptr() + 4 * guard, orders, degrees, norm,
                           status=None if st is None else st.data_ptr() + 4 * guard)
    ctx().synchronize()
    o = out.cpu().numpy()
    s = None if st is None else st.cpu().numpy()
    guards = (o[:guard], o[guard + n * nc:], None if s is None else s[:guard], None if s is None else s[guard + n:])
    return o[guard:guard + n * nc].reshape(n, nc), None if s is None else s[guard:guard + n], guards


@pytest.mark.parametrize("with_gain", [False, True])
@pytest.mark.parametrize("name", list(LISTS))
def test_device_form_against_the_float64_reference(name, with_gain):
    from libear_amd import capi
    o, d = LISTS[name]
    norm = NORM.get(name, "SN3D")
    for n in SIZES:
        az, el, gain = positions(n)
        g = gain if with_gain else None
        got, st, _ = encode_device(o, d, az, el, g, norm, status=True)
        want = M.encode64(o, d, az, el, g, norm)
        ok, worst = M.within_one_spacing(got, want)
        host = capi.hoa_encode(o, d, az, el, g, norm)
        print(f"{name} n={n} gain={with_gain}: worst error {worst:.3f} spacings; bit-identical to float32(reference) "
              f"{100 * np.mean(got == want.astype(np.float32)):.2f}%, to the host form {100 * np.mean(got == host):.2f}%")
        assert ok, (n, worst)
        assert np.all(st == 0)


def test_the_same_call_twice_gives_the_same_bits():
    o, d = M.acn(7)
    az, el, gain = positions(4099, seed=10)
    a, _, _ = encode_device(o, d, az, el, gain, "N3D")
    b, _, _ = encode_device(o, d, az, el, gain, "N3D")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bad_elements_get_nan_rows_and_status_1_and_disturb_nothing():
    o, d = SKIP_ONE
    n = 130
    az, el, gain = positions(n, seed=11)
    clean, st0, _ = encode_device(o, d, az, el, gain, "SN3D", status=True)
    assert np.all(st0 == 0) and np.all(np.isfinite(clean))
    bad = {0: ("az", np.nan), 63: ("az", np.inf), 64: ("az", -np.inf), 77: ("el", 90.0000001), 128: ("gain", np.nan),
           129: ("el", np.inf)}
    az2, el2, gain2 = az.copy(), el.copy(), gain.copy()
    for i, (where, v) in bad.items():
        {"az": az2, "el": el2, "gain": gain2}[where][i] = v
    got, st, _ = encode_device(o, d, az2, el2, gain2, "SN3D", status=True)
    is_bad = np.zeros(n, bool)
    is_bad[list(bad)] = True
    assert np.all(np.isnan(got[is_bad])) and np.array_equal(st, is_bad.astype(np.int32))
    assert np.array_equal(got[~is_bad].view(np.uint32), clean[~is_bad].view(np.uint32))
    again, none, _ = encode_device(o, d, az2, el2, gain2, "SN3D", status=False)  # status=None is accepted
    assert none is None and np.array_equal(again.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("name,n", [("acn7", 65), ("skip15", 63), ("one", 4099), ("acn1", 1)])
def test_nothing_is_written_outside_out_and_status(name, n):
    o, d = LISTS[name]
    az, el, gain = positions(n, seed=12)
    got, st, guards = encode_device(o, d, az, el, gain, NORM.get(name, "SN3D"), status=True, guard=64)
    assert np.all(np.isfinite(got)) and not np.any(got == 12345.0) and np.all(st == 0)
    assert np.all(guards[0] == 12345.0) and np.all(guards[1] == 12345.0)
    assert np.all(guards[2] == -7) and np.all(guards[3] == -7)


def test_empty_call_is_a_no_op():
    from libear_amd import capi
    capi.hoa_encode_device(ctx(), 0, None, None, None, None, [0], [0])
    ctx().synchronize()


def test_rows_as_the_curves_of_a_direct_only_renderer():
    """eight objects, three positions each at block boundaries, order 3 SN3D on a 16-channel bus: the renderer's output against
    a float64 evaluation of 'linear interpolation of the float32 gain rows times the input, summed over objects' — relative
    RMS 1e-6 per channel, the bar of the project's parity gate for this renderer"""
    from libear_amd import capi
    o, d = M.acn(3)
    n_obj, block, nblocks = 8, 64, 4
    az, el, gain = positions(3 * n_obj, seed=13)
    rows, _, _ = encode_device(o, d, az, el, gain, "SN3D")
    times = np.array([0, 2 * block, 3 * block], np.int64)
    curves = [(times, rows[3 * k:3 * k + 3].copy(), None) for k in range(n_obj)]
    x = scenes.audio(n_obj, block * nblocks)
    r = capi.Renderer(ctx(), n_obj, 16, block, None, 0, max_blocks=nblocks)
    for k, (t, g, _) in enumerate(curves):
        r.set_object_points(k, t, g)
    got = r.process(x)
    r.close()
    want = scenes.render_f64(curves, x, 16)
    err = scenes.rel_rms_per_channel(got, want)
    print(f"Ambisonics bus, order 3: worst channel relative RMS {err:.3e}")
    assert err <= 1e-6, err
