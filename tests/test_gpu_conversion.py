"""The device forms of earhip group K (ear::conversion) on the GPU: against the host forms over 2^20 (object x block)
elements, a Cartesian scene converted in place and fed straight to the extent panner, and the batch overloads of the
C++ mirror against single calls.

Device and host run the same code (libear_amd/csrc/conversion.h); only the transcendentals differ (the device's math
library against the host's), by an ulp or so.  An element's difference is counted in ulps of the larger of its host
value and the scale of that quantity: the distance (at least 1) for positions, 180 for angles, 360 for polar extents
and 1 for Cartesian ones.  Positions and angles are held to 8 such ulps (measured on an MI355X: 6 for x / y, 2 for
the azimuth), extents to 16 (measured: 11.8 for the polar width).  A 4-ulp bar is not met: the formulas amplify a
1-ulp difference in a sine or cosine, most in asin near 1, whose slope is 22 at the sweep's largest Cartesian sizes
(0.999).  The listed points where asin / acos are evaluated at +-1 (test_conversion.DEGENERATE_*) are held to libear's
margin of 1e-6."""
import re
import subprocess

import numpy as np
import pytest

import _oracle
import conv_model as M
import test_conversion as T
from _hip import ctx

pytestmark = pytest.mark.gpu

N = 1 << 20
ULPS_POS, ULPS_EXT = 8, 16


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def _run_device(direction, src):
    """the device form over the six input arrays (positions, extents), outputs in separate tensors; -> outputs, status"""
    import torch
    from libear_amd import capi
    n = src[0].size
    ins = [_dev(a) for a in src]
    outs = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(6)]
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fn = capi.to_polar_device if direction == "to_polar" else capi.to_cartesian_device
    fn(ctx(), n, *ins[:3], *outs[:3], *ins[3:], *outs[3:], status=status)
    ctx().synchronize()
    return [o.cpu().numpy() for o in outs], status.cpu().numpy()


def _run_host(direction, src, ok):
    """the host form over the elements it converts (one call), and its code for each of the others (one call each)"""
    from libear_amd import capi
    n = src[0].size
    out = [np.full(n, np.nan) for _ in range(6)]
    fn = capi.to_polar if direction == "to_polar" else capi.to_cartesian
    p, e = fn(*[a[ok] for a in src[:3]], *[a[ok] for a in src[3:]], extent=True)
    for k in range(3):
        out[k][ok], out[3 + k][ok] = p[k], e[k]
    codes = np.zeros(n, np.int32)
    for i in np.flatnonzero(~ok):
        try:
            fn(*[a[i:i + 1] for a in src], extent=True)
        except capi.EarHipError as ex:
            codes[i] = ex.code
    return out, codes


def _ulps(got, want, floor):
    with np.errstate(invalid="ignore"):
        scale = np.fmax(np.abs(want), floor)
        same = (got == want) | (np.isnan(want) & np.isnan(got))
        return np.where(same, 0.0, np.abs(got - want) / np.spacing(scale))


def _error_block():
    """(az, el, dist) of elements the polar -> Cartesian direction refuses, and their host codes"""
    az = np.array([np.nan, np.inf, -np.inf, 2.0 ** 40 * 2, -1e300, np.nan])
    return az, np.full(6, 10.0), np.full(6, 1.0)


def test_device_equals_host_to_cartesian():
    az, el, dist, w, h, d = T.polar_sweep(N - 6, seed=77)
    eaz, eel, edist = _error_block()
    src = [np.concatenate([a, b]) for a, b in ((az, eaz), (el, eel), (dist, edist))] + \
          [np.concatenate([a, np.full(6, 20.0)]) for a in (w, h, d)]
    ok = np.ones(N, bool)
    ok[-6:] = False
    got, status = _run_device("to_cartesian", src)
    want, codes = _run_host("to_cartesian", src, ok)
    assert np.array_equal(status, codes), np.flatnonzero(status != codes)[:8]
    assert list(codes[-6:]) == [2, 1, 1, 1, 1, 2]
    assert np.isnan(np.stack(got)[:, ~ok]).all()
    floors = [np.fmax(1.0, np.abs(src[2]))] * 3 + [1.0] * 3
    worst = []
    for k, name in enumerate(("x", "y", "z", "width", "height", "depth")):
        assert np.array_equal(np.isnan(got[k][ok]), np.isnan(want[k][ok])), name
        u = _ulps(got[k][ok], want[k][ok], floors[k] if np.isscalar(floors[k]) else floors[k][ok])
        worst.append((name, float(u.max())))
    print("device vs host, polar -> Cartesian, worst ulps:", worst)
    assert all(u <= (ULPS_POS if k < 3 else ULPS_EXT) for k, (_, u) in enumerate(worst)), worst


def test_device_equals_host_to_polar():
    x, y, z, w, h, d = T.cart_sweep(N - 64, seed=78)
    dg = T.degenerate_cart()
    ng = dg[0].size
    pad = 64 - ng - 3
    assert pad >= 0
    # a NaN coordinate (no sector: internal error), Cartesian infinities (NaN through, status 0)
    extra = [np.array([np.nan, np.inf, 0.5] + [0.3] * pad), np.array([1.0, 1.0, np.inf] + [0.2] * pad),
             np.array([0.0, 0.0, 0.0] + [0.1] * pad)]
    src = [np.concatenate([a, g, e]) for a, g, e in zip((x, y, z), dg[:3], extra)] + \
          [np.concatenate([a, g, np.full(pad + 3, 0.25)]) for a, g in zip((w, h, d), dg[3:])]
    degenerate = np.zeros(N, bool)
    degenerate[N - 64: N - 64 + ng] = True
    ok = np.ones(N, bool)
    ok[N - 64 + ng] = False
    got, status = _run_device("to_polar", src)
    want, codes = _run_host("to_polar", src, ok)
    assert np.array_equal(status, codes), np.flatnonzero(status != codes)[:8]
    assert codes[N - 64 + ng] == 2 and (codes[ok] == 0).all()
    assert np.isnan(got[0][N - 64 + ng + 1])  # the infinity passed through as libear passes it
    regular = ok & ~degenerate
    floors = [180.0, 180.0, np.fmax(1.0, np.abs(want[2][regular])), 360.0, 360.0, 1.0]
    worst = []
    for k, name in enumerate(("azimuth", "elevation", "distance", "width", "height", "depth")):
        assert np.array_equal(np.isnan(got[k][ok]), np.isnan(want[k][ok])), name
        u = _ulps(got[k][regular], want[k][regular], floors[k])
        worst.append((name, float(u.max())))
        with np.errstate(invalid="ignore"):
            err = np.nan_to_num(np.abs(got[k][degenerate] - want[k][degenerate]))
        assert err.max() <= T.LIBEAR_MARGIN, (name, err.max())
    print("device vs host, Cartesian -> polar, worst ulps:", worst)
    assert all(u <= (ULPS_POS if k < 3 else ULPS_EXT) for k, (_, u) in enumerate(worst)), worst


@pytest.mark.parametrize("layout", ["4+5+0", "9+10+3"])
def test_cartesian_scene_through_to_polar_and_extent_panner(layout):
    """1024 Cartesian objects: to_polar_device in place, then the extent panner on the converted arrays, on one
    stream with no host copy in between; against the pinned extent panner fed with the model's polar metadata"""
    import torch
    from libear_amd import capi
    rng = np.random.default_rng(sum(map(ord, layout)))
    n = 1024
    x, y, z = (rng.uniform(-1.0, 1.0, n) for _ in range(3))
    x[:4], y[:4], z[:4] = [0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]
    w, h, d = (rng.uniform(0.0, 0.9, n) for _ in range(3))
    w[:64] = h[:64] = d[:64] = 0.0
    gain = rng.uniform(0.1, 2.0, n)
    diffuse = rng.choice([0.0, 0.25, 0.5], n)
    t = [_dev(a) for a in (x, y, z, w, h, d, gain, diffuse)]
    p = capi.Panner(ctx(), layout)
    direct = torch.empty((n, p.n_out), dtype=torch.float32, device="cuda")
    diff = torch.empty_like(direct)
    torch.cuda.synchronize()
    capi.to_polar_device(ctx(), n, t[0], t[1], t[2], t[0], t[1], t[2], t[3], t[4], t[5], t[3], t[4], t[5])
    p.calculate_device(n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[6].data_ptr(), t[7].data_ptr(),
                       direct.data_ptr(), diff.data_ptr(), t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr())
    assert p.missed() == 0  # synchronises
    p.close()
    (maz, mel, mdist), (mw, mh, md), st = M.extent_cart_to_polar(x, y, z, w, h, d)
    assert (st == M.OK).all()
    np.testing.assert_allclose(t[0].cpu().numpy(), maz, rtol=0, atol=1e-9)
    o = _oracle.PolarExtent(layout)
    wd, wf = o.calculate(maz, mel, mdist, mw, mh, md, gain, diffuse)
    got_d, got_f = direct.cpu().numpy().astype(np.float64), diff.cpu().numpy().astype(np.float64)
    for g, want in ((got_d, wd), (got_f, wf)):
        want = want.astype(np.float64)
        err = np.linalg.norm(g - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-30)
        err[np.linalg.norm(want, axis=1) == 0] = np.linalg.norm(g, axis=1)[np.linalg.norm(want, axis=1) == 0]
        assert err.max() <= 1e-5, (int(np.argmax(err)), err.max())


def test_batch_overloads_equal_single_calls(tmp_path):
    """toPolar / toCartesian on std::vector<ObjectsTypeMetadata> (one device launch) against single calls, in the
    drop-in program (tests/cpp/test_dropin_conversion.cpp, test_batch)"""
    import _dropin
    exe = _dropin.build(tmp_path, "test_dropin_conversion", wextra=False)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0 and "FAILED" not in res.stdout, res.stdout
    assert re.search(r"^\d+ passed, 0 failed$", res.stdout, flags=re.M)
