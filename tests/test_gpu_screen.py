"""The device form of include/earhip.h group R (screenRef scaling and screenEdgeLock) on the GPU.  The per-element arithmetic
is an exact fmod, comparisons, one subtraction and one explicit fma (libear_amd/csrc/screen.h, shared with the host form), so
the device form is held to the host form's BITS: float64 bit patterns are compared, NaN positions included.  Then the stage in
front of the Objects gain producer, in place on the arrays the panner reads, alone and after the Cartesian conversion."""
import numpy as np
import pytest

import screen_model as M
from _hip import ctx
from test_screen_cpu import bits, c_screen

pytestmark = pytest.mark.gpu

GUARD = 64  # elements past n that must stay untouched


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_device(n, az, el, rep, ref_screen=None, screen_ref=None, lock_h=None, lock_v=None, with_status=True, in_place=False):
    """the device form over the first n elements of guarded buffers -> az_out, el_out (whole buffers), status or None"""
    import torch
    from libear_amd import capi
    pad = np.full(GUARD, -7777.0)
    t_az, t_el = _dev(np.concatenate([az, pad])), _dev(np.concatenate([el, pad]))
    if in_place:
        o_az, o_el = t_az, t_el
    else:
        o_az, o_el = _dev(np.full(n + GUARD, -7777.0)), _dev(np.full(n + GUARD, -7777.0))
    flags = [None if v is None else _dev(np.concatenate([v, np.full(GUARD, 1, np.uint8)])) for v in (screen_ref, lock_h, lock_v)]
    status = torch.full((n + GUARD,), -5, dtype=torch.int32, device="cuda") if with_status else None
    torch.cuda.synchronize()
    capi.screen_apply_device(ctx(), n, t_az, t_el, o_az, o_el, rep, ref_screen, *flags, status=status)
    ctx().synchronize()
    return o_az.cpu().numpy(), o_el.cpu().numpy(), None if status is None else status.cpu().numpy()


def assert_guard(n, *arrays):
    for a in arrays:
        assert (a[n:] == -7777.0).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_device_form_equals_the_host_form_bit_for_bit(n):
    from libear_amd import capi
    az, el, ref, lh, lv, _ = M.mixed_batch(n, seed=1000 + n)
    variants = 0
    for k, (r, p) in enumerate(((None, M.SCREEN_30), (M.CART, M.POLAR_15), (M.OTHERS[0], M.OTHERS[2]), (M.POLAR_15, None))):
        rs, ps = c_screen(r), c_screen(p)
        # every NULL optional array, status NULL and given, in place and out of place: rotated over the screen pairs so that
        # each size sees each of them
        for j, (f_ref, f_lh, f_lv) in enumerate(((ref, lh, lv), (None, lh, lv), (ref, None, lv), (ref, lh, None),
                                                 (None, None, None))):
            # with screen_ref NULL every element is scaled: the batch's untouched oddities would be refused
            a, e = (az, el) if f_ref is not None else (np.nan_to_num(az, nan=12.0), np.clip(el, -90.0, 90.0))
            want = capi.screen_apply(a, e, ps, rs, f_ref, f_lh, f_lv)
            with_status, in_place = bool((k + j) & 1), bool((k + j) & 2)
            g_az, g_el, status = run_device(n, a, e, ps, rs, f_ref, f_lh, f_lv, with_status, in_place)
            assert np.array_equal(bits(g_az[:n]), bits(want[0])), (k, j, np.flatnonzero(bits(g_az[:n]) != bits(want[0]))[:4])
            assert np.array_equal(bits(g_el[:n]), bits(want[1])), (k, j, np.flatnonzero(bits(g_el[:n]) != bits(want[1]))[:4])
            assert_guard(n, g_az, g_el)
            if with_status:
                assert (status[:n] == 0).all() and (status[n:] == -5).all()
            variants += 1
    assert variants == 20


def test_invalid_elements_get_nan_and_status_1():
    from libear_amd import capi
    n = 1500
    az, el, ref, lh, lv, bad = M.mixed_batch(n, seed=99, invalid=True)
    assert bad.sum() >= 12
    rep = c_screen(M.SCREEN_30)
    for in_place in (False, True):
        g_az, g_el, status = run_device(n, az, el, rep, None, ref, lh, lv, True, in_place)
        assert np.array_equal(status[:n], bad.astype(np.int32)) and (status[n:] == -5).all()
        assert np.isnan(g_az[:n][bad]).all() and np.isnan(g_el[:n][bad]).all()
        assert_guard(n, g_az, g_el)
        # the others: the host form's bits (the host form stops at a refused element, so it sees them without it)
        ok = ~bad
        want = capi.screen_apply(az[ok], el[ok], rep, None, ref[ok], lh[ok], lv[ok])
        assert np.array_equal(bits(g_az[:n][ok]), bits(want[0])) and np.array_equal(bits(g_el[:n][ok]), bits(want[1]))
    # and each refused element is one the host form refuses, by its index (behind the accepted elements before it)
    for i in np.flatnonzero(bad)[:6]:
        idx = np.append(np.flatnonzero(~bad[:i]), i)
        with pytest.raises(capi.InvalidArgument) as e:
            capi.screen_apply(az[idx], el[idx], rep, None, ref[idx], lh[idx], lv[idx])
        assert f"element {idx.size - 1}:" in str(e.value)


def test_no_elements_launch_nothing():
    from libear_amd import capi
    g_az, g_el, status = run_device(0, np.zeros(0), np.zeros(0), c_screen(M.SCREEN_30))
    assert_guard(0, g_az, g_el)
    assert (status == -5).all()
    capi.screen_apply_device(ctx(), 0, None, None, None, None, c_screen(M.SCREEN_30))  # no arrays needed
    ctx().synchronize()
    with pytest.raises(capi.InvalidArgument):  # a refused screen is refused by the device form too
        capi.screen_apply_device(ctx(), 0, None, None, None, None, capi.Screen.polar(1.78, 170.0, 0.0, 1.0, 58.0))


def _pan_device(p, n, t_az, t_el, extra=None):
    import torch
    direct = torch.empty((n, p.n_out), dtype=torch.float32, device="cuda")
    diffuse = torch.empty_like(direct)
    p.calculate_objects_device(n, t_az.data_ptr(), t_el.data_ptr(), extra.data_ptr() if extra is not None else None, None, None,
                               direct.data_ptr(), diffuse.data_ptr())
    assert p.missed() == 0  # synchronises
    return direct.cpu().numpy(), diffuse.cpu().numpy()


def test_end_to_end_in_front_of_the_objects_producer():
    """0+5+0: an object at the reference screen's left edge (29, 0) with screenRef lands on the 30 degree reproduction screen's
    left edge, 15 degrees, half way between M+000 and M+030: both gains sqrt(1/2) = 0.70711 (0.7071068; the bar of 2e-6 is the
    one the producer's known-answer tests use, taken about the value itself, which its five-digit rounding misses by 3.2e-6)."""
    import torch
    from libear_amd import capi
    layout = "0+5+0"
    names = [c[0] for c in capi.layout_channels(layout)]
    n = 257
    _, _, ref, lh, lv, _ = M.mixed_batch(n, seed=31)
    rng = np.random.default_rng(31)
    az, el = rng.uniform(-180.0, 180.0, n), rng.uniform(-90.0, 90.0, n)  # (what the panner takes, flagged or not)
    az[0], el[0], ref[0], lh[0], lv[0] = 29.0, 0.0, 1, 0, 0
    rep = c_screen(M.SCREEN_30)
    p = capi.Panner(ctx(), layout)
    t_az, t_el = _dev(az), _dev(el)
    torch.cuda.synchronize()
    capi.screen_apply_device(ctx(), n, t_az, t_el, t_az, t_el, rep, None, _dev(ref), _dev(lh), _dev(lv))
    d, f = _pan_device(p, n, t_az, t_el)
    print("object at (29, 0):", dict(zip(names, d[0].tolist())))
    for i, name in enumerate(names):
        want = np.sqrt(0.5) if name in ("M+000", "M+030") else 0.0
        assert abs(d[0, i] - want) <= 2e-6, (name, d[0, i])
    assert (f[0] == 0.0).all()
    # the whole batch: the producer on the host-scaled positions, bit for bit
    h_az, h_el = capi.screen_apply(az, el, rep, None, ref, lh, lv)
    assert np.array_equal(bits(t_az.cpu().numpy()), bits(h_az)) and np.array_equal(bits(t_el.cpu().numpy()), bits(h_el))
    w_az, w_el = _dev(h_az), _dev(h_el)
    torch.cuda.synchronize()
    wd, wf = _pan_device(p, n, w_az, w_el)
    p.close()
    assert np.array_equal(d.view(np.uint32), wd.view(np.uint32)) and np.array_equal(f.view(np.uint32), wf.view(np.uint32))


def test_chain_conversion_screen_producer():
    """257 Cartesian positions: to_polar_device, screen_apply_device, calculate_objects_device, three launches on one stream in
    place; against the host forms of the first two feeding the same panner call"""
    import torch
    from libear_amd import capi
    n = 257
    rng = np.random.default_rng(257)
    x, y, z = (rng.uniform(-1.0, 1.0, n) for _ in range(3))
    x[:3], y[:3], z[:3] = [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]
    ref = (rng.uniform(0, 1, n) < 0.7).astype(np.uint8)
    lh, lv = rng.choice([0, 0, 1, 2], n).astype(np.uint8), rng.choice([0, 0, 1, 2], n).astype(np.uint8)
    rs, ps = c_screen(M.CART), c_screen(M.POLAR_15)
    p = capi.Panner(ctx(), "4+5+0")
    t = [_dev(a) for a in (x, y, z)]
    torch.cuda.synchronize()
    capi.to_polar_device(ctx(), n, t[0], t[1], t[2], t[0], t[1], t[2])
    capi.screen_apply_device(ctx(), n, t[0], t[1], t[0], t[1], ps, rs, _dev(ref), _dev(lh), _dev(lv))
    d, f = _pan_device(p, n, t[0], t[1], t[2])
    h_az, h_el, h_dist = capi.to_polar(x, y, z)
    h_az, h_el = capi.screen_apply(h_az, h_el, ps, rs, ref, lh, lv)
    # (the conversion's device form is within a few float64 ulps of its host form, tests/test_gpu_conversion.py; the screen
    # stage adds nothing to that, and the float32 gains are held to the host chain's bits)
    assert np.max(np.abs(t[0].cpu().numpy() - h_az)) <= 1e-9 and np.max(np.abs(t[1].cpu().numpy() - h_el)) <= 1e-9
    w = [_dev(a) for a in (h_az, h_el, h_dist)]
    torch.cuda.synchronize()
    wd, wf = _pan_device(p, n, w[0], w[1], w[2])
    p.close()
    assert np.array_equal(d.view(np.uint32), wd.view(np.uint32)) and np.array_equal(f.view(np.uint32), wf.view(np.uint32))
