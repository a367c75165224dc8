"""The device form of include/earhip.h group V (screenRef scaling and screenEdgeLock of Cartesian positions) on the GPU.  One
kernel does what earhip_conversion_to_polar_device, earhip_screen_apply_device and earhip_conversion_to_cartesian_device do in
three, from the same cores (libear_amd/csrc/screen_cart.h), so on every element with a flag set it is held to the BITS of those
three launches; on an element with no flag set to the bits of its INPUT, which the three launches cannot give.  Then the
independent model, the refusals, and the chain the stage exists for: in place in front of the allocentric panner."""
import numpy as np
import pytest

import screen_cart_cases as K
import screen_model as M
from _hip import ctx
from test_screen_cpu import bits, c_screen

pytestmark = pytest.mark.gpu

GUARD = 64  # elements past n that must stay untouched
FILL = -7777.0


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_device(n, pos, rep, ref_screen=None, screen_ref=None, lock_h=None, lock_v=None, with_status=True, in_place=False):
    """the device form over the first n elements of guarded buffers -> [x, y, z] (whole buffers), status or None"""
    import torch
    from libear_amd import capi
    pad = np.full(GUARD, FILL)
    t_in = [_dev(np.concatenate([a, pad])) for a in pos]
    t_out = t_in if in_place else [_dev(np.full(n + GUARD, FILL)) for _ in range(3)]
    flags = [None if v is None else _dev(np.concatenate([v, np.full(GUARD, 1, np.uint8)])) for v in (screen_ref, lock_h, lock_v)]
    status = torch.full((n + GUARD,), -5, dtype=torch.int32, device="cuda") if with_status else None
    torch.cuda.synchronize()
    capi.screen_apply_cartesian_device(ctx(), n, *t_in, *t_out, rep, ref_screen, *flags, status=status)
    ctx().synchronize()
    return [t.cpu().numpy() for t in t_out], None if status is None else status.cpu().numpy()


def run_chain(n, pos, rep, ref_screen, screen_ref, lock_h, lock_v):
    """the three launches the stage fuses, in place on copies of the same arrays -> x, y, z"""
    import torch
    from libear_amd import capi
    t = [_dev(a) for a in pos]
    flags = [None if v is None else _dev(v) for v in (screen_ref, lock_h, lock_v)]
    torch.cuda.synchronize()
    capi.to_polar_device(ctx(), n, *t, *t)
    capi.screen_apply_device(ctx(), n, t[0], t[1], t[0], t[1], rep, ref_screen, *flags)
    capi.to_cartesian_device(ctx(), n, *t, *t)
    ctx().synchronize()
    return [a.cpu().numpy() for a in t]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_device_form_has_the_bits_of_the_three_device_launches(n):
    x, y, z, ref, lh, lv, _ = K.batch(n, seed=3000 + n)
    variants = 0
    for k, (r, p) in enumerate(K.PAIRS):
        rs, ps = c_screen(r), c_screen(p)
        # every NULL optional array, status NULL and given, in place and out of place: rotated over the screen pairs so that
        # each size sees each of them
        for j, (f_ref, f_lh, f_lv) in enumerate(((ref, lh, lv), (None, lh, lv), (ref, None, lv), (ref, lh, None),
                                                 (None, None, None))):
            # with screen_ref NULL every element is scaled: the batch's untouched oddities would be refused
            pos = (x, y, z) if f_ref is not None else K.finite(x, y, z)
            with_status, in_place = bool((k + j) & 1), bool((k + j) & 2)
            got, status = run_device(n, pos, ps, rs, f_ref, f_lh, f_lv, with_status, in_place)
            f = K.flagged(n, f_ref, f_lh, f_lv)
            if p is None:  # no reproduction screen: every element is a copy
                f[:] = False
            want = run_chain(n, pos, ps, rs, f_ref, f_lh, f_lv)
            for g, w, a in zip(got, want, pos):
                assert np.array_equal(bits(g[:n][f]), bits(w[f])), (k, j, np.flatnonzero(bits(g[:n]) != bits(w))[:4])
                assert np.array_equal(bits(g[:n][~f]), bits(a[~f])), (k, j)
                assert (g[n:] == FILL).all()
            if with_status:
                assert (status[:n] == 0).all() and (status[n:] == -5).all()
            variants += 1
    assert variants == 20


def test_device_form_matches_the_model():
    from libear_amd import capi
    from test_gpu_conversion import _ulps
    n = 4099
    x, y, z, ref, lh, lv, _ = K.batch(n, seed=4242)
    worst = worst_ulps = 0.0
    for r, p in K.PAIRS:
        got, status = run_device(n, (x, y, z), c_screen(p), c_screen(r), ref, lh, lv)
        assert (status[:n] == 0).all()
        want = K.model(x, y, z, p, r, ref, lh, lv)
        host = capi.screen_apply_cartesian(x, y, z, c_screen(p), c_screen(r), ref, lh, lv)
        for g, w, h in zip(got, want, host):
            g = g[:n]
            assert np.array_equal(np.isnan(g), np.isnan(w))
            with np.errstate(invalid="ignore"):
                worst = max(worst, float(np.nanmax(np.where(bits(g) == bits(w), 0.0, np.abs(g - w)))))
                worst_ulps = max(worst_ulps, float(np.nanmax(np.where(bits(g) == bits(h), 0.0, _ulps(g, h, 1e-3)))))
    print(f"device form vs model: worst difference {worst:.3e}; vs the host form: {worst_ulps:.1f} ulps at max(|value|, 1e-3)")
    assert worst <= K.ATOL


def test_refused_elements_get_nan_and_status_1():
    n = 1500
    x, y, z, ref, lh, lv, bad = K.batch(n, seed=99, invalid=True)
    assert bad.sum() >= 12
    rep = c_screen(M.SCREEN_30)
    ok = ~bad
    plain = ~K.flagged(n, ref, lh, lv)
    odd = plain & ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
    assert odd.sum() >= 12 and not (odd & bad).any()
    # the accepted elements: the bits of a run without the refused ones
    want, _ = run_device(int(ok.sum()), [a[ok] for a in (x, y, z)], rep, None, ref[ok], lh[ok], lv[ok])
    for in_place in (False, True):
        got, status = run_device(n, (x, y, z), rep, None, ref, lh, lv, True, in_place)
        assert np.array_equal(status[:n], bad.astype(np.int32)) and (status[n:] == -5).all()
        for g, w, a in zip(got, want, (x, y, z)):
            assert np.isnan(g[:n][bad]).all() and (g[n:] == FILL).all()
            assert np.array_equal(bits(g[:n][ok]), bits(w[:int(ok.sum())]))
            # unflagged NaN and infinities come back as they went in
            assert np.array_equal(bits(g[:n][odd]), bits(a[odd]))


def test_no_elements_launch_nothing():
    from libear_amd import capi
    got, status = run_device(0, [np.zeros(0)] * 3, c_screen(M.SCREEN_30))
    assert all((g == FILL).all() for g in got) and (status == -5).all()
    capi.screen_apply_cartesian_device(ctx(), 0, None, None, None, None, None, None, c_screen(M.SCREEN_30))  # no arrays needed
    ctx().synchronize()
    with pytest.raises(capi.InvalidArgument):  # a refused screen is refused by the device form too
        capi.screen_apply_cartesian_device(ctx(), 0, None, None, None, None, None, None,
                                           capi.Screen.polar(1.78, 170.0, 0.0, 1.0, 58.0))


def _allo_device(allo, n, t):
    import torch
    from libear_amd import capi
    direct = torch.empty((n, allo.n_out), dtype=torch.float32, device="cuda")
    diffuse = torch.empty_like(direct)
    capi.allo_calculate_objects_device(ctx(), allo, n, *t, *[None] * 10, direct, diffuse)
    ctx().synchronize()
    return direct.cpu().numpy(), diffuse.cpu().numpy()


def test_in_place_in_front_of_the_allocentric_panner():
    """257 positions on 9+10+3, a third of them flagged: the stage in place, then earhip_allo_calculate_objects_device on the
    same arrays.  Against Allo.calculate_objects on the host form's output, at the bar tests/test_gpu_allo_objects.py holds
    device rows to host rows with (one float32 spacing at max(|want|, 2^-20)); the rows of unflagged elements have the bits
    of a run that never called the stage."""
    import torch
    import allo_model
    from libear_amd import capi
    n = 257
    rng = np.random.default_rng(257)
    x, y, z = (rng.uniform(-1.2, 1.2, n) for _ in range(3))
    x[:4], y[:4], z[:4] = [0.0, 1.0, -1.0, 0.0], [1.0, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]  # on loudspeakers, the centre
    flag = rng.uniform(0, 1, n) < 1.0 / 3.0
    flag[:4] = [True, False, False, False]
    combo = np.array(K.COMBOS)[rng.integers(0, len(K.COMBOS), n)]
    combo[~flag] = 0
    ref, lh, lv = (np.ascontiguousarray(combo[:, j], np.uint8) for j in range(3))
    rs, ps = c_screen(M.CART), c_screen(M.POLAR_15)
    allo = capi.Allo("9+10+3")
    t = [_dev(a) for a in (x, y, z)]
    untouched = [_dev(a) for a in (x, y, z)]
    torch.cuda.synchronize()
    capi.screen_apply_cartesian_device(ctx(), n, *t, *t, ps, rs, _dev(ref), _dev(lh), _dev(lv))
    d, f = _allo_device(allo, n, t)
    for a, b in zip(t, (x, y, z)):
        assert np.array_equal(bits(a.cpu().numpy()[~flag]), bits(b[~flag]))
    hx, hy, hz = capi.screen_apply_cartesian(x, y, z, ps, rs, ref, lh, lv)
    want_d, want_f = allo.calculate_objects(hx, hy, hz)
    for got, want in ((d, want_d), (f, want_f)):
        ok, worst = allo_model.within_one_spacing(got, want.astype(np.float64))
        assert ok, worst
    plain_d, plain_f = _allo_device(allo, n, untouched)
    allo.close()
    assert np.array_equal(d[~flag].view(np.uint32), plain_d[~flag].view(np.uint32))
    assert np.array_equal(f[~flag].view(np.uint32), plain_f[~flag].view(np.uint32))
    assert not np.array_equal(d[flag].view(np.uint32), plain_d[flag].view(np.uint32))  # (the stage did move the others)
