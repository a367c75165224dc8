"""The device form of the allocentric panner (earhip_allo_calculate_device, include/earhip.h group T) on the GPU: against the
float64 model at the tile's edges (n = 1, 63, 64, 65, 4099) on layouts of 2 to 32 channels, repeatability, bad elements, the
bounds of what it writes, and its rows as the curves of a direct-only renderer.

Device and host run one core (libear_amd/csrc/allo.h) and differ only in the math library, so the bar is the host form's: one
float32 spacing at max(|want|, 2^-20) against float32 of the float64 model (tests/allo_model.py)."""
import functools

import numpy as np
import pytest

import allo_model as M
import scenes
from _hip import ctx
from layouts import LAYOUTS

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 4099)
# 0+2+0: one row; 4+5+1: a plane of one loudspeaker; 3+7+0: two LFEs and a one-loudspeaker row; 9+10+3: 24 channels
NAMES = ("0+2+0", "0+5+0", "4+5+1", "3+7+0", "9+10+3", M.DOME32_NAME)


@functools.lru_cache(maxsize=None)
def handle(name):
    from libear_amd import capi
    if name != M.DOME32_NAME:
        return capi.Allo(name), M.Model(name)
    channels, pos = M.dome32()
    capi.define_layout(name, channels)
    return capi.Allo(name, pos), M.Model(positions=pos, lfe=[ch[3] for ch in channels])


@functools.lru_cache(maxsize=None)
def batch(name, seed=9):
    """4099 positions in [-1.3, 1.3]^3 with gains, diffuse values and masks, the special positions last; a batch of n
    elements is the LAST n of these"""
    rng = np.random.default_rng(seed)
    n = max(SIZES)
    pos = rng.uniform(-1.3, 1.3, (n, 3))
    pos[-len(M.SPECIAL):] = M.SPECIAL
    nch = handle(name)[1].n
    mask = (rng.integers(0, 1 << nch, n, dtype=np.uint64) & rng.integers(0, 1 << nch, n, dtype=np.uint64)).astype(np.uint32)
    mask[::5] = 0
    mask[2::40] = (1 << nch) - 1
    return pos, rng.uniform(0.05, 2.0, n), rng.uniform(0.0, 1.0, n), mask


@functools.lru_cache(maxsize=None)
def reference(name, full):
    """the model's float64 rows of the whole batch, computed once: with gain, diffuse and masks, or without all three"""
    pos, gain, diffuse, mask = batch(name)
    model = handle(name)[1]
    return model.calculate64(pos[:, 0], pos[:, 1], pos[:, 2], *((gain, diffuse, mask) if full else (None, None, None)))


def _dev(a, dtype=np.float64):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def run_device(allo, pos, gain=None, diffuse=None, mask=None, status=False, guard=0, diffuse_out=True):
    """-> (direct, diffuse_out or None [n][n_channels] float32, status or None, the guards' contents)"""
    import torch
    from libear_amd import capi
    n, nc = len(pos), allo.n_out
    outs = [torch.full((n * nc + 2 * guard,), 12345.0, dtype=torch.float32, device="cuda") for _ in range(2 if diffuse_out else 1)]
    st = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device="cuda") if status else None
    ins = [_dev(pos[:, 0]), _dev(pos[:, 1]), _dev(pos[:, 2]), _dev(gain), _dev(diffuse),
           None if mask is None else _dev(np.asarray(mask, np.uint32).view(np.int32), np.int32)]
    torch.cuda.synchronize()
    capi.allo_calculate_device(ctx(), allo, n, *ins, outs[0].data_ptr() + 4 * guard,
                               outs[1].data_ptr() + 4 * guard if diffuse_out else None,
                               status=None if st is None else st.data_ptr() + 4 * guard)
    ctx().synchronize()
    o = [t.cpu().numpy() for t in outs]
    s = None if st is None else st.cpu().numpy()
    guards = [g for a in o for g in (a[:guard], a[guard + n * nc:])]
    if s is not None:
        guards += [s[:guard], s[guard + n:]]
    rows = [a[guard:guard + n * nc].reshape(n, nc) for a in o]
    return rows[0], rows[1] if diffuse_out else None, None if s is None else s[guard:guard + n], guards


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_device_form_against_the_float64_model(name, full):
    allo, model = handle(name)
    pos, gain, diffuse, mask = batch(name)
    want_d, want_f = reference(name, full)
    lfe = np.array(model.lfe)
    for n in SIZES:
        args = (gain[-n:], diffuse[-n:], mask[-n:]) if full else (None, None, None)
        got_d, got_f, st, _ = run_device(allo, pos[-n:], *args, status=True)
        host_d, host_f = allo.calculate(pos[-n:, 0], pos[-n:, 1], pos[-n:, 2], *args)
        for what, got, want, host in (("direct", got_d, want_d[-n:], host_d), ("diffuse", got_f, want_f[-n:], host_f)):
            ok, worst = M.within_one_spacing(got, want)
            print(f"{name} n={n} full={full} {what}: worst error {worst:.3f} spacings; bit-identical to the host form "
                  f"{100 * np.mean(got.view(np.uint32) == host.view(np.uint32)):.2f}%")
            assert ok, (n, what, worst)
            assert np.all(got[:, lfe].view(np.uint32) == 0)
        assert np.all(st == 0)
        assert np.all(np.count_nonzero(got_d, axis=1) <= 8)


def test_the_same_call_twice_gives_the_same_bits():
    allo, _ = handle("9+10+3")
    pos, gain, diffuse, mask = batch("9+10+3")
    a = run_device(allo, pos, gain, diffuse, mask)
    b = run_device(allo, pos, gain, diffuse, mask)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_bad_elements_get_nan_rows_and_status_1_where_the_host_form_refuses():
    from libear_amd import capi
    allo, _ = handle("3+7+0")
    n = 130
    pos, gain, diffuse, mask = (v[-n:].copy() for v in batch("3+7+0"))
    clean_d, clean_f, st0, _ = run_device(allo, pos, gain, diffuse, mask, status=True)
    assert np.all(st0 == 0) and np.all(np.isfinite(clean_d)) and np.all(np.isfinite(clean_f))
    bad = {0: ("x", np.nan), 5: ("y", np.inf), 63: ("z", -np.inf), 64: ("gain", np.nan), 77: ("diffuse", 1.0000001),
           100: ("diffuse", -1e-9), 127: ("diffuse", np.nan), 128: ("gain", np.inf), 129: ("x", np.inf)}
    cols = {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "gain": gain, "diffuse": diffuse}
    for i, (where, v) in bad.items():
        cols[where][i] = v
    mask[10] |= 0xfffff000  # bits beyond the 12 channels: the device form ignores them (the host form refuses)
    refused = np.zeros(n, bool)
    for i in range(n):
        try:
            allo.calculate(*pos[i], gain[i], diffuse[i], mask[i] & 0xfff)
        except capi.InvalidArgument:
            refused[i] = True
    assert sorted(np.flatnonzero(refused)) == sorted(bad)
    got_d, got_f, st, _ = run_device(allo, pos, gain, diffuse, mask, status=True)
    assert np.all(np.isnan(got_d[refused])) and np.all(np.isnan(got_f[refused]))
    assert np.array_equal(st, refused.astype(np.int32))
    assert np.array_equal(got_d[~refused].view(np.uint32), clean_d[~refused].view(np.uint32))
    assert np.array_equal(got_f[~refused].view(np.uint32), clean_f[~refused].view(np.uint32))
    again = run_device(allo, pos, gain, diffuse, mask, status=False)  # status=None is accepted
    assert again[2] is None and np.array_equal(again[0].view(np.uint32), got_d.view(np.uint32))
    assert np.array_equal(again[1].view(np.uint32), got_f.view(np.uint32))


@pytest.mark.parametrize("name,n", [(M.DOME32_NAME, 65), ("3+7+0", 63), ("0+2+0", 4099), ("9+10+3", 1)])
def test_nothing_is_written_outside_the_outputs_and_status(name, n):
    allo, _ = handle(name)
    pos, gain, diffuse, mask = (v[-n:] for v in batch(name))
    got_d, got_f, st, guards = run_device(allo, pos, gain, diffuse, mask, status=True, guard=64)
    assert np.all(np.isfinite(got_d)) and np.all(np.isfinite(got_f)) and np.all(st == 0)
    assert not np.any(got_d == 12345.0) and not np.any(got_f == 12345.0)
    assert all(np.all(g == 12345.0) for g in guards[:4]) and all(np.all(g == -7) for g in guards[4:])


def test_diffuse_out_may_be_absent_when_diffuse_is():
    allo, _ = handle("0+5+0")
    pos, gain, _, mask = (v[-65:] for v in batch("0+5+0"))
    both = run_device(allo, pos, gain, None, mask)
    only, none, _, guards = run_device(allo, pos, gain, None, mask, guard=64, diffuse_out=False)
    assert none is None and np.array_equal(only.view(np.uint32), both[0].view(np.uint32))
    assert np.all(both[1].view(np.uint32) == 0) and all(np.all(g == 12345.0) for g in guards)


def test_empty_call_is_a_no_op():
    from libear_amd import capi
    capi.allo_calculate_device(ctx(), handle("0+5+0")[0], 0, None, None, None, None, None, None, None, None)
    ctx().synchronize()


def test_rows_as_the_curves_of_a_direct_only_renderer():
    """65 objects at fixed positions on 0+5+0, one 512-sample block: the renderer's output with the device form's rows as
    its curve points against a float64 evaluation of 'the model's gains times the input, summed over objects' — relative
    RMS 1e-6 per channel, the bar of the project's parity gate for this renderer"""
    from libear_amd import capi
    allo, _ = handle("0+5+0")
    n_obj, block = 65, 512
    pos, gain, _, mask = (v[-n_obj:] for v in batch("0+5+0"))
    rows, _, _, _ = run_device(allo, pos, gain, None, mask, diffuse_out=False)
    want_rows = handle("0+5+0")[1].calculate64(pos[:, 0], pos[:, 1], pos[:, 2], gain, None, mask)[0]
    times = np.array([0], np.int64)
    x = scenes.audio(n_obj, block)
    r = capi.Renderer(ctx(), n_obj, 6, block, None, 0, max_blocks=1)
    for k in range(n_obj):
        r.set_object_points(k, times, rows[k:k + 1].copy())
    got = r.process(x)
    r.close()
    want = scenes.render_f64([(times, want_rows[k:k + 1], None) for k in range(n_obj)], x, 6)
    err = scenes.rel_rms_per_channel(got, want)
    print(f"allocentric rows on 0+5+0: worst channel relative RMS {err:.3e}")
    assert err <= 1e-6, err
