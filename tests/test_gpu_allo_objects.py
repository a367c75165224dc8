"""The device form of the allocentric panner with extent, channelLock and divergence (earhip_allo_calculate_objects_device,
include/earhip.h group U) on the GPU: against the float64 brute-force model of tests/allo_objects_model.py at the edges of the
kernel's objects-per-workgroup count on layouts of 2 to 32 channels, repeatability, the bit rule for plain rows, absent arrays,
bad elements and the bounds of what it writes.

Device and host run one core (libear_amd/csrc/allo_objects.h) and differ only in the math library, so the bar is the host
form's: one float32 spacing at max(|want|, 2^-20) against float32 of the float64 model."""
import numpy as np
import pytest

import allo_model as M
import allo_objects_model as OM
from _hip import ctx

pytestmark = pytest.mark.gpu

NAMES = ("0+2+0", "0+5+0", "4+5+1", "3+7+0", "9+10+3", M.DOME32_NAME)
RAGGED = 77  # on 9+10+3 and dome32 (8 objects per workgroup): 10 workgroups, the last with 5 objects


def per_workgroup(n_channels):
    """the kernel's objects per workgroup (libear_amd/csrc/allo_objects_kernels.h): 256 threads, an object takes the power
    of two at or above the channel count, at least 2"""
    width = 2
    while width < n_channels:
        width *= 2
    return 256 // width


def sizes(name):
    k = per_workgroup(OM.handle(name)[1].n)
    return (1, k - 1, k, k + 1) + ((RAGGED,) if k == 8 else ())


def _dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def run_device(allo, b, status=False, guard=0, diffuse_out=True, absent=()):
    """b: a batch (allo_objects_model), the keys in `absent` passed as NULL -> (direct, diffuse_out or None
    [n][n_channels] float32, status or None, the guards' contents)"""
    import torch
    from libear_amd import capi
    n, nc = len(b["x"]), allo.n_out
    outs = [torch.full((n * nc + 2 * guard,), 12345.0, dtype=torch.float32, device="cuda") for _ in range(2 if diffuse_out else 1)]
    st = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device="cuda") if status else None
    ins = [None if k in absent else _dev(b[k]) for k in OM.KEYS]
    torch.cuda.synchronize()
    capi.allo_calculate_objects_device(ctx(), allo, n, *ins, outs[0].data_ptr() + 4 * guard,
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


@pytest.mark.parametrize("name", NAMES)
def test_device_form_against_the_brute_force_model(name):
    allo, model, _ = OM.handle(name)
    full, (want_d, want_f) = OM.reference(name)
    lfe = np.array(model.lfe)
    for n in sizes(name):
        b = OM.last(full, n)
        got_d, got_f, st, _ = run_device(allo, b, status=True)
        host_d, host_f = allo.calculate_objects(*(b[k] for k in OM.KEYS))
        for what, got, want, host in (("direct", got_d, want_d[-n:], host_d), ("diffuse", got_f, want_f[-n:], host_f)):
            ok, worst = M.within_one_spacing(got, want)
            print(f"{name} n={n} {what}: worst error {worst:.3f} spacings; bit-identical to the host form "
                  f"{100 * np.mean(got.view(np.uint32) == host.view(np.uint32)):.2f}%")
            assert ok, (n, what, worst)
            assert np.all(got[:, lfe].view(np.uint32) == 0)
        assert np.all(st == 0)


def test_the_same_call_twice_gives_the_same_bits():
    allo, _, _ = OM.handle("9+10+3")
    b = OM.last(OM.reference("9+10+3")[0], RAGGED)
    first, second = run_device(allo, b), run_device(allo, b)
    assert np.array_equal(first[0].view(np.uint32), second[0].view(np.uint32))
    assert np.array_equal(first[1].view(np.uint32), second[1].view(np.uint32))


@pytest.mark.parametrize("name", ("0+5+0", "9+10+3", M.DOME32_NAME))
def test_plain_rows_have_the_bits_of_the_point_source_device_form(name):
    import torch
    from libear_amd import capi
    allo, _, _ = OM.handle(name)
    full = OM.reference(name)[0]
    n, nc = 41, allo.n_out
    b = OM.last(full, n)
    plain = {**OM.plain(n), **{k: b[k] for k in ("x", "y", "z", "gain", "diffuse", "excluded")}}
    got_d, got_f, _, _ = run_device(allo, plain)
    want = [torch.empty((n, nc), dtype=torch.float32, device="cuda") for _ in range(2)]
    capi.allo_calculate_device(ctx(), allo, n, *(_dev(plain[k]) for k in ("x", "y", "z", "gain", "diffuse", "excluded")), *want)
    ctx().synchronize()
    assert np.array_equal(got_d.view(np.uint32), want[0].cpu().numpy().view(np.uint32))
    assert np.array_equal(got_f.view(np.uint32), want[1].cpu().numpy().view(np.uint32))
    # the plain rows of a mixed batch have those bits too: no row depends on its neighbours in the workgroup
    mixed_d, mixed_f, _, _ = run_device(allo, b)
    is_plain = (b["channel_lock"] == 0) & (b["divergence"] == 0) & (b["width"] == 0) & (b["height"] == 0) & (b["depth"] == 0)
    assert np.count_nonzero(is_plain) >= n // 4
    assert np.array_equal(mixed_d[is_plain].view(np.uint32), got_d[is_plain].view(np.uint32))
    assert np.array_equal(mixed_f[is_plain].view(np.uint32), got_f[is_plain].view(np.uint32))


def test_every_optional_array_absent_and_diffuse_out_absent():
    allo, _, _ = OM.handle("4+5+1")
    n = 33
    b = {**OM.plain(n), **{k: OM.last(OM.reference("4+5+1")[0], n)[k] for k in ("x", "y", "z")}}
    optional = [k for k in OM.KEYS if k not in ("x", "y", "z")]
    given = run_device(allo, b)
    bare = run_device(allo, b, absent=optional)
    assert np.array_equal(given[0].view(np.uint32), bare[0].view(np.uint32)) and np.all(bare[1].view(np.uint32) == 0)
    only, none, _, guards = run_device(allo, b, absent=optional, guard=64, diffuse_out=False)
    assert none is None and np.array_equal(only.view(np.uint32), bare[0].view(np.uint32))
    assert all(np.all(g == 12345.0) for g in guards)
    host = allo.calculate_objects(b["x"], b["y"], b["z"])[0]
    ok, worst = M.within_one_spacing(only, host.astype(np.float64))
    assert ok, worst


def test_bad_elements_get_nan_rows_and_status_1_where_the_host_form_refuses():
    from libear_amd import capi
    allo, _, _ = OM.handle("3+7+0")
    n = 40  # 16 objects per workgroup: three workgroups, the last ragged
    b = OM.last(OM.reference("3+7+0")[0], n)
    clean_d, clean_f, st0, _ = run_device(allo, b, status=True)
    assert np.all(st0 == 0) and np.all(np.isfinite(clean_d)) and np.all(np.isfinite(clean_f))
    bad = {0: ("x", np.nan), 3: ("width", -1e-9), 7: ("height", np.inf), 15: ("depth", np.nan), 16: ("divergence", 1.0000001),
           17: ("divergence", np.nan), 21: ("position_range", -1e-9), 22: ("position_range", np.inf),
           30: ("lock_max_distance", -1e-9), 31: ("lock_max_distance", np.nan), 32: ("gain", np.inf), 38: ("diffuse", -1e-9),
           39: ("z", -np.inf)}
    for i, (key, v) in bad.items():
        b[key][i] = v
    b["excluded"][10] |= 0xfffff000  # bits beyond the 12 channels: the device form ignores them (the host form refuses)
    refused = np.zeros(n, bool)
    for i in range(n):
        try:
            row = OM.rows(b, slice(i, i + 1))
            row["excluded"] &= 0xfff
            allo.calculate_objects(*(row[k] for k in OM.KEYS))
        except capi.InvalidArgument:
            refused[i] = True
    assert sorted(np.flatnonzero(refused)) == sorted(bad)
    got_d, got_f, st, _ = run_device(allo, b, status=True)
    assert np.all(np.isnan(got_d[refused])) and np.all(np.isnan(got_f[refused]))
    assert np.array_equal(st, refused.astype(np.int32))
    assert np.array_equal(got_d[~refused].view(np.uint32), clean_d[~refused].view(np.uint32))
    assert np.array_equal(got_f[~refused].view(np.uint32), clean_f[~refused].view(np.uint32))
    again = run_device(allo, b, status=False)  # status=None is accepted
    assert again[2] is None and np.array_equal(again[0].view(np.uint32), got_d.view(np.uint32))


@pytest.mark.parametrize("name,n", [(M.DOME32_NAME, 9), ("3+7+0", 15), ("0+2+0", 129), ("9+10+3", 1), ("0+5+0", RAGGED)])
def test_nothing_is_written_outside_the_outputs_and_status(name, n):
    allo, _, _ = OM.handle(name)
    b = OM.last(OM.reference(name)[0], n)
    got_d, got_f, st, guards = run_device(allo, b, status=True, guard=64)
    assert np.all(np.isfinite(got_d)) and np.all(np.isfinite(got_f)) and np.all(st == 0)
    assert not np.any(got_d == 12345.0) and not np.any(got_f == 12345.0)
    assert all(np.all(g == 12345.0) for g in guards[:4]) and all(np.all(g == -7) for g in guards[4:])


def test_empty_call_is_a_no_op():
    from libear_amd import capi
    capi.allo_calculate_objects_device(ctx(), OM.handle("0+5+0")[0], 0, *([None] * 15))
    ctx().synchronize()
