"""The biquad filter matrix on the device (include/earhip.h, group O) against the float64 model (tests/iir_model.py) under the
header's bound  |y - ref64| <= 2^-24 |ref64| + 1e-9 peak(row),  at the smallest shapes at which the kernels can still go wrong
(sized from earhip_iir_info), under cuttings of the stream, twice for the same bits, and behind a renderer on one stream.

Measured on an MI355X (worst error as a share of the bound, printed by every test): 0.90 .. 0.97 for the sample counts with 1,
2 and 8 sections (0.66 .. 0.96 at n = 1), 0.961 for 24 routes into one output, 0.957 / 0.962 for the 0+5+0 / 9+10+3
bass-management lists, 0.963 under every cutting.  Those figures are the rounding to float32 (half an ulp against
2^-24 |ref|: any correct implementation approaches 1); what the chunking costs in float64 is measured on the CPU form, which
runs the kernels' order of operations: 1.3e-11 of the row's peak against the 1e-9 allowed (tests/test_iir_cpu.py)."""
import numpy as np
import pytest

import iir_model as im
import scenes
from layouts import LAYOUTS

pytestmark = pytest.mark.gpu
FS = 48000.0


@pytest.fixture(scope="module")
def ctx():
    from libear_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run_device(ctx, bank, x, calls=None):
    """x [n_in][n] through process_device in calls of the given lengths, NaN behind the rows' samples -> out [n_out][n]"""
    import torch
    C, n = x.shape
    calls = [n] if calls is None else calls
    assert sum(calls) == n
    stride = n + 5
    xin = torch.full((C, stride), float("nan"), dtype=torch.float32, device="cuda")
    xin[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    K = bank.n_out
    out = torch.full((K + 2, n + 3), 7.5, dtype=torch.float32, device="cuda")
    at = 0
    for k in calls:
        bank.process_device(k, xin.data_ptr() + 4 * at, stride, out[1].data_ptr() + 4 * at, n + 3)
        at += k
    ctx.synchronize()
    o = out.cpu().numpy()
    assert (o[0] == 7.5).all() and (o[K + 1] == 7.5).all() and (o[:, n:] == 7.5).all(), "written beside the call's rows"
    return o[1:K + 1, :n]


def noise(C, n, seed=3):
    return (0.25 * np.random.default_rng(seed).standard_normal((C, n))).astype(np.float32)


def sections(S):
    """S sections with poles close to the unit circle"""
    if S == 1:
        return im.butter_sections(2, 80.0, FS)
    if S == 2:
        return im.lr4("lowpass", 80.0, FS)
    assert S == 8
    return np.concatenate([im.butter_sections(8, 40.0, FS), im.lr4("highpass", 20.0, FS), im.lr4("lowpass", 120.0, FS)])


def check(y, ref, what):
    worst = max(im.worst_ratio(y[k], ref[k]) for k in range(ref.shape[0]))
    print(f"{what}: worst error {worst:.3f} of the bound")
    assert worst <= 1.0, what
    return worst


def lengths(info):
    Lc, lanes, groups = info["chunk"], info["scan_lanes"], info["scan_groups"]
    return [1, Lc - 1, Lc, Lc + 1, lanes * Lc, lanes * Lc + 1, (lanes + 1) * Lc + 3, (groups + 1) * Lc + 5,
            (lanes * groups + 2 + 1) * Lc + 5]  # (the last: just past what one launch holds)


@pytest.mark.parametrize("S", [1, 2, 8])
def test_sample_counts_against_the_model(ctx, S):
    from libear_amd import capi
    sec = sections(S)
    # three inputs, three outputs: a diagonal route, a row of two routes, a row of one
    routes = [(0, 0, 1.0, sec), (1, 1, 0.5, sec), (2, 1, -0.75, sec), (2, 2, 1.5, sec)]
    probe = capi.IirBank(ctx, 3, 3, routes, max_samples=1)
    info = probe.info()
    probe.close()
    assert info["chunk"] >= 2 and info["scan_lanes"] == 64 and info["routes"] == 4 and info["max_state"] == 2 * S
    ns = lengths(info)
    x = noise(3, max(ns), seed=S)
    for n in ns:
        bank = capi.IirBank(ctx, 3, 3, routes, max_samples=n)
        try:
            y = run_device(ctx, bank, x[:, :n])
            check(y, im.model(x[:, :n], 3, routes), f"S = {S}, n = {n}")
        finally:
            bank.close()


def test_routing_gain_routes_an_empty_output_and_more_routes_than_waves(ctx):
    from libear_amd import capi
    n = 70 * 256 + 9
    x = noise(24, n, seed=5)
    lp, hp = im.lr4("lowpass", 80.0, FS), im.lr4("highpass", 80.0, FS)
    # output 0: 24 inputs of 2 sections each; 1: gain routes only; 2: none; 3: a gain route between filtered ones
    routes = [(i, 0, 1.0 / (1 + i % 3), lp) for i in range(24)]
    routes += [(3, 1, -0.5, None), (4, 1, 2.0, None), (0, 3, 1.0, hp), (1, 3, 0.25, None), (2, 3, 1.0, im.butter_sections(2, 500.0, FS))]
    bank = capi.IirBank(ctx, 24, 4, routes, max_samples=n)
    try:
        y = run_device(ctx, bank, x)
        check(y, im.model(x, 4, routes), "24 routes into one output, gain routes, an empty output")
        assert np.all(y[2].view(np.uint32) == 0), "an output without a route must be +0.0"
        want = np.float32(np.float64(-0.5) * x[3].astype(np.float64) + np.float64(2.0) * x[4].astype(np.float64))
        assert np.array_equal(bits(y[1]), bits(want))  # (exact products: the fused sum equals the plain one)
    finally:
        bank.close()


@pytest.mark.parametrize("layout", ["0+5+0", "9+10+3"])
def test_bass_management_lists(ctx, layout):
    from libear_amd import capi
    names = LAYOUTS[layout]
    N, n = len(names), 66 * 256 + 31
    routes = im.bass_management(names, FS)
    x = noise(N, n, seed=8)
    bank = capi.IirBank(ctx, N, N, routes, max_samples=n)
    try:
        assert bank.info()["routes"] == len(routes)
        check(run_device(ctx, bank, x), im.model(x, N, routes), f"bass management of {layout}")
    finally:
        bank.close()


def test_cuttings_the_same_calls_twice_reset_and_two_banks(ctx):
    from libear_amd import capi
    n = 131 * 256 + 77
    x = noise(3, n, seed=13)
    x[1, :] = 0.0
    x[1, 100:] = 0.5  # a step
    routes = [(0, 0, 1.0, sections(8)), (1, 1, 1.0, im.lr4("lowpass", 20.0, FS)), (2, 1, 0.5, None), (2, 2, 1.0, im.lr4("highpass", 80.0, FS))]
    ref = im.model(x, 3, routes)
    a, b = capi.IirBank(ctx, 3, 3, routes, max_samples=n), capi.IirBank(ctx, 3, 3, routes, max_samples=n)
    try:
        Lc = a.info()["chunk"]
        one = run_device(ctx, a, x)
        for cut, calls in im.cuttings(n, Lc).items():
            a.reset()
            y = run_device(ctx, a, x, calls)
            check(y, ref, f"device, {cut}")
            # against one call.  Both are float32 roundings of float64 values that each lie within 1e-9 of the peak of the
            # model; where those two values straddle a rounding tie the outputs differ by a whole ulp = 2^-23 |ref| however
            # close they are, so the bound's first term doubles between two rounded outputs and the second stays
            assert np.all(np.abs(y.astype(np.float64) - one) <= 2.0 ** -23 * np.abs(ref) + 1e-9 * np.abs(ref).max(axis=1, keepdims=True)), cut
            # the same calls on another bank of the same context: the same bits; the first bank is not disturbed
            y2 = run_device(ctx, b, x, calls)
            assert np.array_equal(bits(y), bits(y2)), cut
            b.reset()
        # without a reset the state carries on: the second half of a stream in a call of its own
        a.reset()
        h = n // 2 + 3
        first, second = run_device(ctx, a, x[:, :h]), run_device(ctx, a, x[:, h:])
        check(np.concatenate([first, second], axis=1), ref, "two calls")
        # the host form
        a.reset()
        yh = np.concatenate([a.process(x[:, :h]), a.process(x[:, h:])], axis=1)
        assert np.array_equal(bits(yh), bits(np.concatenate([first, second], axis=1)))
        assert a.process(x[:, :0]).shape == (3, 0)
    finally:
        a.close()
        b.close()


def test_a_refused_call_consumes_nothing(ctx):
    import torch
    from libear_amd import capi
    n = 3000
    x = noise(2, n, seed=17)
    routes = [(0, 0, 1.0, sections(2)), (1, 1, 1.0, sections(1))]
    bank, twin = capi.IirBank(ctx, 2, 2, routes, max_samples=2000), capi.IirBank(ctx, 2, 2, routes, max_samples=2000)
    try:
        first = run_device(ctx, bank, x[:, :1000])
        xi = torch.from_numpy(x).cuda()
        o = torch.zeros((2, n), dtype=torch.float32, device="cuda")
        with pytest.raises(capi.InvalidArgument):
            bank.process_device(2001, xi.data_ptr(), n, o.data_ptr(), n)
        with pytest.raises(capi.InvalidArgument):
            bank.process(x[:, :2001])
        with pytest.raises(capi.InvalidArgument):
            bank.process_device(100, xi.data_ptr(), 99, o.data_ptr(), n)
        with pytest.raises(capi.InvalidArgument):
            bank.process_device(100, None, n, o.data_ptr(), n)
        ctx.synchronize()
        assert not o.any()
        second = run_device(ctx, bank, x[:, 1000:3000])
        want = [run_device(ctx, twin, x[:, :1000]), run_device(ctx, twin, x[:, 1000:3000])]
        assert np.array_equal(bits(first), bits(want[0])) and np.array_equal(bits(second), bits(want[1]))
    finally:
        bank.close()
        twin.close()


def test_a_nan_stays_behind_its_sample_and_in_its_routes(ctx):
    from libear_amd import capi
    n, p = 70 * 256 + 40, 9 * 256 + 77
    x = noise(3, n, seed=19)
    routes = [(0, 0, 1.0, sections(2)), (1, 0, 0.5, sections(8)), (1, 1, 1.0, sections(1)), (2, 2, 1.0, sections(2)), (2, 3, 2.0, None)]
    bank = capi.IirBank(ctx, 3, 4, routes, max_samples=n)
    try:
        clean = run_device(ctx, bank, x)
        bad = x.copy()
        bad[1, p] = np.nan
        bank.reset()
        y = run_device(ctx, bank, bad)
        assert np.array_equal(bits(y[:, :p]), bits(clean[:, :p]))           # earlier samples
        assert np.array_equal(bits(y[2:]), bits(clean[2:]))                  # outputs fed only by other channels
        assert not np.isfinite(y[0, p:]).any() and not np.isfinite(y[1, p:]).any()
        bank.reset()
        assert np.array_equal(bits(run_device(ctx, bank, x)), bits(clean))   # until reset
    finally:
        bank.close()


def test_behind_a_renderer_on_the_same_stream(ctx):
    """the bank fed the rows a render call just wrote, with no synchronisation between the two: both enqueue on the context's
    stream (how a bus is bass-managed while it is still in device memory)"""
    import torch
    from libear_amd import capi
    layout, M, B, T = "0+5+0", 64, 512, 40
    names = LAYOUTS[layout]
    N, n = len(names), T * B
    r = capi.Renderer(ctx, M, N, B, capi.design_decorrelators(names), 255, max_blocks=T)
    for i, (t, d, f) in enumerate(scenes.ragged_curves(M, N, n, seed=41)):
        r.set_object_points(i, t, d, f)
    r.commit()
    routes = im.bass_management(names, FS)
    bank = capi.IirBank(ctx, N, N, routes, max_samples=n)
    x = torch.from_numpy(scenes.audio(M, n, seed=46)).cuda()
    bus = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    managed = torch.full((N, n + 3), 5.5, dtype=torch.float32, device="cuda")
    try:
        torch.cuda.synchronize()
        r.process_device(T, x.data_ptr(), n, bus.data_ptr(), n)
        bank.process_device(n, bus.data_ptr(), n, managed.data_ptr(), n + 3)
        ctx.synchronize()
        got = managed.cpu().numpy()
        assert (got[:, n:] == 5.5).all()
        check(got[:, :n], im.model(bus.cpu().numpy(), N, routes), "behind a renderer, bass management of 0+5+0")
    finally:
        bank.close()
        r.close()
