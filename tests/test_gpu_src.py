"""The polyphase sample-rate converter on the device (include/earhip.h, group P) against scipy.signal.upfirdn under the derived
bound of tests/src_model.py (gamma_T S + T 2^-149, nothing left out) and BIT FOR BIT against the host form of
libear_amd/csrc/src.h built plainly (tests/cpp/src_host.cpp), at the smallest shapes at which the kernel can still go wrong
(three tiles and a bit, sized from earhip_src_info), under cuttings of the stream, with guards around every row, and at the
shapes where the kernel reads its table or its inputs through the caches instead of LDS.

Measured on an MI355X (worst error as a share of the bound, printed by every test, the same under every cutting): 0.11 .. 0.21
for the ratio cases with T = 24 and 48, 0.02 .. 0.04 at T = 256, 0.54 at 1/64 with T = 4, 0.48 for 16 x 200,000 samples at 3/2;
every shape has the host program's bits."""
import numpy as np
import pytest

import src_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from libear_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def make(ctx, C, case, max_samples, h=None):
    from libear_amd import capi
    L, M, T = case
    return capi.SampleRateConverter(ctx, C, L, M, T, sm.taps_for(L, M, T) if h is None else h, max_samples=max_samples)


def run_device(ctx, src, x, calls=None, in_pad=5, out_pad=3, counts=None):
    """x [C][n] through process_device in calls of the given lengths, every call with exactly the capacity it needs; NaN behind
    the input rows' samples, guard rows above and below the output rows and guard samples behind them -> out [C][total]
    (counts: a list that receives the outputs of every call)"""
    import torch
    C, n = x.shape
    calls = [n] if calls is None else calls
    assert sum(calls) == n
    total = 0
    stride = n + in_pad
    xin = torch.full((C, stride), float("nan"), dtype=torch.float32, device="cuda")
    xin[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    room = sm.n_outputs(n, src.up, src.down)  # (a stream that does not start at clock 0 produces no more)
    out = torch.full((C + 2, room + out_pad), 7.5, dtype=torch.float32, device="cuda")
    at = 0
    for k in calls:
        want = src.next_out(k)
        got = src.process_device(k, xin.data_ptr() + 4 * at, stride, out[1].data_ptr() + 4 * total, room + out_pad, want)
        assert got == want
        if counts is not None:
            counts.append(got)
        at += k
        total += got
    ctx.synchronize()
    o = out.cpu().numpy()
    assert (o[0] == 7.5).all() and (o[C + 1] == 7.5).all() and (o[:, total:] == 7.5).all(), "written beside the call's rows"
    return o[1:C + 1, :total]


def check(y, ref, S, T, what):
    worst = sm.worst_ratio(y, ref, S, T)
    print(f"{what}: worst error {worst:.3f} of the bound")
    assert worst <= 1.0, what


@pytest.mark.parametrize("case", sm.CASES, ids=sm.case_id)
def test_ratio_cases_against_upfirdn_the_host_program_and_under_every_cutting(ctx, case):
    L, M, T = case
    probe = make(ctx, 3, case, 1)
    info = probe.info()
    probe.close()
    assert (info["up"], info["down"], info["taps_per_phase"]) == case and info["max_out"] == sm.n_outputs(1, L, M)
    assert info["table_in_lds"] == 1 and info["window_in_lds"] == 1
    assert info["latency_prototype"] == (L * T - 1) / 2 and info["latency_in"] == (L * T - 1) / (2 * L) and info["latency_out"] == (L * T - 1) / (2 * M)
    tile = info["tile_in"]
    assert tile == -((-info["tile_out"] * M) // L)
    n = 3 * tile + 77
    x = sm.noise(3, n, seed=L + M)
    h = sm.taps_for(L, M, T)
    ref, S = sm.model(x, h, L, M)
    host, _ = sm.host_run(x, h, L, M, T, sanitize=False)
    src = make(ctx, 3, case, n)
    try:
        assert src.max_out == sm.n_outputs(n, L, M)
        for cut, calls in sm.cuttings(n, tile).items():
            src.reset()
            counts = []
            y = run_device(ctx, src, x, calls, counts=counts)
            assert [int(v) for v in np.cumsum(counts)] == [sm.n_outputs(int(v), L, M) for v in np.cumsum(calls)], cut
            check(y, ref, S, T, f"{sm.case_id(case)}, {cut}")
            assert np.array_equal(sm.bits(y), sm.bits(host)), cut
    finally:
        src.close()


@pytest.mark.parametrize("case,table,window", [((128, 127, 256), 0, 1), ((1, 64, 4), 1, 0), ((67, 1024, 256), 0, 0)],
                         ids=["table through the caches", "inputs through the caches", "both through the caches"])
def test_shapes_that_do_not_fit_the_lds(ctx, case, table, window):
    L, M, T = case
    probe = make(ctx, 2, case, 1)
    info = probe.info()
    probe.close()
    assert (info["table_in_lds"], info["window_in_lds"]) == (table, window)
    tile = info["tile_in"]
    n = 2 * tile + 77
    x = sm.noise(2, n, seed=T)
    h = sm.taps_for(L, M, T)
    ref, S = sm.model(x, h, L, M)
    host, _ = sm.host_run(x, h, L, M, T, sanitize=False)
    src = make(ctx, 2, case, n)
    try:
        for cut in ("one call", "around the tile"):
            src.reset()
            y = run_device(ctx, src, x, sm.cuttings(n, tile)[cut])
            check(y, ref, S, T, f"{sm.case_id(case)}, {cut}")
            assert np.array_equal(sm.bits(y), sm.bits(host)), cut
    finally:
        src.close()


def test_workgroups_that_take_several_tiles(ctx):
    """enough tiles that a workgroup keeps its table over more than one (16 rows of 293 tiles)"""
    case = L, M, T = (3, 2, 8)
    n = 200000
    x = sm.noise(16, n, seed=29)
    h = sm.taps_for(L, M, T)
    ref, S = sm.model(x, h, L, M)
    host, _ = sm.host_run(x, h, L, M, T, sanitize=False)
    src = make(ctx, 16, case, n)
    try:
        y = run_device(ctx, src, x)
        check(y, ref, S, T, "16 x 200,000 samples at 3/2")
        assert np.array_equal(sm.bits(y), sm.bits(host))
    finally:
        src.close()


def test_a_call_longer_than_one_launch(ctx):
    """a call of more than 2^20 inputs runs as two launches: the second starts from the first's clock and history"""
    case = L, M, T = (2, 3, 8)
    n = (1 << 20) + 777
    x = sm.noise(1, n, seed=30)
    h = sm.taps_for(L, M, T)
    host, _ = sm.host_run(x, h, L, M, T, sanitize=False)
    src = make(ctx, 1, case, n)
    try:
        y = run_device(ctx, src, x)
        assert np.array_equal(sm.bits(y), sm.bits(host))
        src.reset()
        assert np.array_equal(sm.bits(src.process(x)), sm.bits(host))  # the host-pointer form
    finally:
        src.close()


def test_a_nan_reaches_exactly_the_outputs_whose_window_holds_it(ctx):
    for case in ((160, 147, 48), (1, 2, 8)):
        L, M, T = case
        src = make(ctx, 2, case, 8000)
        try:
            n = 2 * src.info()["tile_in"] + 300
            x = sm.noise(2, n, seed=31)
            clean = run_device(ctx, src, x)
            for s in (0, 1500, n - 1):
                bad = x.copy()
                bad[1, s] = np.nan
                src.reset()
                y = run_device(ctx, src, bad, [700, n - 700])
                i = (np.arange(y.shape[1]) * M) // L
                hit = (i - T + 1 <= s) & (s <= i)
                # (at 1/2 no output reads the odd last sample: then every output must have the clean bits)
                assert hit.any() == (case != (1, 2, 8) or s != n - 1) and not np.isfinite(y[1, hit]).any(), (case, s)
                assert np.array_equal(sm.bits(y[1, ~hit]), sm.bits(clean[1, ~hit])), (case, s)
                assert np.array_equal(sm.bits(y[0]), sm.bits(clean[0])), (case, s)
        finally:
            src.close()


def test_strides_unequal_to_the_lengths(ctx):
    case = (147, 160, 48)
    src = make(ctx, 3, case, 4000)
    try:
        x = sm.noise(3, 3001, seed=37)
        a = run_device(ctx, src, x, [1000, 2001])
        src.reset()
        b = run_device(ctx, src, x, [1000, 2001], in_pad=1234, out_pad=777)
        assert np.array_equal(sm.bits(a), sm.bits(b))
    finally:
        src.close()


def test_a_refused_call_consumes_nothing_and_reset_restarts_the_stream(ctx):
    import torch
    from libear_amd import capi
    case = L, M, T = (160, 147, 48)
    n = 3000
    x = sm.noise(2, n, seed=41)
    src, twin = make(ctx, 2, case, 2000), make(ctx, 2, case, 2000)
    try:
        first = run_device(ctx, src, x[:, :1001])
        xi = torch.from_numpy(x).cuda()
        o = torch.zeros((2, 4000), dtype=torch.float32, device="cuda")
        need = src.next_out(1999)
        assert need == sm.n_outputs(3000, L, M) - sm.n_outputs(1001, L, M)
        with pytest.raises(capi.InvalidArgument):
            src.process_device(1999, xi.data_ptr() + 4 * 1001, n, o.data_ptr(), 4000, need - 1)  # one short
        with pytest.raises(capi.InvalidArgument):
            src.process_device(2001, xi.data_ptr(), n, o.data_ptr(), 4000, 4000)  # beyond max_samples
        with pytest.raises(capi.InvalidArgument):
            src.process(x[:, :2001])
        with pytest.raises(capi.InvalidArgument):
            src.next_out(2001)
        with pytest.raises(capi.InvalidArgument):
            src.process_device(100, xi.data_ptr(), 99, o.data_ptr(), 4000, 4000)
        with pytest.raises(capi.InvalidArgument):
            src.process_device(100, None, n, o.data_ptr(), 4000, 4000)
        ctx.synchronize()
        assert not o.any()
        assert src.next_out(1999) == need  # the clock has not moved
        second = run_device(ctx, src, x[:, 1001:])
        want = [run_device(ctx, twin, x[:, :1001]), run_device(ctx, twin, x[:, 1001:])]
        assert np.array_equal(sm.bits(first), sm.bits(want[0])) and np.array_equal(sm.bits(second), sm.bits(want[1]))
        host, _ = sm.host_run(x, sm.taps_for(L, M, T), L, M, T, sanitize=False)
        assert np.array_equal(sm.bits(np.concatenate([first, second], axis=1)), sm.bits(host))
        # after reset the stage restarts the stream
        src.reset()
        again = run_device(ctx, src, x[:, :1001])
        assert np.array_equal(sm.bits(again), sm.bits(first))
    finally:
        src.close()
        twin.close()


def test_host_pointer_form_and_two_converters_on_one_context(ctx):
    up, down = (160, 147, 48), (147, 160, 48)
    n = 2500
    x = sm.noise(3, n, seed=43)
    a, b = make(ctx, 3, up, n), make(ctx, 3, down, n)
    try:
        want_a = sm.host_run(x, sm.taps_for(*up), *up, sanitize=False)[0]
        want_b = sm.host_run(x, sm.taps_for(*down), *down, sanitize=False)[0]
        # interleaved calls of the two: neither disturbs the other
        cuts = [0, 3, 40, 1301, n]
        ya, yb, ha, hb = [], [], [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            ya.append(run_device(ctx, a, x[:, lo:hi]))
            yb.append(run_device(ctx, b, x[:, lo:hi]))
        assert np.array_equal(sm.bits(np.concatenate(ya, axis=1)), sm.bits(want_a))
        assert np.array_equal(sm.bits(np.concatenate(yb, axis=1)), sm.bits(want_b))
        # the host-pointer form gives the device form's bits
        a.reset()
        b.reset()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            ha.append(a.process(x[:, lo:hi]))
            hb.append(b.process(x[:, lo:hi]))
        assert np.array_equal(sm.bits(np.concatenate(ha, axis=1)), sm.bits(want_a))
        assert np.array_equal(sm.bits(np.concatenate(hb, axis=1)), sm.bits(want_b))
        assert a.process(x[:, :0]).shape == (3, 0)
    finally:
        a.close()
        b.close()
