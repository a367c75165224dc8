"""The delay matrix on the device (include/earhip.h, group S) BIT FOR BIT against the host form of libear_amd/csrc/delaymix.h
built plainly (tests/cpp/delaymix_host.cpp) and against the float64 model under the derived bound of tests/delaymix_model.py, at
the smallest shapes at which the kernel can still go wrong (two tiles and a bit, sized from earhip_delaymix_info), under
cuttings of the stream, with rows on and off the 16-byte grid, canaries around every row, the largest route, a call longer than
one launch, and chained in front of the biquad matrix on one stream.

Measured on an MI355X (worst error as a share of the bound gamma_K S + K 2^-149, printed by every test, the same under every
cutting and row layout): 0.998 for the delayed gains and 0.979 for T = 1, 2, 16, 32 (one product: half an ulp against gamma_1),
0.115 for 18 products into one output, 0.604 for the full matrix, 0.094 at D = 65536 with T = 32; behind the alignment the
biquad matrix is at 0.959 of its own bound; every shape has the host program's bits."""
import numpy as np
import pytest

import delaymix_model as dm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from libear_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def make(ctx, n_in, n_out, routes, max_samples):
    from libear_amd import capi
    return capi.DelayMatrix(ctx, n_in, n_out, routes, max_samples=max_samples)


def run_device(ctx, mx, x, calls=None, odd=False):
    """x [n_in][n] through process_device in calls of the given lengths -> out [n_out][n].  odd: odd strides and row bases one
    float behind a 16-byte boundary, so that no row is made of 16-byte vectors.  NaN behind the input rows' samples and in a
    guard row; canaries in guard rows above and below the output rows and behind their samples"""
    import torch
    n_in, n = x.shape
    calls = [n] if calls is None else calls
    assert sum(calls) == n
    off = 1 if odd else 0
    si = n + (9 if odd else 8) + (n % 2 if odd else -n % 4)
    so = n + (5 if odd else 4) + (n % 2 if odd else -n % 4)
    assert si % 2 == so % 2 == (1 if odd else 0)
    xin = torch.full(((n_in + 1) * si + 4,), float("nan"), dtype=torch.float32, device="cuda")
    rows_in = xin[off:off + n_in * si].view(n_in, si)
    rows_in[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.full(((mx.n_out + 2) * so + 4,), 7.5, dtype=torch.float32, device="cuda")
    assert xin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    torch.cuda.synchronize()  # (the canaries are torch's work on its own stream: done before the context's stream writes among them)
    at = 0
    for k in calls:
        mx.process_device(k, xin.data_ptr() + 4 * (off + at), si, out.data_ptr() + 4 * (off + so + at), so)
        at += k
    ctx.synchronize()
    o = out.cpu().numpy()
    body = o[off:off + (mx.n_out + 2) * so].reshape(mx.n_out + 2, so)
    assert (o[:off] == 7.5).all() and (o[off + (mx.n_out + 2) * so:] == 7.5).all(), "written in front of or behind the rows"
    assert (body[0] == 7.5).all() and (body[-1] == 7.5).all() and (body[:, n:] == 7.5).all(), "written beside the call's rows"
    return body[1:-1, :n].copy()


def check(y, ref, S, K, what):
    worst = dm.worst_ratio(y, ref, S, K)
    print(f"{what}: worst error {worst:.3f} of the bound")
    assert worst <= 1.0, what


def tile_of(ctx):
    probe = make(ctx, 1, 1, [(0, 0, 0, [1.0])], 1)
    info = probe.info()
    probe.close()
    return info["tile_out"], info["launch_in"]


@pytest.mark.parametrize("name", list(dm.CASES))
def test_cases_have_the_host_forms_bits_under_every_cutting_and_row_layout(ctx, name):
    n_in, n_out, routes = dm.CASES[name]
    tile, _ = tile_of(ctx)
    n = 2 * tile + 331
    x = dm.noise(n_in, n, seed=len(name))
    for c in dm.unread(n_in, routes):
        x[c] = np.nan  # an input without a route is never read
    ref, S, K = dm.model(x, n_out, routes)
    host = dm.host_run(x, n_out, routes, sanitize=False)
    H = dm.history(routes)
    mx = make(ctx, n_in, n_out, routes, n)
    try:
        info = mx.info()
        assert info["routes"] == len(routes) and info["history"] == H and info["total_taps"] == sum(len(r[3]) for r in routes)
        assert info["max_fan_in"] == max(sum(1 for r in routes if r[1] == k) for k in range(n_out)) and info["device_bytes"] > 0
        for cut, calls in dm.cuttings(n, H, tile).items():
            for odd in (False, True):
                mx.reset()
                y = run_device(ctx, mx, x, calls, odd=odd)
                check(y, ref, S, K, f"{name}, {cut}, odd rows {odd}")
                assert np.array_equal(dm.bits(y), dm.bits(host)), (cut, odd)
        mx.reset()
        assert np.array_equal(dm.bits(mx.process(x)), dm.bits(host))  # the host-pointer form
    finally:
        mx.close()


def test_calls_of_a_tile_and_its_neighbours(ctx):
    tile, _ = tile_of(ctx)
    n_in, n_out, routes = dm.CASES["T = 1, 2, 16, 32"]
    mx = make(ctx, n_in, n_out, routes, tile + 1)
    try:
        for n in (tile - 1, tile, tile + 1):
            x = dm.noise(n_in, n, seed=n)
            host = dm.host_run(x, n_out, routes, sanitize=False)
            for odd in (False, True):
                mx.reset()
                assert np.array_equal(dm.bits(run_device(ctx, mx, x, odd=odd)), dm.bits(host)), (n, odd)
    finally:
        mx.close()


def test_output_from_history_alone_over_several_calls(ctx):
    """calls much shorter than the delay: for 300 samples every output comes out of the history, which short calls shift"""
    routes = [(0, 0, 300, dm.taps_for(16, 9)), (1, 1, 299, [1.0]), (1, 0, 2, [0.5])]
    n = 1500
    x = dm.noise(2, n, seed=12)
    host = dm.host_run(x, 2, routes, sanitize=False)
    calls = [50] * 12 + [1, 2, 3, 0, 94] + [100] * 8
    mx = make(ctx, 2, 2, routes, 100)
    try:
        for odd in (False, True):
            mx.reset()
            assert np.array_equal(dm.bits(run_device(ctx, mx, x, calls, odd=odd)), dm.bits(host)), odd
    finally:
        mx.close()


def test_the_largest_route(ctx):
    """D = 65536 with T = 32 on one channel, 70,000 samples in two calls: the first gives +0.0 alone"""
    routes = [(0, 0, 65536, dm.taps_for(32, 17))]
    n = 70000
    x = dm.noise(1, n, seed=13)
    host = dm.host_run(x, 1, routes, sanitize=False)
    ref, S, K = dm.model(x, 1, routes)
    mx = make(ctx, 1, 1, routes, 40000)
    try:
        assert mx.info()["history"] == 65536 + 31
        y = run_device(ctx, mx, x, [40000, 30000])
        assert not y[0, :65536].view(np.uint32).any()
        check(y, ref, S, K, "D = 65536, T = 32")
        assert np.array_equal(dm.bits(y), dm.bits(host))
    finally:
        mx.close()


def test_a_call_one_sample_longer_than_a_launch(ctx):
    _, launch = tile_of(ctx)
    routes = [(0, 0, 5, dm.taps_for(2, 21))]
    n = launch + 1
    x = dm.noise(1, n, seed=14)
    host = dm.host_run(x, 1, routes, sanitize=False)
    mx = make(ctx, 1, 1, routes, n)
    try:
        assert np.array_equal(dm.bits(run_device(ctx, mx, x)), dm.bits(host))
    finally:
        mx.close()


def test_a_nan_reaches_exactly_the_outputs_whose_window_holds_it(ctx):
    n_in, n_out, routes = dm.CASES["a full matrix"]
    tile, _ = tile_of(ctx)
    n = tile + 500
    x = dm.noise(n_in, n, seed=5)
    mx = make(ctx, n_in, n_out, routes, n)
    try:
        clean = run_device(ctx, mx, x)
        for c, s in ((0, tile - 1), (1, 0), (2, n - 140)):
            bad = x.copy()
            bad[c, s] = np.nan
            mx.reset()
            y = run_device(ctx, mx, bad, [700, n - 700], odd=True)
            hit = np.zeros((n_out, n), bool)
            t = np.arange(n)
            for i, o, d, h in dm.routes32(routes):
                if i == c:
                    hit[o] |= (t - d - h.size + 1 <= s) & (s <= t - d)
            assert hit.any() and not np.isfinite(y[hit]).any(), (c, s)
            assert np.array_equal(dm.bits(y[~hit]), dm.bits(clean[~hit])), (c, s)
    finally:
        mx.close()


def test_a_refused_call_consumes_nothing_reset_restarts_and_two_matrices_interleave(ctx):
    import torch
    from libear_amd import capi
    _, n_out, routes = dm.CASES["a full matrix"]
    other = [(0, 0, 17, dm.taps_for(16, 31)), (1, 1, 0, [-1.0]), (2, 2, 3, [1.0])]
    n = 3000
    x = dm.noise(3, n, seed=41)
    want_a = dm.host_run(x, 3, routes, sanitize=False)
    want_b = dm.host_run(x, 3, other, sanitize=False)
    a, b = make(ctx, 3, 3, routes, 2000), make(ctx, 3, 3, other, 2000)
    try:
        first = run_device(ctx, a, x[:, :1001])
        xi = torch.from_numpy(x).cuda()
        o = torch.zeros((3, 4000), dtype=torch.float32, device="cuda")
        with pytest.raises(capi.InvalidArgument):
            a.process_device(2001, xi.data_ptr(), n, o.data_ptr(), 4000)  # beyond max_samples
        with pytest.raises(capi.InvalidArgument):
            a.process(x[:, :2001])
        with pytest.raises(capi.InvalidArgument):
            a.process_device(100, xi.data_ptr(), 99, o.data_ptr(), 4000)
        with pytest.raises(capi.InvalidArgument):
            a.process_device(100, xi.data_ptr(), n, o.data_ptr(), 99)
        with pytest.raises(capi.InvalidArgument):
            a.process_device(100, None, n, o.data_ptr(), 4000)
        ctx.synchronize()
        assert not o.any()
        second = run_device(ctx, a, x[:, 1001:])  # the stream goes on where it was
        assert np.array_equal(dm.bits(np.concatenate([first, second], axis=1)), dm.bits(want_a))
        a.reset()
        assert np.array_equal(dm.bits(run_device(ctx, a, x[:, :1001])), dm.bits(first))
        # interleaved calls of the two: neither disturbs the other
        a.reset()
        cuts = [0, 3, 40, 1301, n]
        ya, yb = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            ya.append(run_device(ctx, a, x[:, lo:hi]))
            yb.append(run_device(ctx, b, x[:, lo:hi], odd=True))
        assert np.array_equal(dm.bits(np.concatenate(ya, axis=1)), dm.bits(want_a))
        assert np.array_equal(dm.bits(np.concatenate(yb, axis=1)), dm.bits(want_b))
        assert a.process(x[:, :0]).shape == (3, 0)
    finally:
        a.close()
        b.close()


def test_in_front_of_the_biquad_matrix_on_one_stream(ctx):
    """process_device, then IirBank.process_device on its rows without a synchronisation in between: the two models chained,
    within the biquad matrix's bound"""
    import torch
    import iir_model as im
    from libear_amd import capi
    fs, n = 48000.0, 4000
    names = ["M+030", "M-030", "M+000", "LFE1"]
    delay, gain = capi.delaymix_align([2.0, 2.5, 3.1, 1.2], fs)
    routes = []
    for c in range(4):
        whole, h = capi.delaymix_fractional(delay[c] + 7.0, 16, 8.0)
        routes.append((c, c, whole, (h * gain[c]).astype(np.float32)))
    iir_routes = im.bass_management(names, fs)
    x = dm.noise(4, n, seed=51)
    aligned = dm.host_run(x, 4, routes, sanitize=False)
    ref = im.model(aligned, 4, iir_routes)
    mx, bank = make(ctx, 4, 4, routes, n), capi.IirBank(ctx, 4, 4, iir_routes, max_samples=n)
    try:
        xi = torch.from_numpy(x).cuda()
        mid = torch.zeros((4, n), dtype=torch.float32, device="cuda")
        out = torch.zeros((4, n), dtype=torch.float32, device="cuda")
        for lo, hi in ((0, 1500), (1500, n)):
            mx.process_device(hi - lo, xi.data_ptr() + 4 * lo, n, mid.data_ptr() + 4 * lo, n)
            bank.process_device(hi - lo, mid.data_ptr() + 4 * lo, n, out.data_ptr() + 4 * lo, n)
        ctx.synchronize()
        assert np.array_equal(dm.bits(mid.cpu().numpy()), dm.bits(aligned))
        worst = im.worst_ratio(out.cpu().numpy(), ref)
        print(f"alignment in front of bass management: worst error {worst:.3f} of the biquad matrix's bound")
        assert worst <= 1.0
    finally:
        mx.close()
        bank.close()


def test_the_host_form_never_looks_at_the_row_of_an_input_without_a_route(ctx):
    """include/earhip.h, group S: the host form does not look at the pointer of an input without a route.  3 -> 2, two routes, input 2
    unrouted, one tile + 3 samples, through the library's own symbols (the wrapper cannot pass a NULL row): a NULL pointer there
    gives the bits of a NaN row there; a NULL pointer of an input that is read is EARHIP_INVALID_ARGUMENT and consumes nothing"""
    import ctypes as C
    from libear_amd import capi
    lib = capi.load()
    tile, _ = tile_of(ctx)
    n = tile + 3
    routes = [(0, 0, 5, dm.taps_for(2, 21)), (1, 1, 0, [-0.5])]
    x = dm.noise(3, n, seed=23)
    x[2] = np.nan

    def call(mx, null_row):
        rows = capi._chan_ptrs(x)
        if null_row is not None:
            rows[null_row] = None
        out = np.full((2, n), 7.5, np.float32)
        return lib.earhip_delaymix_process(mx.h, C.c_size_t(n), rows, capi._chan_ptrs(out)), out

    mx, fresh = make(ctx, 3, 2, routes, n), make(ctx, 3, 2, routes, n)
    try:
        rc, with_nan = call(fresh, None)
        assert rc == capi.OK and np.isfinite(with_nan).all()
        rc, untouched = call(mx, 1)  # an input that is read
        assert rc == capi.INVALID_ARGUMENT and (untouched == 7.5).all()
        rc, with_null = call(mx, 2)  # the next valid call: a fresh matrix's bits, the unread row's pointer NULL
        assert rc == capi.OK, lib.earhip_last_error()
        assert np.array_equal(dm.bits(with_null), dm.bits(with_nan))
    finally:
        mx.close()
        fresh.close()
