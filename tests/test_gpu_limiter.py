"""The look-ahead limiter (include/earhip.h, group N) on the device: against the float64 model (tests/limiter_model.py) under the
model's bound, bit-identical to the shared maths header compiled for the host (libear_amd/csrc/limiter.h) and to itself however
the stream is cut, never above c (1 + 2^-22), its PCM form against pcm_out_model, and attached to a renderer
(earhip_render_attach_limiter), where the sink must hold the bits of a stand-alone limiter fed the rows the call returned.

Measured on an MI355X: see DESIGN.md section 5."""
import numpy as np
import pytest

import limiter_model as lm
import pcm_model
import pcm_out_model
import scenes
from layouts import LAYOUTS
from test_gpu_loudness import BLOCK, FORMS, LAYOUT, M_OBJ, NBLOCKS, TWIN, make_renderer, run_form

pytestmark = pytest.mark.gpu

TILE = 1024  # samples of a workgroup of the gain pass; the detector's tiles are 512 and 256


@pytest.fixture(scope="module")
def ctx():
    from libear_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run_device(ctx, lim, x, calls=None, in_stride=None):
    """x [C][n] through process_device in calls of the given lengths, NaN behind the rows' samples -> (out [C][n], g [n])"""
    import torch
    C, n = x.shape
    calls = [n] if calls is None else calls
    assert sum(calls) == n
    stride = in_stride or n + 5
    xin = torch.full((C, stride), float("nan"), dtype=torch.float32, device="cuda")
    xin[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.full((C + 2, n + 3), 7.5, dtype=torch.float32, device="cuda")
    g = torch.full((n + 1,), 7.5, dtype=torch.float32, device="cuda")
    at = 0
    for k in calls:
        lim.process_device(k, xin.data_ptr() + 4 * at, stride, out[1].data_ptr() + 4 * at, n + 3, g.data_ptr() + 4 * at)
        at += k
    ctx.synchronize()
    o, gg = out.cpu().numpy(), g.cpu().numpy()
    assert (o[0] == 7.5).all() and (o[C + 1] == 7.5).all() and (o[:, n:] == 7.5).all() and gg[n] == 7.5, "written beside the call's rows"
    return o[1:C + 1, :n], gg[:n]


def small_signal(c, M, n=3 * TILE + 77, seed=21):
    """C = 3: noise at 2.5 c with a silent stretch (longer than M where the signal has room for it, else a third of it), noise in
    bursts, and a channel of quarter-rate-sine inter-sample overs"""
    rng = np.random.default_rng(seed)
    x = np.zeros((3, n), np.float32)
    x[0] = rng.uniform(-2.5 * c, 2.5 * c, n)
    x[1] = rng.uniform(-2.5 * c, 2.5 * c, n) * (rng.uniform(0, 1, n) < 0.02)
    x[2] = 0.99 * c * np.sin(2 * np.pi * np.arange(n) / 4.0 + np.pi / 4) / np.sin(np.pi / 4)  # samples at 0.99 c, true peak 1.4 c
    quiet = min(M + 9, n // 3)
    x[:, 600:600 + quiet] = 0.0
    x[:, :100] = 0.0  # (the gain starts at 1)
    return x


@pytest.mark.parametrize("L,H,detect,table", [(8, 0, 1, None), (64, 1500, 1, None), (64, 0, 0, None), (1024, 8192, 1, None),
                                               (16, 30, 1, "2x24"), (8, 3, 1, "1x1")])
def test_smallest_shapes_against_the_model_and_the_header(ctx, L, H, detect, table):
    from libear_amd import capi
    c = 0.4
    if table == "2x24":
        table = np.random.default_rng(5).uniform(-0.3, 0.3, (2, 24))
        table[:, 11] += 1.0
    elif table == "1x1":
        table = np.array([[-1.25]])
    D, M, _, taps, phases = lm.shape(L, H, detect, table)
    x = small_signal(c, M)
    n = x.shape[1]
    want = lm.limit(x, c, L, H, detect, table)
    host = lm.host_run(x, c, L, H, detect, table=table, sanitize=False)
    lim = capi.Limiter(ctx, 3, c, L, H, 96000 if table is not None else 48000, (phases, taps, table) if table is not None else bool(detect),
                       max_samples=n)
    try:
        assert lim.latency() == D + L == want["latency"]
        runs = {"one call": None, "calls across the tiles": [1, TILE - 1, 5, 0, TILE + 500, n - 2 * TILE - 505]}
        for name, calls in runs.items():
            lim.reset()
            out, g = run_device(ctx, lim, x, calls)
            ro, rg = lm.worst_ratios(out, g, want, x, c, L, H, detect, table)
            print(f"L={L} H={H} detect={detect}, {name}: worst error {ro:.3f} of the bound (out), {rg:.3f} (g); "
                  f"max |out| / c = {np.abs(out).max() / np.float32(c):.9f}; limited {int((g < 1).sum())} of {n}")
            assert ro <= 1.0 and rg <= 1.0
            assert np.abs(out).max() <= lm.guarantee(c)
            assert np.array_equal(bits(out), bits(host["out"])) and np.array_equal(bits(g), bits(host["g"])), name
            mg, cnt = lim.stats()
            assert mg == g.min() == host["min_gain"] and cnt == int((g < 1).sum()) == host["limited"] and 0 < cnt < n
    finally:
        lim.close()


def test_cut_invariance_stats_and_levels(ctx):
    import torch
    from libear_amd import capi
    C, n, c, L, H = 24, 2 * 48000 + 1234, 0.891, 64, 480
    rng = np.random.default_rng(31)
    x = (rng.standard_normal((C, n)) * 0.4).astype(np.float32)
    x[:, 30000:33000] *= 0.01
    cuts = [int(v) for v in rng.integers(1, 30000, 12)]
    cuts = cuts[:next(i for i in range(len(cuts)) if sum(cuts[:i + 1]) > n - 30000)]
    short = [int(v) for v in rng.integers(0, 700, 40)]
    cuttings = {"one call": [n], "random calls": cuts + [n - sum(cuts)], "40 calls under 700 samples first": short + [n - sum(short)]}
    lim = capi.Limiter(ctx, C, c, L, H, max_samples=n)
    frames = torch.zeros((n, C), dtype=torch.int16, device="cuda")
    xin = torch.from_numpy(x).cuda()
    first = None
    try:
        for name, calls in cuttings.items():
            for again in range(2):
                lim.reset()
                out, g = run_device(ctx, lim, x, calls, in_stride=n + 13)
                stats = lim.stats()
                assert stats[0] == g.min() and stats[1] == int((g < 1).sum())  # exactly the returned gain row's
                lim.reset()
                frames.zero_()
                at = 0
                for k in calls:
                    lim.process_pcm_device(k, xin.data_ptr() + 4 * at, n, frames.data_ptr() + 2 * C * at, 2 * C, 0, "s16", dither=True, seed=3)
                    at += k
                peak, clipped = lim.output_levels()
                got = (out, g, np.array(stats[0]), np.array(stats[1]), frames.cpu().numpy(), peak, clipped, np.array(lim.stats()[1]))
                if first is None:
                    first = got
                    assert 1000 < stats[1] < n and np.abs(out).max() <= lm.guarantee(c) and peak.max() <= lm.guarantee(c)
                    assert np.array_equal(peak, np.abs(out).max(axis=1))
                for a, b in zip(got, first):
                    assert np.array_equal(bits(a), bits(b)), (name, again)
    finally:
        lim.close()


def test_host_form_reset_and_two_limiters_on_one_context(ctx):
    from libear_amd import capi
    c, L, H = 0.5, 32, 100
    x = small_signal(c, L + 2 + H, n=2 * TILE + 300, seed=4)
    n = x.shape[1]
    a, b = capi.Limiter(ctx, 3, c, L, H, true_peak=True, max_samples=n), capi.Limiter(ctx, 3, c, L, H, true_peak=False, max_samples=n)
    try:
        want = {True: lm.host_run(x, c, L, H, True, sanitize=False), False: lm.host_run(x, c, L, H, False, sanitize=False)}
        # the two take turns call by call
        half = n // 2 + 3
        got = {True: [], False: []}
        for lo, hi in ((0, half), (half, n)):
            for lim, detect in ((a, True), (b, False)):
                got[detect].append(lim.process(x[:, lo:hi], with_gain=True))
        for detect in (True, False):
            out, g = np.concatenate([p[0] for p in got[detect]], axis=1), np.concatenate([p[1] for p in got[detect]])
            assert np.array_equal(bits(out), bits(want[detect]["out"])) and np.array_equal(bits(g), bits(want[detect]["g"])), detect
        assert a.stats() == (want[True]["min_gain"], want[True]["limited"]) and b.stats()[1] == want[False]["limited"]
        assert not np.array_equal(want[True]["g"], want[False]["g"])
        # reset: a fresh object's bits again, stats at their start; without the gain row too
        a.reset()
        assert a.stats() == (1.0, 0)
        assert np.array_equal(bits(a.process(x)), bits(want[True]["out"]))
        assert a.stats(reset=True)[1] == want[True]["limited"] and a.stats() == (1.0, 0)
        assert a.process(np.zeros((3, 0), np.float32)).shape == (3, 0)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("fmt,dither", [("s16", False), ("s16", True), ("s24", False), ("s32", False)])
def test_pcm_form_against_the_conversion_model(ctx, fmt, dither):
    import torch
    from libear_amd import capi
    C, n, c, L, H = 5, 2 * TILE + 131, 0.891, 64, 200
    x = (np.random.default_rng(17).standard_normal((C, n)) * 0.7).astype(np.float32)
    S = {"s16": 2, "s24": 3, "s32": 4}[fmt]
    first_byte, frame_bytes = (7, C * S + 12) if fmt == "s24" else (2 * S, (C + 5) * S)
    lim, twin = capi.Limiter(ctx, C, c, L, H, max_samples=n), capi.Limiter(ctx, C, c, L, H, max_samples=n)
    try:
        rows, _ = run_device(ctx, twin, x)
        xin = torch.from_numpy(x).cuda()
        frames = torch.full((n, frame_bytes), 0xA5, dtype=torch.uint8, device="cuda")
        calls = [TILE + 7, n - TILE - 7]  # the dither's t runs on across the calls
        at = 0
        for k in calls:
            lim.process_pcm_device(k, xin.data_ptr() + 4 * at, n, frames.data_ptr() + frame_bytes * at, frame_bytes, first_byte, fmt,
                                   dither=dither, seed=99)
            at += k
        peak, clipped = lim.output_levels()
        got = frames.cpu().numpy()
        want, want_clipped = pcm_out_model.from_float(rows.T, fmt, dither, 99, 0)
        run = got[:, first_byte:first_byte + C * S]
        assert np.array_equal(run, pcm_out_model.as_bytes(want)), fmt
        assert (got[:, :first_byte] == 0xA5).all() and (got[:, first_byte + C * S:] == 0xA5).all(), "bytes outside the runs were written"
        assert np.array_equal(peak, pcm_out_model.peak(rows.T)) and peak.max() <= lm.guarantee(c)
        assert np.array_equal(clipped, want_clipped.sum(axis=0).astype(np.uint64))
        if not dither:
            assert not clipped.any()  # the point of the stage: the float rows clip (|x| reaches 3), the limited ones do not
        assert np.abs(x).max() > 1.5 and lim.stats() == twin.stats()
        assert lim.output_levels(reset=True)[0].max() > 0 and not lim.output_levels()[0].any()
    finally:
        lim.close()
        twin.close()


def test_argument_refusals_consume_nothing(ctx):
    import torch
    from libear_amd import capi
    C, n, c, L, H = 2, 700, 0.3, 8, 0
    x = small_signal(c, L + 2 + H, n=n, seed=6)[:C]
    lim, fresh = capi.Limiter(ctx, C, c, L, H, max_samples=n // 2), capi.Limiter(ctx, C, c, L, H, max_samples=n // 2)
    xin = torch.from_numpy(x).cuda()
    out = torch.zeros((C, n), dtype=torch.float32, device="cuda")
    pcm = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    try:
        want_a, _ = run_device(ctx, fresh, x[:, :n // 2])
        ok = dict(n_channels=C, ceiling=c, lookahead=L, hold=H, max_samples=10)
        for kw in (dict(n_channels=0), dict(n_channels=65), dict(sample_rate=0), dict(sample_rate=96000), dict(ceiling=0.0),
                   dict(ceiling=float("nan")), dict(lookahead=7), dict(lookahead=1025), dict(hold=-1), dict(hold=8193),
                   dict(max_samples=0), dict(true_peak=(0, 12, np.zeros(0))), dict(true_peak=(9, 2, np.ones(18))),
                   dict(true_peak=(2, 65, np.ones(130))), dict(true_peak=(1, 2, np.array([1.0, np.inf])))):
            with pytest.raises(capi.InvalidArgument):
                capi.Limiter(ctx, **dict(ok, **kw))
        capi.Limiter(ctx, **dict(ok, sample_rate=96000, true_peak=False)).close()  # (sample peaks at any rate)
        p, o = xin.data_ptr(), out.data_ptr()
        refused = [lambda: lim.process_device(n // 2 + 1, p, n, o, n), lambda: lim.process_device(10, 0, n, o, n),
                   lambda: lim.process_device(10, p, n, 0, n), lambda: lim.process_device(10, p, 9, o, n),
                   lambda: lim.process_device(10, p, n, o, 9), lambda: lim.process(x), lambda: lim.process(x[:1, :10]),
                   lambda: lim.process_pcm_device(n // 2 + 1, p, n, pcm.data_ptr(), 64, 0, "s16"),
                   lambda: lim.process_pcm_device(10, p, n, 0, 64, 0, "s16"),
                   lambda: lim.process_pcm_device(10, p, n, pcm.data_ptr() + 1, 64, 0, "s16"),
                   lambda: lim.process_pcm_device(10, p, n, pcm.data_ptr(), 2 * C - 2, 0, "s16"),
                   lambda: lim.process_pcm_device(10, p, n, pcm.data_ptr(), 64, 62, "s16"),
                   lambda: lim.process_pcm_device(10, p, n, pcm.data_ptr(), 64, 1, "s16"),
                   lambda: lim.process_pcm_device(10, p, n, pcm.data_ptr(), 64, 0, "s24", dither=True),
                   lambda: lim.process_pcm_device(10, p, n, pcm.data_ptr(), 64, 0, 9),
                   lambda: lim.process_pcm_device(10, p, 9, pcm.data_ptr(), 64, 0, "s16")]
        for i, call in enumerate(refused):
            with pytest.raises((capi.InvalidArgument, AssertionError, ValueError)):
                call()
        ctx.synchronize()
        assert not pcm.any() and not out.any() and lim.stats() == (1.0, 0)
        got, _ = run_device(ctx, lim, x[:, :n // 2])
        assert np.array_equal(bits(got), bits(want_a)), "a refused call consumed something"
    finally:
        lim.close()
        fresh.close()


# ---- attached to a renderer -------------------------------------------------------------------------------------------------
def ceiling_for(rows):
    """a ceiling the bus passes by 10 dB"""
    c = float(np.float32(0.3 * np.abs(rows).max()))
    assert np.isfinite(c) and c > 1e-3
    return c


def alone_on(ctx, rows, c, L=64, H=480):
    """a stand-alone limiter over the rows [N][n] in one call (the cutting changes no bit) -> (out, stats)"""
    from libear_amd import capi
    lim = capi.Limiter(ctx, rows.shape[0], c, L, H, max_samples=rows.shape[1])
    try:
        out, _ = run_device(ctx, lim, rows)
        return out, lim.stats()
    finally:
        lim.close()


@pytest.mark.parametrize("form", FORMS)
def test_attached_limiter_through_every_form_of_process_call(ctx, form):
    import torch
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    n = NBLOCKS * BLOCK
    r = make_renderer(ctx, M_OBJ, LAYOUT, BLOCK, NBLOCKS, scenes.ragged_curves(M_OBJ, N, 2 * n, seed=41))
    frames = pcm_model.random_frames(np.random.default_rng(43), "s16", 2 * n, M_OBJ)
    x = np.ascontiguousarray(pcm_model.rows(frames, "s16", 0, M_OBJ))
    lim = None
    cap = 2 * n
    sink = torch.full((N, cap + 3), 5.5, dtype=torch.float32, device="cuda")
    try:
        r.reset(0)
        plain = [run_form(form, ctx, r, x, frames, k) for k in range(2)]
        if form in TWIN:
            r.reset(0)
            rows = [run_form(TWIN[form], ctx, r, x, frames, k)[1] for k in range(2)]
        else:
            rows = [p[1] for p in plain]
        rows = np.concatenate(rows, axis=1)
        c = ceiling_for(rows)
        lim = capi.Limiter(ctx, N, c, 64, 480, max_samples=n)
        r.reset(0)
        r.attach_limiter(lim, sink.data_ptr(), cap + 3, cap)
        assert r.limiter_position() == 0
        attached = [run_form(form, ctx, r, x, frames, k) for k in range(2)]
        assert r.limiter_position() == cap
        ctx.synchronize()
        for a, b in zip(plain, attached):
            assert a[0].dtype == b[0].dtype and np.array_equal(bits(a[0]), bits(b[0])), form  # the render is untouched
        want, stats = alone_on(ctx, rows, c)
        assert stats[1] > 1000, "precondition: the bus is over the ceiling"
        got = sink.cpu().numpy()
        assert np.array_equal(bits(got[:, :cap]), bits(want)), form
        assert (got[:, cap:] == 5.5).all() and np.abs(got[:, :cap]).max() <= lm.guarantee(c)
        assert lim.stats() == stats
        # the render's reset leaves the limiter alone; attaching again rewinds the position
        r.reset(0)
        assert r.limiter_position() == cap and lim.stats() == stats
        r.attach_limiter(lim, sink.data_ptr(), cap + 3, cap)
        assert r.limiter_position() == 0
        assert r.scratch_regrows() == 0
    finally:
        r.attach_limiter(None)
        if lim is not None:
            lim.close()
        r.close()


def test_attached_limiter_a_long_host_call_that_runs_as_a_pipeline(ctx):
    import torch
    from libear_amd import capi
    M, B, T = 64, 512, 160
    N = len(LAYOUTS[LAYOUT])
    n = T * B
    assert M * n * 4 >= 16 << 20
    r = make_renderer(ctx, M, LAYOUT, B, T, scenes.ragged_curves(M, N, n, seed=45))
    x = scenes.audio(M, n, seed=46)
    sink = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    lim = None
    try:
        plain = r.process(x)
        assert r.last_host_chunks() > 1
        c = ceiling_for(plain)
        lim = capi.Limiter(ctx, N, c, 64, 480, max_samples=n)
        r.reset(0)
        r.attach_limiter(lim, sink.data_ptr(), n, n)
        out = r.process(x)
        assert r.last_host_chunks() > 1, "precondition: the call ran as a pipeline of chunks"
        assert np.array_equal(bits(plain), bits(out))
        assert r.limiter_position() == n  # once per sample
        ctx.synchronize()
        want, stats = alone_on(ctx, out, c)
        assert stats[1] > 1000 and np.array_equal(bits(sink.cpu().numpy()), bits(want)) and lim.stats() == stats
    finally:
        r.attach_limiter(None)
        if lim is not None:
            lim.close()
        r.close()


def test_attached_limiter_a_call_that_runs_as_two_spans(ctx):
    import torch
    from libear_amd import capi
    layout, M, B, T = "4+5+0", 96, 512, 257
    N = len(LAYOUTS[layout])
    n = T * B
    r = make_renderer(ctx, M, layout, B, T, scenes.dense_curves(M, N, B, T))
    x = torch.from_numpy(scenes.audio(M, n, seed=99)).cuda()
    sink = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    lim = None
    try:
        plain = torch.zeros((N, n), dtype=torch.float32, device="cuda")
        r.process_device(T, x.data_ptr(), n, plain.data_ptr(), n)
        ctx.synchronize()
        assert r.last_tail_blocks() > 0, "precondition: the call was cut into a main span and a tail"
        c = ceiling_for(plain.cpu().numpy())
        lim = capi.Limiter(ctx, N, c, 64, 480, max_samples=n)
        r.reset(0)
        r.attach_limiter(lim, sink.data_ptr(), n, n)
        out = torch.zeros((N, n), dtype=torch.float32, device="cuda")
        r.process_device(T, x.data_ptr(), n, out.data_ptr(), n)
        ctx.synchronize()
        assert r.last_tail_blocks() > 0 and torch.equal(plain, out) and r.limiter_position() == n
        want, stats = alone_on(ctx, out.cpu().numpy(), c)
        assert stats[1] > 1000 and np.array_equal(bits(sink.cpu().numpy()), bits(want)) and lim.stats() == stats
    finally:
        r.attach_limiter(None)
        if lim is not None:
            lim.close()
        r.close()


def test_a_meter_a_matrix_and_a_limiter_together_and_refused_calls(ctx):
    import torch
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    T, B, M = 10, 512, 64
    n = T * B
    x = scenes.audio(M, 2 * n, seed=78)
    h = (np.random.default_rng(9).uniform(-1, 1, (2, N, 700)) * np.exp(-np.arange(700) / 150.0)).astype(np.float32)
    r = make_renderer(ctx, M, LAYOUT, B, T, scenes.ragged_curves(M, N, 2 * n, seed=41))
    never = make_renderer(ctx, M, LAYOUT, B, T, scenes.ragged_curves(M, N, 2 * n, seed=41))
    fm = capi.FirMatrix(ctx, h, B, max_blocks=T)
    meter = capi.Loudness(ctx, N, 48000, max_steps=8, true_peak=True)
    c = 0.05
    lim = capi.Limiter(ctx, N, c, 64, 480, max_samples=n)
    short = capi.Limiter(ctx, N, c, 64, 480, max_samples=n - 1)
    narrow = capi.Limiter(ctx, N - 1, c, 64, 480, max_samples=n)
    other_ctx = capi.Context(0)
    foreign = capi.Limiter(other_ctx, N, c, 64, 480, max_samples=n)
    fsink = torch.zeros((2, 2 * n), dtype=torch.float32, device="cuda")
    lsink = torch.zeros((N, 2 * n), dtype=torch.float32, device="cuda")
    try:
        # the meter and the matrix without the limiter
        r.attach_loudness(meter)
        r.attach_fir_matrix(fm, fsink.data_ptr(), 2 * n, 2 * n)
        rows = [r.process(x[:, :n]), r.process(x[:, n:])]
        ctx.synchronize()
        steps, peaks, mix = meter.steps(), meter.peaks(), fsink.cpu().numpy().copy()
        assert (steps > 0).any() and peaks[0].max() > 2 * c and np.abs(mix).max() > 1e-3, "precondition: the bus is over the ceiling"
        # ... and with it: both still see the unlimited bus
        meter.reset(), fm.reset(), r.reset(0), fsink.zero_()
        r.attach_fir_matrix(fm, fsink.data_ptr(), 2 * n, 2 * n)
        r.attach_limiter(lim, lsink.data_ptr(), 2 * n, 2 * n)
        both = [r.process(x[:, :n]), r.process(x[:, n:])]
        ctx.synchronize()
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(rows, both))
        assert np.array_equal(bits(meter.steps()), bits(steps)) and all(np.array_equal(a, b) for a, b in zip(meter.peaks(), peaks))
        assert np.array_equal(bits(fsink.cpu().numpy()), bits(mix))
        want, stats = alone_on(ctx, np.concatenate(rows, axis=1), c)
        assert np.array_equal(bits(lsink.cpu().numpy()), bits(want)) and stats[1] > 1000
        r.attach_loudness(None)
        r.attach_fir_matrix(None)
        # room for one call and one block: the second call would pass sink_capacity, and nothing is rendered
        want = [never.process(x[:, :n]), never.process(x[:, n:])]
        r.reset(0)
        r.attach_limiter(lim, lsink.data_ptr(), 2 * n, n + B)
        assert np.array_equal(bits(r.process(x[:, :n])), bits(want[0]))
        with pytest.raises(capi.InvalidArgument):
            r.process(x[:, n:])
        assert r.limiter_position() == n
        r.attach_limiter(None)
        assert r.limiter_position() == 0
        assert np.array_equal(bits(r.process(x[:, n:])), bits(want[1])), "the refused call changed the render state"
        # a call longer than the limiter's max_samples, through two forms
        r.reset(0)
        r.attach_limiter(short, lsink.data_ptr(), 2 * n, 2 * n)
        xi = torch.from_numpy(np.ascontiguousarray(x[:, :n])).cuda()
        o = torch.zeros((N, n), dtype=torch.float32, device="cuda")
        for call in (lambda: r.process(x[:, :n]), lambda: r.process_device(T, xi.data_ptr(), n, o.data_ptr(), n)):
            with pytest.raises(capi.InvalidArgument):
                call()
        assert r.limiter_position() == 0 and short.stats() == (1.0, 0)
        r.attach_limiter(None)
        assert np.array_equal(bits(r.process(x[:, :n])), bits(want[0]))
        # wrong width, another context, no sink, a sink narrower than its capacity
        for args in ((narrow, lsink.data_ptr(), 2 * n, 2 * n), (foreign, lsink.data_ptr(), 2 * n, 2 * n), (lim, None, 2 * n, 2 * n),
                     (lim, lsink.data_ptr(), n, 2 * n)):
            with pytest.raises(capi.InvalidArgument):
                r.attach_limiter(*args)
    finally:
        r.attach_loudness(None)
        r.attach_fir_matrix(None)
        r.attach_limiter(None)
        for o in (lim, short, narrow, foreign, meter, fm, r, never, other_ctx):
            o.close()
