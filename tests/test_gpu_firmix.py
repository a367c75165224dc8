"""The FIR filter matrix (include/earhip.h, group M) on the device: stand-alone against the bar of tests/firmix_model.py —
per output channel e = ||. - truth|| / ||truth||, e_device <= 1.5 e_cpu and e_cpu <= 1e-6, the CPU path being one libear
BlockConvolver per non-zero pair summed in float32 — and attached to a renderer (earhip_render_attach_firmix), where the sink
must hold the bits of a stand-alone matrix fed the rows the call returned.

Measured on an MI355X (worst output channel: e_device, e_cpu, ratio): see DESIGN.md section 5."""
import numpy as np
import pytest

import firmix_model as fm
import pcm_model
import scenes
from layouts import LAYOUTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from libear_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run_calls(m, x, B, calls):
    out, at = [], 0
    for nb in calls:
        out.append(m.process(np.ascontiguousarray(x[:, at * B:(at + nb) * B])))
        at += nb
    assert at * B == x.shape[1]
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("name", list(fm.SHAPES))
def test_shapes_against_the_cpu_path(ctx, name):
    from libear_amd import capi
    C, K, J, B, T, calls = fm.SHAPES[name]
    x, h, want, e_cpu = fm.case(name)
    m = capi.FirMatrix(ctx, h, B, max_blocks=max(calls))
    try:
        assert m.info() == {"n_in": C, "n_out": K, "block_size": B, "partitions": -(-J // B), "pairs": K * C}
        got = run_calls(m, x, B, calls)
        fm.check_against_bar(got, want, e_cpu, f"{name} {fm.SHAPES[name]}")
    finally:
        m.close()


@pytest.mark.parametrize("d", [0, 1, 63, 64, 65])
def test_a_delay_matrix_delays(ctx, d):
    from libear_amd import capi
    B, C, T = 64, 3, 4
    assert d in (0, 1, B - 1, B, B + 1)
    h = np.zeros((C, C, B + 2), np.float32)
    for k in range(C):
        h[k, k, d] = 1.0
    x = np.random.default_rng(d).uniform(-1.0, 1.0, (C, T * B)).astype(np.float32)
    m = capi.FirMatrix(ctx, h, B, max_blocks=T)
    try:
        got = m.process(x)
    finally:
        m.close()
    want = np.zeros_like(x)
    want[:, d:] = x[:, :x.shape[1] - d]
    worst = np.abs(got - want).max()
    print(f"delay {d}: worst absolute difference {worst:.3e}")
    assert worst <= 1e-6


def test_diagonal_with_a_nan_channel_and_an_output_without_a_pair(ctx):
    """diagonal 24 x 24 x 300 taps at B 128, 6 blocks, plus input channel 24 full of NaN and output 24, both without a pair"""
    from libear_amd import capi
    D, J, B, T = 24, 300, 128, 6
    x, hd = fm.make_case(D, 1, J, T * B, seed=31)
    h = np.zeros((D + 1, D + 1, J), np.float32)
    for k in range(D):
        h[k, k] = hd[0, k]
    xin = np.concatenate([x, np.full((1, T * B), np.nan, np.float32)])
    want = fm.truth(x, h[:D, :D])
    e_cpu = fm.rel_err(fm.cpu_path(x, h[:D, :D], B), want)
    m = capi.FirMatrix(ctx, h, B, max_blocks=4)
    try:
        assert m.info()["pairs"] == D
        got = run_calls(m, xin, B, (4, 2))
    finally:
        m.close()
    assert np.isfinite(got).all()
    fm.check_against_bar(got[:D], want, e_cpu, "diagonal 24 x 24 with a NaN channel")
    assert not bits(got[D]).any(), "an output without a pair must be +0.0"


def test_the_same_calls_give_the_same_bits_and_reset_equals_a_fresh_object(ctx):
    from libear_amd import capi
    C, K, J, B, T, calls = fm.SHAPES["last_partition_one_tap"]
    x, h, _, _ = fm.case("last_partition_one_tap")
    m = capi.FirMatrix(ctx, h, B, max_blocks=max(calls))
    fresh = capi.FirMatrix(ctx, h, B, max_blocks=max(calls))
    try:
        first = run_calls(m, x, B, calls)
        m.reset()
        again = run_calls(m, x, B, calls)
        assert np.array_equal(bits(first), bits(again))
        assert np.array_equal(bits(first), bits(run_calls(fresh, x, B, calls)))
    finally:
        m.close()
        fresh.close()


def test_strides_sentinels_and_a_call_beyond_max_blocks(ctx):
    import torch
    from libear_amd import capi
    C, K, J, B, T, _ = fm.SHAPES["taps_not_a_multiple"]
    x, h, want, e_cpu = fm.case("taps_not_a_multiple")
    nb = 2  # two calls of two blocks, the fifth block is not fed
    n = nb * B
    in_stride, out_stride = T * B + 7, n + 11
    xin = torch.full((C, in_stride), float("nan"), dtype=torch.float32, device="cuda")
    xin[:, :T * B] = torch.from_numpy(x.copy()).cuda()
    m = capi.FirMatrix(ctx, h, B, max_blocks=nb)
    try:
        got = []
        for call in range(2):
            out = torch.full((K + 2, out_stride), 123.25, dtype=torch.float32, device="cuda")
            # a call of max_blocks + 1 is refused and consumes nothing
            with pytest.raises(capi.InvalidArgument):
                m.process_device(nb + 1, xin.data_ptr(), in_stride, out[1].data_ptr(), out_stride)
            m.process_device(nb, xin[:, call * n:].data_ptr(), in_stride, out[1].data_ptr(), out_stride)
            ctx.synchronize()
            o = out.cpu().numpy()
            assert (o[0] == 123.25).all() and (o[K + 1] == 123.25).all(), "rows beside the call's were written"
            assert (o[1:K + 1, n:] == 123.25).all(), "samples behind the call's were written"
            got.append(o[1:K + 1, :n])
        got = np.concatenate(got, axis=1)
        fm.check_against_bar(got, want[:, :2 * n], fm.rel_err(fm.cpu_path(x[:, :2 * n], h, B), want[:, :2 * n]),
                             "strided device rows, two calls")
        with pytest.raises(capi.InvalidArgument):  # a stride shorter than the call
            m.process_device(nb, xin.data_ptr(), n - 1, out.data_ptr(), out_stride)
    finally:
        m.close()


def test_create_refuses_what_the_header_says(ctx):
    from libear_amd import capi
    ok = np.ones((2, 3, 100), np.float32)
    capi.FirMatrix(ctx, ok, 64, 1).close()
    bad_taps = ok.copy()
    bad_taps[1, 2, 50] = np.inf
    for taps, B, T in ((np.ones((2, 65, 4), np.float32), 64, 1), (np.ones((65, 2, 4), np.float32), 64, 1), (ok, 32, 1), (ok, 8192, 1),
                       (ok, 96, 1), (np.ones((1, 1, 64 * 64 + 1), np.float32), 64, 1), (ok, 64, 0), (bad_taps, 64, 1),
                       (np.ones((2, 3, 0), np.float32), 64, 1)):
        with pytest.raises(capi.InvalidArgument):
            capi.FirMatrix(ctx, taps, B, T)


# ---- attached to a renderer -------------------------------------------------------------------------------------------------
LAYOUT, M_OBJ, BLOCK, NBLOCKS, TAPS = "0+5+0", 64, 512, 3, 1024
FORMS = ["process_device", "process", "process_frames", "process_frames_pcm"]


def make_renderer(ctx, M, B, T, seed=41, total=None):
    from libear_amd import capi
    names = LAYOUTS[LAYOUT]
    r = capi.Renderer(ctx, M, len(names), B, capi.design_decorrelators(names), 255, max_blocks=T)
    for i, (t, d, f) in enumerate(scenes.ragged_curves(M, len(names), total or 2 * T * B, seed=seed)):
        r.set_object_points(i, t, d, f)
    r.commit()
    return r


def monitor_taps(N, K=2, J=TAPS, seed=9):
    return fm.make_case(N, K, J, 1, seed)[1]


def run_form(form, ctx, r, x, frames, call, nblocks):
    """one process call -> (what it handed back; the float32 rows [N][n] of that call, None where it hands back no floats)"""
    import torch
    n = nblocks * r.B
    xs, fs = np.ascontiguousarray(x[:, call * n:(call + 1) * n]), np.ascontiguousarray(frames[call * n:(call + 1) * n])
    if form == "process_device":
        xi = torch.from_numpy(xs).cuda()
        o = torch.zeros((r.N, n + 5), dtype=torch.float32, device="cuda")
        r.process_device(nblocks, xi.data_ptr(), n, o.data_ptr(), n + 5)
        ctx.synchronize()
        out = o.cpu().numpy()[:, :n]
        return out, out
    if form == "process":
        out = r.process(xs)
        return out, out
    if form == "process_frames":
        out = r.process_frames(fs, "s16")
        return out, out
    assert form == "process_frames_pcm"
    return r.process_frames_pcm(fs, "s16", out_fmt="s16", dither=True, seed=77), None


@pytest.mark.parametrize("form", FORMS)
def test_attached_matrix_through_every_form_of_process_call(ctx, form):
    import torch
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    n = NBLOCKS * BLOCK
    r = make_renderer(ctx, M_OBJ, BLOCK, NBLOCKS)
    frames = pcm_model.random_frames(np.random.default_rng(43), "s16", 2 * n, M_OBJ)
    x = np.ascontiguousarray(pcm_model.rows(frames, "s16", 0, M_OBJ))
    h = monitor_taps(N)
    m = capi.FirMatrix(ctx, h, BLOCK, max_blocks=NBLOCKS)
    alone = capi.FirMatrix(ctx, h, BLOCK, max_blocks=NBLOCKS)
    cap = 2 * n
    pinned = form == "process"  # one form with the sink in earhip_host_alloc memory, read without a copy call
    sink = ctx.pinned_array((2, cap + 3)) if pinned else torch.full((2, cap + 3), 5.5, dtype=torch.float32, device="cuda")
    if pinned:
        sink[...] = 5.5
    try:
        r.reset(0)
        plain = [run_form(form, ctx, r, x, frames, k, NBLOCKS) for k in range(2)]
        if form == "process_frames_pcm":  # its float samples are those of process_frames, says the header
            r.reset(0)
            rows = [run_form("process_frames", ctx, r, x, frames, k, NBLOCKS)[1] for k in range(2)]
        else:
            rows = [p[1] for p in plain]
        assert all(np.isfinite(v).all() and np.abs(v).max() > 1e-3 for v in rows)
        r.reset(0)
        r.attach_fir_matrix(m, sink.ctypes.data if pinned else sink.data_ptr(), cap + 3, cap)
        assert r.fir_matrix_position() == 0
        attached = [run_form(form, ctx, r, x, frames, k, NBLOCKS) for k in range(2)]
        assert r.fir_matrix_position() == 2 * n
        ctx.synchronize()
        for a, b in zip(plain, attached):
            assert a[0].dtype == b[0].dtype and np.array_equal(bits(a[0]), bits(b[0])), form  # the render is untouched
        got = np.array(sink) if pinned else sink.cpu().numpy()
        want = np.concatenate([alone.process(v) for v in rows], axis=1)
        assert np.abs(want).max() > 1e-3
        assert np.array_equal(bits(got[:, :cap]), bits(want)), (form, np.abs(got[:, :cap] - want).max())
        assert (got[:, cap:] == 5.5).all()
        # the render's reset leaves the matrix alone; attaching again rewinds the position
        r.reset(0)
        assert r.fir_matrix_position() == 2 * n
        r.attach_fir_matrix(m, sink.ctypes.data if pinned else sink.data_ptr(), cap + 3, cap)
        assert r.fir_matrix_position() == 0
    finally:
        r.attach_fir_matrix(None)
        m.close()
        alone.close()
        r.close()
        if pinned:
            ctx.release(sink)


def test_attached_matrix_a_long_host_call_that_runs_as_a_pipeline(ctx):
    import torch
    from libear_amd import capi
    M, B, T = 61, 512, 140
    N = len(LAYOUTS[LAYOUT])
    n = T * B
    assert 4 * M * n >= 16 << 20
    r = make_renderer(ctx, M, B, T, seed=45, total=n)
    x = scenes.audio(M, n, seed=46)
    h = monitor_taps(N, seed=10)
    m = capi.FirMatrix(ctx, h, B, max_blocks=T)
    sink = torch.zeros((2, n), dtype=torch.float32, device="cuda")
    ctx.set_option("HOST_CHUNK_MB", 4)
    try:
        plain = r.process(x)
        assert r.last_host_chunks() >= 3
        r.reset(0)
        r.attach_fir_matrix(m, sink.data_ptr(), n, n)
        out = r.process(x)
        assert r.last_host_chunks() >= 3, "precondition: the call ran as a pipeline of chunks"
        assert np.array_equal(bits(plain), bits(out))
        assert r.fir_matrix_position() == n  # once per sample
        ctx.synchronize()
        want = fm.truth(out, h)
        e_cpu = fm.rel_err(fm.cpu_path(out, h, B), want)
        fm.check_against_bar(sink.cpu().numpy(), want, e_cpu, f"attached, pipeline of {r.last_host_chunks()} chunks")
    finally:
        ctx.set_option("HOST_CHUNK_MB", None)
        r.attach_fir_matrix(None)
        m.close()
        r.close()


def test_refused_calls_leave_the_render_untouched_and_wrong_matrices_are_refused(ctx):
    import torch
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    n = NBLOCKS * BLOCK
    x = scenes.audio(M_OBJ, 2 * n, seed=77)
    h = monitor_taps(N)
    m = capi.FirMatrix(ctx, h, BLOCK, max_blocks=NBLOCKS)
    short = capi.FirMatrix(ctx, h, BLOCK, max_blocks=NBLOCKS - 1)
    sink = torch.zeros((2, 2 * n), dtype=torch.float32, device="cuda")
    r = make_renderer(ctx, M_OBJ, BLOCK, NBLOCKS)
    never = make_renderer(ctx, M_OBJ, BLOCK, NBLOCKS)
    other_ctx = capi.Context(0)
    try:
        want = [never.process(x[:, :n]), never.process(x[:, n:])]
        # room for one call and one block: the second call would pass sink_capacity
        r.attach_fir_matrix(m, sink.data_ptr(), 2 * n, n + BLOCK)
        assert np.array_equal(bits(r.process(x[:, :n])), bits(want[0]))
        with pytest.raises(capi.InvalidArgument):
            r.process(x[:, n:])
        assert r.fir_matrix_position() == n
        r.attach_fir_matrix(None)
        assert np.array_equal(bits(r.process(x[:, n:])), bits(want[1])), "the refused call changed the render state"
        # a call longer than the matrix's max_blocks
        r.reset(0)
        r.attach_fir_matrix(short, sink.data_ptr(), 2 * n, 2 * n)
        with pytest.raises(capi.InvalidArgument):
            r.process(x[:, :n])
        assert r.fir_matrix_position() == 0
        r.attach_fir_matrix(None)
        assert np.array_equal(bits(r.process(x[:, :n])), bits(want[0]))
        # wrong n_in, wrong block size, another context
        for taps, B, c in ((monitor_taps(N + 1), BLOCK, ctx), (h, BLOCK // 2, ctx), (h, BLOCK, other_ctx)):
            wrong = capi.FirMatrix(c, taps, B, max_blocks=NBLOCKS)
            try:
                with pytest.raises(capi.InvalidArgument):
                    r.attach_fir_matrix(wrong, sink.data_ptr(), 2 * n, 2 * n)
            finally:
                wrong.close()
    finally:
        r.attach_fir_matrix(None)
        m.close()
        short.close()
        r.close()
        never.close()
        other_ctx.close()


def test_a_meter_and_a_matrix_together(ctx):
    import torch
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    T = 10
    n = T * BLOCK
    assert 2 * n // 4800 >= 2
    x = scenes.audio(M_OBJ, 2 * n, seed=78)
    h = monitor_taps(N)
    r = make_renderer(ctx, M_OBJ, BLOCK, T)
    m = capi.FirMatrix(ctx, h, BLOCK, max_blocks=T)
    alone = capi.FirMatrix(ctx, h, BLOCK, max_blocks=T)
    meter = capi.Loudness(ctx, N, 48000, max_steps=8)
    sink = torch.zeros((2, 2 * n), dtype=torch.float32, device="cuda")
    try:
        r.attach_loudness(meter)
        rows = [r.process(x[:, :n]), r.process(x[:, n:])]
        only = meter.steps()
        assert only.shape == (2 * n // 4800, N) and (only > 0).any()
        meter.reset()
        r.reset(0)
        r.attach_fir_matrix(m, sink.data_ptr(), 2 * n, 2 * n)
        both = [r.process(x[:, :n]), r.process(x[:, n:])]
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(rows, both))
        assert np.array_equal(bits(meter.steps()), bits(only))
        want = np.concatenate([alone.process(v) for v in rows], axis=1)
        assert np.array_equal(bits(sink.cpu().numpy()), bits(want))
    finally:
        r.attach_loudness(None)
        r.attach_fir_matrix(None)
        meter.close()
        m.close()
        alone.close()
        r.close()


def test_the_host_form_never_looks_at_the_row_of_a_channel_without_a_pair(ctx):
    """include/earhip.h, group M: the pointer of an input channel that is never read is not looked at.  3 -> 2 at B = 64, 2 blocks, input 2
    without a pair, through the library's own symbols (the wrapper cannot pass a NULL row): a NULL pointer there gives the bits
    of a NaN row there; a NULL pointer of a channel that is read is EARHIP_INVALID_ARGUMENT and consumes nothing"""
    import ctypes as C
    from libear_amd import capi
    lib = capi.load()
    B, T = 64, 2
    rng = np.random.default_rng(77)
    h = rng.uniform(-0.1, 0.1, (2, 3, B + 7)).astype(np.float32)
    h[:, 2] = 0.0
    x = rng.uniform(-1.0, 1.0, (3, T * B)).astype(np.float32)
    x[2] = np.nan

    def call(m, null_row):
        rows = capi._chan_ptrs(x)
        if null_row is not None:
            rows[null_row] = None
        out = np.full((2, T * B), 7.5, np.float32)
        return lib.earhip_firmix_process(m.h, C.c_size_t(T), rows, capi._chan_ptrs(out)), out

    m, fresh = capi.FirMatrix(ctx, h, B, max_blocks=T), capi.FirMatrix(ctx, h, B, max_blocks=T)
    try:
        assert m.info()["pairs"] == 4
        rc, with_nan = call(fresh, None)
        assert rc == capi.OK and np.isfinite(with_nan).all()
        rc, untouched = call(m, 1)  # a channel that is read
        assert rc == capi.INVALID_ARGUMENT and (untouched == 7.5).all()
        rc, with_null = call(m, 2)  # the next valid call: a fresh matrix's bits, the unread row's pointer NULL
        assert rc == capi.OK, lib.earhip_last_error()
        assert np.array_equal(bits(with_null), bits(with_nan))
    finally:
        m.close()
        fresh.close()
