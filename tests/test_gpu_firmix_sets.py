"""Filter sets of the FIR filter matrix (include/earhip.h, group M, FILTER SETS) on the device: earhip_firmix_create_sets,
load_set, load_set_device, select.  The fade blocks are held to the bar of tests/firmix_model.py against the model of
tests/firmix_sets_model.py (e_device <= 1.5 e_cpu and e_cpu <= 1e-6 per output channel, over the fade blocks' samples only);
every steady block must have the BITS of a plain matrix (earhip_firmix_create) of that set fed the same calls — same ring, same
clock, same order of summation — which is what guards the steady path."""
import numpy as np
import pytest

import firmix_model as fm
import firmix_sets_model as fsm
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


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def run_calls(m, x, B, calls, before=None):
    """feeds x in `calls`; before(block index) runs before each call"""
    out, at = [], 0
    for nb in calls:
        if before:
            before(at)
        out.append(m.process(np.ascontiguousarray(x[:, at * B:(at + nb) * B])))
        at += nb
    assert at * B == x.shape[1]
    return np.concatenate(out, axis=1)


def plain_run(ctx, h, x, B, calls):
    from libear_amd import capi
    m = capi.FirMatrix(ctx, h, B, max_blocks=max(calls))
    try:
        return run_calls(m, x, B, calls)
    finally:
        m.close()


@pytest.mark.parametrize("name", list(fsm.SHAPES))
def test_shapes_fade_against_the_cpu_path_and_steady_blocks_by_bits(ctx, name):
    from libear_amd import capi
    C, K, J, B, T, calls, s, F = fsm.SHAPES[name]
    calls = fsm.cut_calls(calls, s)
    x, h0, h1, want, e_cpu = fsm.case(name)
    m = capi.FirMatrix(ctx, h0, B, max_blocks=max(calls), n_sets=2)
    try:
        assert m.state() == {"current": 0, "from": -1, "done": 0, "total": 0}
        assert m.set_info(0) == {"loaded": True, "pairs": int(np.any(h0 != 0, axis=2).sum())}
        assert m.set_info(1) == {"loaded": False, "pairs": 0}
        m.load_set(1, h1)
        assert m.set_info(1) == {"loaded": True, "pairs": int(np.any(h1 != 0, axis=2).sum())}
        assert m.info()["pairs"] == m.set_info(0)["pairs"]

        def before(block):
            if block == s:
                m.select(1, F)
                assert m.state() == {"current": 1, "from": 0, "done": 0, "total": F}
        got = run_calls(m, x, B, calls, before)
        assert m.state() == {"current": 1, "from": -1, "done": 0, "total": 0}
        assert m.info()["pairs"] == m.set_info(1)["pairs"]
    finally:
        m.close()
    fade = slice(s * B, (s + F) * B)
    fm.check_against_bar(got[:, fade], want[:, fade], e_cpu, f"{name} {fsm.SHAPES[name]}, fade blocks")
    assert same_bits(got[:, :s * B], plain_run(ctx, h0, x, B, calls)[:, :s * B]), "blocks before the select"
    assert same_bits(got[:, (s + F) * B:], plain_run(ctx, h1, x, B, calls)[:, (s + F) * B:]), "blocks after the fade"
    if name == "lists_differ":  # the last output has no pair in set 1: exactly +0.0 once set 1 alone is applied
        assert not bits(got[K - 1, (s + F) * B:]).any()


def test_a_matrix_with_sets_that_never_selects_has_the_bits_of_a_plain_one(ctx):
    from libear_amd import capi
    C, K, J, B, T, calls = fm.SHAPES["last_partition_one_tap"]
    x, h, _, _ = fm.case("last_partition_one_tap")
    m = capi.FirMatrix(ctx, h, B, max_blocks=max(calls), n_sets=3)
    try:
        got = run_calls(m, x, B, calls)
    finally:
        m.close()
    assert same_bits(got, plain_run(ctx, h, x, B, calls))


def test_a_hard_switch_gives_the_bits_of_the_new_set_fed_the_whole_stream(ctx):
    from libear_amd import capi
    C, K, J, B, T, calls, s, _ = fsm.SHAPES["across_calls"]
    x, h0, h1, _, _ = fsm.case("across_calls")
    m = capi.FirMatrix(ctx, h0, B, max_blocks=max(calls), n_sets=2)
    try:
        m.load_set(1, h1)

        def before(block):
            if block == s:
                m.select(1, 0)
                assert m.state() == {"current": 1, "from": -1, "done": 0, "total": 0}
        got = run_calls(m, x, B, calls, before)
    finally:
        m.close()
    assert same_bits(got[:, :s * B], plain_run(ctx, h0, x, B, calls)[:, :s * B])
    assert same_bits(got[:, s * B:], plain_run(ctx, h1, x, B, calls)[:, s * B:])


@pytest.mark.parametrize("device_taps", [False, True])
def test_ping_pong_loads_the_idle_set_while_blocks_are_in_flight(ctx, device_taps):
    """the head-tracking pattern: before each one-block call from the second on, fresh taps into the idle set (no synchronise by
    the caller) and select(idle, 1); every block but the first is a fade block between the two newest sets"""
    import torch
    from libear_amd import capi
    C, K, J, B, T = 3, 2, 150, 64, 8
    rng = np.random.default_rng(77)
    x = rng.uniform(-1.0, 1.0, (C, T * B)).astype(np.float32)
    hs = [fm.make_case(C, K, J, 1, 300 + t)[1] for t in range(T)]
    y64 = [fm.truth(x, h) for h in hs]
    ycpu = [fm.cpu_path(x, h, B) for h in hs]
    want, cpu = np.array(y64[0]), np.array(ycpu[0])
    for t in range(1, T):
        blk = slice(t * B, (t + 1) * B)
        want[:, blk] = (1.0 - fsm.gain(1, B, np.float64)) * y64[t - 1][:, blk] + fsm.gain(1, B, np.float64) * y64[t][:, blk]
        a = fsm.gain(1, B, np.float32)
        cpu[:, blk] = (np.float32(1) - a) * ycpu[t - 1][:, blk] + a * ycpu[t][:, blk]
    xin = torch.from_numpy(x).cuda()
    out = torch.zeros((K, T * B), dtype=torch.float32, device="cuda")
    dev = [torch.from_numpy(h).cuda() for h in hs] if device_taps else None
    m = capi.FirMatrix(ctx, hs[0], B, max_blocks=1, n_sets=2)
    try:
        ctx.synchronize()
        for t in range(T):
            if t:
                idle = t % 2
                assert m.state()["current"] == 1 - idle
                if device_taps:
                    m.load_set_device(idle, dev[t].data_ptr())
                    assert m.set_info(idle) == {"loaded": True, "pairs": K * C}
                else:
                    m.load_set(idle, hs[t])
                m.select(idle, 1)
            m.process_device(1, xin[:, t * B:].data_ptr(), T * B, out[:, t * B:].data_ptr(), T * B)
        ctx.synchronize()
        got = out.cpu().numpy()
    finally:
        m.close()
    for t in range(T):
        blk = slice(t * B, (t + 1) * B)
        fm.check_against_bar(got[:, blk], want[:, blk], fm.rel_err(cpu[:, blk], want[:, blk]),
                             f"ping-pong ({'device' if device_taps else 'host'} taps), block {t}")


# ---- attached to a renderer -------------------------------------------------------------------------------------------------
LAYOUT, M_OBJ, BLOCK, NBLOCKS, TAPS = "0+5+0", 64, 512, 3, 1024


def make_renderer(ctx, M, B, T, seed=41, total=None):
    from libear_amd import capi
    names = LAYOUTS[LAYOUT]
    r = capi.Renderer(ctx, M, len(names), B, capi.design_decorrelators(names), 255, max_blocks=T)
    for i, (t, d, f) in enumerate(scenes.ragged_curves(M, len(names), total or 2 * T * B, seed=seed)):
        r.set_object_points(i, t, d, f)
    r.commit()
    return r


def test_attached_to_a_renderer_select_between_two_calls(ctx):
    import torch
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    n = NBLOCKS * BLOCK
    x = scenes.audio(M_OBJ, 2 * n, seed=51)
    h0, h1 = fm.make_case(N, 2, TAPS, 1, 12)[1], fm.make_case(N, 2, TAPS, 1, 13)[1]
    r = make_renderer(ctx, M_OBJ, BLOCK, NBLOCKS)
    m = capi.FirMatrix(ctx, h0, BLOCK, max_blocks=NBLOCKS, n_sets=2)
    alone = capi.FirMatrix(ctx, h0, BLOCK, max_blocks=NBLOCKS, n_sets=2)
    sink = torch.zeros((2, 2 * n), dtype=torch.float32, device="cuda")
    try:
        plain = [r.process(x[:, :n]), r.process(x[:, n:])]
        r.reset(0)
        m.load_set(1, h1)
        alone.load_set(1, h1)
        r.attach_fir_matrix(m, sink.data_ptr(), 2 * n, 2 * n)
        rows = [r.process(x[:, :n])]
        m.select(1, 2)
        rows.append(r.process(x[:, n:]))
        assert m.state() == {"current": 1, "from": -1, "done": 0, "total": 0}
        ctx.synchronize()
        assert all(same_bits(a, b) for a, b in zip(plain, rows)), "the render's own outputs changed"
        want = [alone.process(rows[0])]
        alone.select(1, 2)
        want.append(alone.process(rows[1]))
        want = np.concatenate(want, axis=1)
        got = sink.cpu().numpy()
        assert np.abs(want).max() > 1e-3
        assert same_bits(got, want), np.abs(got - want).max()
        # and the fade did something: the second call differs from set 0 alone and from set 1 alone in its first two blocks
        alone.reset()
        alone.select(0, 0)
        only0 = np.concatenate([alone.process(v) for v in rows], axis=1)
        assert not same_bits(got[:, n:n + 2 * BLOCK], only0[:, n:n + 2 * BLOCK])
        assert same_bits(got[:, :n], only0[:, :n])
    finally:
        r.attach_fir_matrix(None)
        m.close()
        alone.close()
        r.close()


def test_attached_a_fade_that_crosses_a_chunk_boundary_of_a_pipelined_call(ctx):
    import torch
    from libear_amd import capi
    M, B, T, F = 61, 512, 140, 64
    N = len(LAYOUTS[LAYOUT])
    n = T * B
    assert 4 * M * n >= 16 << 20
    r = make_renderer(ctx, M, B, T, seed=45, total=n)
    x = scenes.audio(M, n, seed=46)
    h0, h1 = fm.make_case(N, 2, TAPS, 1, 14)[1], fm.make_case(N, 2, TAPS, 1, 15)[1]
    m = capi.FirMatrix(ctx, h0, B, max_blocks=T, n_sets=2)
    alone = capi.FirMatrix(ctx, h0, B, max_blocks=T, n_sets=2)
    sink = torch.zeros((2, n), dtype=torch.float32, device="cuda")
    ctx.set_option("HOST_CHUNK_MB", 4)
    try:
        plain = r.process(x)
        chunks = r.last_host_chunks()
        assert chunks >= 3 and T / chunks < F, "precondition: the first chunk is shorter than the fade"
        r.reset(0)
        m.load_set(1, h1)
        alone.load_set(1, h1)
        r.attach_fir_matrix(m, sink.data_ptr(), n, n)
        m.select(1, F)
        out = r.process(x)
        assert r.last_host_chunks() == chunks
        assert same_bits(plain, out)
        assert m.state() == {"current": 1, "from": -1, "done": 0, "total": 0}
        ctx.synchronize()
        got = sink.cpu().numpy()
        # the fade blocks against the model over the rows the call returned; the blocks behind it by bits
        fade = slice(0, F * B)  # (causal: the model needs no more than the fade's own samples)
        want = fsm.truth(out[:, fade], h0, h1, B, 0, F)
        cpu = fsm.cpu_path(out[:, fade], h0, h1, B, 0, F)
        fm.check_against_bar(got[:, fade], want[:, fade], fm.rel_err(cpu[:, fade], want[:, fade]),
                             f"attached, a fade of {F} blocks over a pipeline of {chunks} chunks")
        alone.select(1, F)
        assert same_bits(got[:, F * B:], alone.process(out)[:, F * B:])
    finally:
        ctx.set_option("HOST_CHUNK_MB", None)
        r.attach_fir_matrix(None)
        m.close()
        alone.close()
        r.close()


# ---- refusals and accepted calls --------------------------------------------------------------------------------------------
def small_sets(ctx, n_sets=3, max_blocks=2):
    from libear_amd import capi
    C, K, J, B = 3, 2, 100, 64
    x = np.random.default_rng(5).uniform(-1.0, 1.0, (C, 6 * B)).astype(np.float32)
    hs = [fm.make_case(C, K, J, 1, 400 + i)[1] for i in range(3)]
    return capi.FirMatrix(ctx, hs[0], B, max_blocks=max_blocks, n_sets=n_sets), x, hs, B


def test_refusals_leave_the_state_and_the_next_outputs_unchanged(ctx):
    from libear_amd import capi
    m, x, hs, B = small_sets(ctx)
    twin, _, _, _ = small_sets(ctx)
    try:
        for n_sets in (0, 4097, -1):
            with pytest.raises(capi.InvalidArgument):
                capi.FirMatrix(ctx, hs[0], B, n_sets=n_sets)
        for o in (m, twin):
            o.load_set(1, hs[1])

        def refused(call):
            before = m.state(), m.set_info(0), m.set_info(1), m.set_info(2)
            with pytest.raises(capi.InvalidArgument):
                call()
            assert (m.state(), m.set_info(0), m.set_info(1), m.set_info(2)) == before

        bad = hs[2].copy()
        bad[1, 2, 99] = np.nan
        refused(lambda: m.load_set(0, hs[2]))        # the current set
        refused(lambda: m.select(2, 1))              # an unloaded set
        refused(lambda: m.select(1, 65))             # F out of range
        refused(lambda: m.select(1, -1))
        refused(lambda: m.select(3, 1))              # a set index out of range
        refused(lambda: m.select(-1, 1))
        refused(lambda: m.load_set(3, hs[2]))
        refused(lambda: m.load_set(2, bad))          # a non-finite tap
        refused(lambda: m.set_info(3))
        assert same_bits(m.process(x[:, :B]), twin.process(x[:, :B]))
        for o in (m, twin):
            o.select(1, 3)
        assert same_bits(m.process(x[:, B:2 * B]), twin.process(x[:, B:2 * B]))
        assert m.state() == {"current": 1, "from": 0, "done": 1, "total": 3}
        refused(lambda: m.load_set(0, hs[2]))        # the set being faded from
        refused(lambda: m.load_set(1, hs[2]))        # the fade's target
        refused(lambda: m.select(0, 1))              # a select during a started fade
        refused(lambda: m.select(1, 0))
        m.load_set(2, hs[2])                         # the idle set may be loaded in mid-fade
        twin.load_set(2, hs[2])
        assert same_bits(m.process(x[:, 2 * B:4 * B]), twin.process(x[:, 2 * B:4 * B]))
        assert same_bits(m.process(x[:, 4 * B:]), twin.process(x[:, 4 * B:]))
        assert m.state() == {"current": 1, "from": -1, "done": 0, "total": 0}
        # a plain matrix has no sets to load or select
        p = capi.FirMatrix(ctx, hs[0], B)
        try:
            assert p.state() == {"current": 0, "from": -1, "done": 0, "total": 0}
            assert p.set_info(0) == {"loaded": True, "pairs": 6}
            for call in (lambda: p.load_set(0, hs[1]), lambda: p.select(0, 0), lambda: p.set_info(1)):
                with pytest.raises(capi.InvalidArgument):
                    call()
        finally:
            p.close()
    finally:
        m.close()
        twin.close()


def test_a_select_before_any_block_replaces_the_previous_one_and_selecting_the_current_set_is_a_no_op(ctx):
    m, x, hs, B = small_sets(ctx)
    twin, _, _, _ = small_sets(ctx)
    try:
        for o in (m, twin):
            o.load_set(1, hs[1])
            o.load_set(2, hs[2])
        m.select(0, 7)  # the current set, no fade running
        assert m.state() == {"current": 0, "from": -1, "done": 0, "total": 0}
        m.select(1, 5)
        m.select(2, 2)  # replaces it: from stays
        assert m.state() == {"current": 2, "from": 0, "done": 0, "total": 2}
        twin.select(2, 2)
        assert same_bits(m.process(x[:, :2 * B]), twin.process(x[:, :2 * B]))
        assert m.state() == {"current": 2, "from": -1, "done": 0, "total": 0}
        m.select(1, 4)
        m.select(2, 4)  # back to the set it would have left: nothing to fade
        assert m.state() == {"current": 2, "from": -1, "done": 0, "total": 0}
        assert same_bits(m.process(x[:, 2 * B:4 * B]), twin.process(x[:, 2 * B:4 * B]))
    finally:
        m.close()
        twin.close()


def test_reset_in_mid_fade_makes_the_target_current_and_equals_a_fresh_matrix_of_that_set(ctx):
    from libear_amd import capi
    m, x, hs, B = small_sets(ctx)
    fresh = capi.FirMatrix(ctx, hs[1], B, max_blocks=2)
    try:
        m.load_set(1, hs[1])
        m.process(x[:, :2 * B])
        m.select(1, 4)
        m.process(x[:, 2 * B:3 * B])
        assert m.state() == {"current": 1, "from": 0, "done": 1, "total": 4}
        m.reset()
        assert m.state() == {"current": 1, "from": -1, "done": 0, "total": 0}
        assert m.set_info(0)["loaded"] and m.set_info(1)["loaded"]
        got = np.concatenate([m.process(x[:, :2 * B]), m.process(x[:, 2 * B:4 * B])], axis=1)
        want = np.concatenate([fresh.process(x[:, :2 * B]), fresh.process(x[:, 2 * B:4 * B])], axis=1)
        assert same_bits(got, want)
    finally:
        m.close()
        fresh.close()


def test_a_nan_channel_reaches_no_output_while_no_set_in_use_has_a_pair_on_it(ctx):
    """against a plain matrix every channel is read; a channel without a pair in the sets applied is still never multiplied"""
    from libear_amd import capi
    C, K, J, B, T = 3, 2, 70, 64, 4
    x, h0 = fm.make_case(C, K, J, T * B, 61)
    h1 = fm.make_case(C, K, J, 1, 62)[1]
    h0[:, 2] = 0.0
    h1[:, 2] = 0.0
    xin = x.copy()
    xin[2] = np.nan
    m = capi.FirMatrix(ctx, h0, B, max_blocks=2, n_sets=2)
    try:
        m.load_set(1, h1)
        got = [m.process(xin[:, :2 * B])]
        m.select(1, 1)
        got.append(m.process(xin[:, 2 * B:]))
        got = np.concatenate(got, axis=1)
    finally:
        m.close()
    assert np.isfinite(got).all()
    want = fsm.truth(x, h0, h1, B, 2, 1)
    e_cpu = fm.rel_err(fsm.cpu_path(x, h0, h1, B, 2, 1), want)
    fm.check_against_bar(got, want, e_cpu, "a NaN channel without a pair in either set")
