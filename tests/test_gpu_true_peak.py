"""The true-peak meter and the loudness range (include/earhip.h, group L: ITU-R BS.1770-4 annex 2, EBU Tech 3342) on the GPU:
stand-alone over device and host rows, and attached to a renderer through every form of process call.

The reference of every comparison is the float64 model (tests/true_peak_model.py) run on the float32 samples the meter saw.
True peaks everywhere under the derived bound |tp - tp_model| <= (taps + 1) 2^-24 A X_c (tm.bound); sample peaks equal numpy's;
per-step and total peaks bit-identical however the stream was cut.  Every test prints the worst ratio to the bound it measured
before it asserts.  Measured on an MI355X: see DESIGN.md section 5."""
import numpy as np
import pytest

import loudness_model as lm
import pcm_model
import scenes
import true_peak_model as tm
from layouts import LAYOUTS
from test_gpu_loudness import FORMS, LAYOUT, M_OBJ, BLOCK, NBLOCKS, TWIN, make_renderer, run_form, standalone_rows

pytestmark = pytest.mark.gpu

RATE, STEP = 48000, 4800


@pytest.fixture(scope="module")
def ctx():
    from libear_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_peaks(m, samples, what, table=None, rate=RATE):
    """the meter's per-step and total peaks against the model on `samples` [C][n] (everything the meter has seen)"""
    want = tm.peaks(samples, table, rate)
    tp, sp = m.step_peaks()
    tot_tp, tot_sp = m.peaks()
    assert tp.shape == want["step_tp"].shape == sp.shape, (what, tp.shape, want["step_tp"].shape)
    assert np.array_equal(sp.astype(np.float64), want["step_sp"]), what  # sample peaks: exact
    assert np.array_equal(tot_sp.astype(np.float64), want["sp"]), what
    r = max(tm.worst_ratio(tp, want["step_tp"], table, want["sp"]), tm.worst_ratio(tot_tp, want["tp"], table, want["sp"]))
    print(f"{what}: {tp.shape[0]} steps x {tp.shape[1]} channels, worst true-peak error {r:.3f} of the bound; "
          f"largest true peak {float(np.max(tm.dbtp(tot_tp))):.3f} dBTP")
    assert r <= 1.0, (what, r)
    if tp.shape[0]:  # the totals are the maxima of the finished steps and of the open one
        assert np.all(tot_tp >= tp.max(axis=0)) and np.all(tot_sp >= sp.max(axis=0))
    return want


def overs_rows(n, channels=24, seed=5):
    """standalone_rows with channel 7 replaced by inter-sample overs: a quarter-rate sine at 45 degrees, amplitude 1.35"""
    x = standalone_rows(n, channels, seed)
    if channels > 7:
        x[7] = (1.35 * np.sin(2 * np.pi * np.arange(n) / 4.0 + np.pi / 4) * np.minimum(np.arange(n) / 2000.0, 1.0)).astype(np.float32)
    return x


def test_standalone_true_peak_any_cutting_bit_identical(ctx):
    import torch
    from libear_amd import capi
    n, extra, C_ = 10 * RATE + 1234, STEP - 1234, 24
    x = overs_rows(n + extra)
    stride = n + extra + 37
    dev = torch.zeros((C_, stride), dtype=torch.float32, device="cuda")
    dev[:, :n + extra] = torch.from_numpy(x).cuda()
    rng = np.random.default_rng(17)
    cuts = [1, 0, 11, 12, 2047, 2049, 200_000, 0, 2]
    while sum(cuts) < n - 200_000:
        cuts.append(int(rng.integers(1, 200_001)))
    cuts.append(n - sum(cuts))
    small = [int(v) for v in rng.integers(1, 700, size=40)]
    cuts2 = small + [n - sum(small)]
    m = capi.Loudness(ctx, C_, RATE, max_steps=200, true_peak=True)
    plain = capi.Loudness(ctx, C_, RATE, max_steps=200)
    try:
        runs = []
        for name, calls in (("one call", [n]), ("random calls", cuts), ("40 calls under 700 samples first", cuts2)):
            for rep in range(2):
                for v in (m, plain):
                    v.reset()
                    at = 0
                    for k in calls:
                        v.process_device(k, dev.data_ptr() + 4 * at, stride)
                        at += k
                    assert at == n and v.num_steps() == 100
                # the energies do not know of the peaks: a meter without true peak over the same calls holds the same bits
                assert np.array_equal(m.steps().view(np.uint64), plain.steps().view(np.uint64)), name
                w = np.where(np.arange(C_) % 5 == 0, 1.41, 1.0)
                assert m.result(w) == plain.result(w) and m.range(w) == plain.range(w) == capi.loudness_range(m.steps(), w)
                runs.append((name, m.step_peaks(), m.peaks()))
            want = check_peaks(m, x[:, :n], f"stand-alone, {name}")
        assert want["sp"][7] < 1.0 < want["tp"][7]  # the overs channel: only the true peak sees them
        assert m.peaks()[1][7] < 1.0 < m.peaks()[0][7]
        for name, sp_, tot in runs[1:]:
            for a, b in zip(sp_ + tot, runs[0][1] + runs[0][2]):
                assert np.array_equal(bits(a), bits(b)), name  # no cutting and no repeat changes a bit
        # the 1,234 samples behind step 99 were in the open step: completed, they are step 100
        m.process_device(extra, dev.data_ptr() + 4 * n, stride)
        assert m.num_steps() == 101
        check_peaks(m, x, "stand-alone, the open step completed")
        # host rows: pieces through the staging buffer, the same bits
        m.reset()
        m.process(x[:, :70_000])
        m.process(x[:, 70_000:n])
        assert m.num_steps() == 100
        for a, b in zip(m.step_peaks() + m.peaks(), runs[0][1] + runs[0][2]):
            assert np.array_equal(bits(a), bits(b))
    finally:
        m.close()
        plain.close()


@pytest.mark.parametrize("form", FORMS)
def test_attached_true_peak_through_every_form_of_process_call(ctx, form):
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    n = NBLOCKS * BLOCK
    r = make_renderer(ctx, M_OBJ, LAYOUT, BLOCK, NBLOCKS, scenes.ragged_curves(M_OBJ, N, 2 * n, seed=41))
    rng = np.random.default_rng(43)
    frames = pcm_model.random_frames(rng, "s16", 2 * n, M_OBJ)
    x = np.ascontiguousarray(pcm_model.rows(frames, "s16", 0, M_OBJ))
    m = capi.Loudness(ctx, N, RATE, max_steps=64, true_peak=True)
    try:
        r.reset(0)
        plain = [run_form(form, ctx, r, x, frames, k) for k in range(2)]
        if form in TWIN:
            r.reset(0)
            samples = [run_form(TWIN[form], ctx, r, x, frames, k)[1] for k in range(2)]
        else:
            samples = [p[1] for p in plain]
        samples = np.concatenate(samples, axis=1)
        assert samples.shape == (N, 2 * n) and np.isfinite(samples).all() and np.abs(samples).max() > 1e-3
        r.reset(0)
        r.attach_loudness(m)
        metered = [run_form(form, ctx, r, x, frames, k) for k in range(2)]
        for a, b in zip(plain, metered):
            assert a[0].dtype == b[0].dtype and np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)), form  # the render is untouched
        assert m.num_steps() == 2 * n // STEP  # once per sample
        check_peaks(m, samples, f"attached, {form}")
        ok, worst = lm.within_bound(m.steps(), lm.step_energies(samples))
        assert ok, worst
        assert r.scratch_regrows() == 0
    finally:
        r.attach_loudness(None)
        m.close()
        r.close()


def test_attached_true_peak_a_long_host_call_that_runs_as_a_pipeline(ctx):
    from libear_amd import capi
    M, B, T = 64, 512, 160
    N = len(LAYOUTS[LAYOUT])
    n = T * B
    r = make_renderer(ctx, M, LAYOUT, B, T, scenes.ragged_curves(M, N, n, seed=45))
    x = scenes.audio(M, n, seed=46)
    m = capi.Loudness(ctx, N, RATE, max_steps=64, true_peak=True)
    try:
        plain = r.process(x)
        assert r.last_host_chunks() > 1
        r.reset(0)
        r.attach_loudness(m)
        out = r.process(x)
        assert r.last_host_chunks() > 1, "precondition: the call ran as a pipeline of chunks"
        assert np.array_equal(plain.view(np.uint32), out.view(np.uint32))
        assert m.num_steps() == n // STEP
        check_peaks(m, out, f"attached, pipeline of {r.last_host_chunks()} chunks")
        assert r.scratch_regrows() == 0
    finally:
        r.attach_loudness(None)
        m.close()
        r.close()


def test_attached_true_peak_a_call_that_runs_as_two_spans(ctx):
    import torch
    from libear_amd import capi
    layout, M, B, T = "4+5+0", 96, 512, 257
    N = len(LAYOUTS[layout])
    n = T * B
    r = make_renderer(ctx, M, layout, B, T, scenes.dense_curves(M, N, B, T))
    x = torch.from_numpy(scenes.audio(M, n, seed=99)).cuda()
    m = capi.Loudness(ctx, N, RATE, max_steps=64, true_peak=True)
    try:
        plain = torch.zeros((N, n), dtype=torch.float32, device="cuda")
        r.process_device(T, x.data_ptr(), n, plain.data_ptr(), n)
        ctx.synchronize()
        assert r.last_tail_blocks() > 0, "precondition: the call was cut into a main span and a tail"
        r.reset(0)
        r.attach_loudness(m)
        out = torch.zeros((N, n), dtype=torch.float32, device="cuda")
        r.process_device(T, x.data_ptr(), n, out.data_ptr(), n)
        ctx.synchronize()
        assert r.last_tail_blocks() > 0
        assert torch.equal(plain, out)
        assert m.num_steps() == n // STEP
        check_peaks(m, out.cpu().numpy(), f"attached, two spans (tail {r.last_tail_blocks()} blocks)")
        assert r.scratch_regrows() == 0
    finally:
        r.attach_loudness(None)
        m.close()
        r.close()


def test_resets_capacity_and_no_allocation_in_process_calls(ctx):
    import torch
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    T, B, M = 24, 512, 16
    n = T * B
    r = make_renderer(ctx, M, LAYOUT, B, T, scenes.ragged_curves(M, N, 8 * n, seed=51))
    x = torch.from_numpy(scenes.audio(M, n, seed=52)).cuda()
    o = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    m = capi.Loudness(ctx, N, RATE, max_steps=3 * n // STEP + 1, true_peak=True)
    try:
        r.attach_loudness(m)
        outs = []

        def call():
            r.process_device(T, x.data_ptr(), n, o.data_ptr(), n)
            ctx.synchronize()
            outs.append(o.cpu().numpy())

        call()
        free0 = torch.cuda.mem_get_info()[0]
        call()
        assert torch.cuda.mem_get_info()[0] == free0, "a process call with a true-peak meter attached allocated device memory"
        # earhip_render_reset leaves history and peaks alone
        before = m.peaks()
        r.reset(0)
        after = m.peaks()
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after)) and before[0].max() > 0
        call()
        check_peaks(m, np.concatenate(outs, axis=1), "attached, across a render reset")
        # a call beyond max_steps is refused before anything is rendered and changes no peak
        before = m.step_peaks() + m.peaks()
        steps = m.num_steps()
        o.fill_(-3.0)
        with pytest.raises(capi.InvalidArgument):
            r.process_device(T, x.data_ptr(), n, o.data_ptr(), n)
        with pytest.raises(capi.InvalidArgument):
            m.process_device(2 * STEP, o.data_ptr(), n)
        ctx.synchronize()
        assert float(o.min()) == -3.0 and float(o.max()) == -3.0 and m.num_steps() == steps
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, m.step_peaks() + m.peaks()))
        # earhip_loudness_reset clears history and peaks: the same samples again give what a new meter gives
        r.attach_loudness(None)
        m.reset()
        assert m.num_steps() == 0 and not m.peaks()[0].any() and not m.peaks()[1].any()
        rows = torch.from_numpy(outs[0]).cuda()
        m.process_device(n, rows.data_ptr(), n)
        check_peaks(m, outs[0], "after earhip_loudness_reset")
        assert r.scratch_regrows() == 0
    finally:
        r.attach_loudness(None)
        r.close()
        m.close()


def test_nan_and_infinities(ctx):
    import torch
    from libear_amd import capi
    x = np.zeros((3, 2 * STEP + 100), np.float32)
    x[:, 100] = 0.5
    x[0, 200] = np.nan
    x[1, STEP + 50] = -np.inf
    x[2, STEP + 50], x[2, STEP + 53] = np.inf, -np.inf  # two infinities of opposite sign inside one window: some y are NaN
    x[2, 2 * STEP + 7] = -0.25
    dev = torch.from_numpy(x).cuda()
    m = capi.Loudness(ctx, 3, RATE, max_steps=4, true_peak=True)
    try:
        m.process_device(x.shape[1], dev.data_ptr(), x.shape[1])
        tp, sp = m.step_peaks()
        tot_tp, tot_sp = m.peaks()
        want = tm.peaks(x)
        assert np.array_equal(sp.astype(np.float64), want["step_sp"]) and np.array_equal(tot_sp.astype(np.float64), want["sp"])
        assert sp[0].tolist() == [0.5, 0.5, 0.5] and sp[1].tolist() == [0.0, np.inf, np.inf]
        assert np.isfinite(tp[0]).all() and (tp[0] >= 0.48).all()  # the NaN, and every y it touches, are ignored
        assert tp[1].tolist() == [0.0, np.inf, np.inf]
        assert tot_tp.tolist()[1:] == [np.inf, np.inf] and np.isfinite(tot_tp[0])
        assert tm.worst_ratio(tp[0], want["step_tp"][0], None, [0.5, 0.5, 0.5]) <= 1.0
    finally:
        m.close()


def test_a_callers_table_two_phases_at_96000(ctx):
    import torch
    from libear_amd import capi
    rng = np.random.default_rng(5)
    table = rng.uniform(-0.4, 0.4, (2, 24))
    table[:, 11] += 1.0
    rate, C_ = 96000, 5
    n = 3 * rate + 777
    x = overs_rows(n, C_, seed=8)
    x[3] = rng.uniform(-1.0, 1.0, n)
    dev = torch.from_numpy(x).cuda()
    m = capi.Loudness(ctx, C_, rate, max_steps=40, coeffs=lm.COEFFS, true_peak=(2, 24, table))
    d = capi.Loudness(ctx, C_, RATE, max_steps=80, true_peak=(4, 12, tm.default_table()))  # the default table, brought by the caller
    e = capi.Loudness(ctx, C_, RATE, max_steps=80, true_peak=True)
    try:
        runs = []
        for calls in ([n], [5, 23, 24, 255, 257, 100_000, n - 100_564]):
            m.reset()
            at = 0
            for k in calls:
                m.process_device(k, dev.data_ptr() + 4 * at, n)
                at += k
            assert at == n and m.num_steps() == 30
            runs.append(m.step_peaks() + m.peaks())
        check_peaks(m, x, "a caller's 2 x 24 table at 96 kHz", table, rate)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(*runs))
        for v in (d, e):
            v.process_device(n, dev.data_ptr(), n)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(d.step_peaks() + d.peaks(), e.step_peaks() + e.peaks()))
    finally:
        for v in (m, d, e):
            v.close()


def test_a_callers_4x12_table_at_1000_hz_steps_shorter_than_a_tile(ctx):
    """a step of 100 samples: a wave of k_true_peak_4x12 (512 samples) crosses several step boundaries, so samples beyond its
    first two steps go to the store one by one"""
    import torch
    from libear_amd import capi
    rng = np.random.default_rng(12)
    table = tm.default_table() * rng.uniform(0.8, 1.2, (4, 12))
    rate, C_ = 1000, 3
    n = 123 * 100 + 57
    x = rng.uniform(-1.0, 1.0, (C_, n)).astype(np.float32)
    x[1] *= np.sin(2 * np.pi * np.arange(n) / 777.0).astype(np.float32)  # steps of very different peaks
    x[2, 3000:9000] = 0.0
    dev = torch.from_numpy(x).cuda()
    m = capi.Loudness(ctx, C_, rate, max_steps=130, coeffs=lm.COEFFS, true_peak=(4, 12, table))
    try:
        runs = []
        for calls in ([n], [1, 99, 100, 511, 513, 2048, 5000, n - 8272], [7] * 40 + [n - 280]):
            m.reset()
            at = 0
            for k in calls:
                m.process_device(k, dev.data_ptr() + 4 * at, n)
                at += k
            assert at == n and m.num_steps() == 123
            runs.append(m.step_peaks() + m.peaks())
        check_peaks(m, x, "a caller's 4 x 12 table at 1000 Hz", table, rate)
        for other in runs[1:]:
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(other, runs[0]))
    finally:
        m.close()


def test_create_refuses_what_the_header_says(ctx):
    from libear_amd import capi
    ok = tm.default_table()
    with pytest.raises(capi.InvalidArgument):
        capi.Loudness(ctx, 2, 96000, coeffs=lm.COEFFS, true_peak=True)  # the built-in table is for 44100 and 48000
    for phases, taps in ((0, 12), (9, 12), (4, 0), (4, 65)):
        with pytest.raises(capi.InvalidArgument):
            capi.Loudness(ctx, 2, RATE, true_peak=(phases, taps, np.ones((max(phases, 1), max(taps, 1)))[:phases, :taps]))
    for bad in (np.nan, np.inf):
        t = ok.copy()
        t[2, 3] = bad
        with pytest.raises(capi.InvalidArgument):
            capi.Loudness(ctx, 2, RATE, true_peak=(4, 12, t))
    m = capi.Loudness(ctx, 2, 44100, max_steps=20, coeffs=lm.COEFFS, true_peak=True)  # 44100: allowed
    p = capi.Loudness(ctx, 2, RATE, max_steps=20)
    try:
        x = overs_rows(44100 + 50, 2, seed=3)
        m.process(x)
        assert m.num_steps() == 10
        check_peaks(m, x, "44100 Hz, the built-in table", None, 44100)
        # a meter made without true peak has no peaks to give
        p.process(x[:, :9600])
        for q in (p.peaks, p.step_peaks):
            with pytest.raises(capi.InvalidArgument):
                q()
        assert p.num_steps() == 2 and np.isfinite(p.steps()).all()
    finally:
        m.close()
        p.close()


def test_two_meters_over_channel_halves_equal_one_over_all(ctx):
    import torch
    from libear_amd import capi
    C_, n = 24, 4 * RATE + 999
    x = overs_rows(n, C_, seed=21)
    dev = torch.from_numpy(x).cuda()
    whole, lo, hi = (capi.Loudness(ctx, c, RATE, max_steps=50, true_peak=True) for c in (C_, 11, 13))
    try:
        for at, k in ((0, 100_001), (100_001, n - 100_001)):
            whole.process_device(k, dev.data_ptr() + 4 * at, n)
            lo.process_device(k, dev.data_ptr() + 4 * at, n)
            hi.process_device(k, dev.data_ptr() + 4 * (11 * n + at), n)
        for a, b, c in zip(lo.step_peaks() + lo.peaks(), hi.step_peaks() + hi.peaks(), whole.step_peaks() + whole.peaks()):
            joined = np.concatenate([a, b], axis=-1)
            assert joined.shape == c.shape and np.array_equal(bits(joined), bits(c))
        w = capi.loudness_layout_weights("9+10+3")
        joined = np.concatenate([lo.steps(), hi.steps()], axis=1)
        assert capi.loudness_range(joined, w) == whole.range(w)
    finally:
        for v in (whole, lo, hi):
            v.close()
