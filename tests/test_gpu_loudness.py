"""The programme loudness meter (include/earhip.h, group L: ITU-R BS.1770-4) on the GPU: stand-alone over device and host rows,
and attached to a renderer through every form of process call.

The reference of every comparison is the float64 model (tests/loudness_model.py) run on the float32 samples the meter saw.
Step energies everywhere under the bound |z - z_model| <= 1e-9 z_model + 1e-18 Z_c (lm.within_bound); every test prints the
worst relative difference it measured before it asserts.  Measured on an MI355X: see DESIGN.md section 5."""
import numpy as np
import pytest

import loudness_model as lm
import pcm_model
import scenes
from layouts import LAYOUTS

pytestmark = pytest.mark.gpu

RATE, STEP, CHUNK = 48000, 4800, 240


@pytest.fixture(scope="module")
def ctx():
    from libear_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def check_steps(got, samples, what):
    want = lm.step_energies(samples)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok, worst = lm.within_bound(got, want)
    print(f"{what}: {got.shape[0]} steps x {got.shape[1]} channels, worst relative difference {worst:.3e} "
          f"({worst / 1e-9:.2%} of the bound)")
    assert ok, (what, worst)
    return want


def standalone_rows(n, channels=24, seed=5):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    x = np.zeros((channels, n), np.float32)
    freqs = np.geomspace(20.0, 20000.0, channels)
    for c in range(channels):
        kind = c % 6
        if kind == 0:
            x[c] = rng.uniform(-0.7, 0.7, n)
        elif kind == 1:
            x[c] = 0.5 * np.sin(2 * np.pi * freqs[c] * t)
        elif kind == 2:
            x[c] = 0.3 + 0.2 * np.sin(2 * np.pi * freqs[c] * t)  # DC offset
        elif kind == 3:
            x[c] = rng.uniform(-0.5, 0.5, n)
            x[c, n // 5:n // 5 + 30_000] = 0.0  # digital silence after a signal
            x[c, n // 2:n // 2 + 4801] = 0.0
        elif kind == 4:
            x[c] = 1e-4 * rng.uniform(-0.5, 0.5, n)  # 80 dB down
        else:
            x[c] = 0.25 * np.sin(2 * np.pi * freqs[c] * t) - 0.125
    x[channels - 1] = 0.4 * np.sin(2 * np.pi * 20000.0 * t)
    x[1] = 0.4 * np.sin(2 * np.pi * 20.0 * t)
    return x


def test_standalone_meter_any_cutting_and_determinism(ctx):
    import torch
    from libear_amd import capi
    n, extra, C_ = 10 * RATE + 1234, STEP - 1234, 24
    x = standalone_rows(n + extra)
    stride = n + extra + 37
    dev = torch.zeros((C_, stride), dtype=torch.float32, device="cuda")
    dev[:, :n + extra] = torch.from_numpy(x).cuda()
    rng = np.random.default_rng(17)
    cuts = [1, 0, CHUNK - 1, CHUNK + 1, 200_000, 0, 2]
    while sum(cuts) < n - 200_000:
        cuts.append(int(rng.integers(1, 200_001)))
    cuts.append(n - sum(cuts))
    small = [int(v) for v in rng.integers(1, 700, size=40)]
    cuts2 = small + [n - sum(small)]
    m = capi.Loudness(ctx, C_, RATE, max_steps=200)
    try:
        results = {}
        for name, calls in (("one call", [n]), ("random calls", cuts), ("short calls first", cuts2)):
            runs = []
            for _ in range(2):
                m.reset()
                at = 0
                for k in calls:
                    m.process_device(k, dev.data_ptr() + 4 * at, stride)
                    at += k
                assert at == n
                assert m.num_steps() == 100
                runs.append(m.steps())
            assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64)), name  # determinism: the same bits
            check_steps(runs[0], x[:, :n], f"stand-alone meter, {name}")
            results[name] = runs[0]
        # the 1,234 samples behind step 99 were held back: they are the start of step 100
        m.process_device(extra, dev.data_ptr() + 4 * n, stride)
        assert m.num_steps() == 101
        check_steps(m.steps(), x, "stand-alone meter, the held-back samples completed")
        same = np.array_equal(results["one call"].view(np.uint64), results["random calls"].view(np.uint64))
        print(f"bit-identical across cuttings (welcome, not required): {same}")
        # host rows: pieces through the staging buffer
        m.reset()
        m.process(x[:, :70_000])
        m.process(x[:, 70_000:n])
        assert m.num_steps() == 100
        check_steps(m.steps(), x[:, :n], "stand-alone meter, host rows")
        # result() is the gating of those steps
        w = np.where(np.arange(C_) % 5 == 0, 1.41, 1.0)
        want = lm.gate(lm.step_energies(x[:, :n]), w)
        got = m.result(w)
        assert all(abs(g - v) <= 1e-6 for g, v in zip(got, want)), (got, want)
        assert got == capi.loudness_gate(m.steps(), w)
    finally:
        m.close()


def test_a_call_beyond_max_steps_is_refused_and_changes_nothing(ctx):
    import torch
    from libear_amd import capi
    C_, n = 3, 8 * STEP
    x = standalone_rows(n, C_, seed=9)
    dev = torch.from_numpy(x).cuda()
    a, b = capi.Loudness(ctx, C_, RATE, max_steps=6), capi.Loudness(ctx, C_, RATE, max_steps=10)
    try:
        first = 5 * STEP + 100
        for m in (a, b):
            m.process_device(first, dev.data_ptr(), n)
        before = a.steps()
        with pytest.raises(capi.InvalidArgument):
            a.process_device(2 * STEP, dev.data_ptr() + 4 * first, n)  # would finish step 7 of 6
        with pytest.raises(capi.InvalidArgument):
            a.process(x[:, first:first + 2 * STEP])
        assert a.num_steps() == 5 and np.array_equal(a.steps().view(np.uint64), before.view(np.uint64))
        for m in (a, b):
            m.process_device(STEP - 100, dev.data_ptr() + 4 * first, n)  # exactly to the end of step 6
        assert a.num_steps() == 6
        assert np.array_equal(a.steps().view(np.uint64), b.steps().view(np.uint64))  # the state was not touched either
        check_steps(a.steps(), x[:, :6 * STEP], "capacity")
        with pytest.raises(capi.InvalidArgument):
            a.process_device(STEP, dev.data_ptr(), n)
        a.process_device(STEP - 1, dev.data_ptr(), n)  # an unfinished step needs no room
        assert a.num_steps() == 6
    finally:
        a.close()
        b.close()


def test_create_refuses_what_the_header_says(ctx):
    from libear_amd import capi
    with pytest.raises(capi.InvalidArgument):
        capi.Loudness(ctx, 2, 44100)  # built-in coefficients are those of 48 kHz
    with pytest.raises(capi.InvalidArgument):
        capi.Loudness(ctx, 2, 48001, coeffs=lm.COEFFS)
    with pytest.raises(capi.InvalidArgument):
        capi.Loudness(ctx, 0)
    m = capi.Loudness(ctx, 2, 44100, max_steps=20, coeffs=lm.COEFFS)  # (a caller's coefficients at another rate: step 4410, chunks of 210)
    try:
        x = standalone_rows(44100, 2, seed=3)
        m.process(x)
        assert m.num_steps() == 10
        want = lm.step_energies(x, rate=44100)
        ok, worst = lm.within_bound(m.steps(), want)
        print(f"44100 Hz with the caller's coefficients: worst relative difference {worst:.3e}")
        assert ok
    finally:
        m.close()


# ---- attached to a renderer -----------------------------------------------------------------------------------------------------
M_OBJ, LAYOUT, BLOCK, NBLOCKS = 64, "0+5+0", 512, 120
FORMS = ["process_device", "process", "frames_planar", "frames_interleaved", "frames_device", "frames_pcm_s16_dither",
         "frames_pcm_s24", "frames_pcm_device"]


def make_renderer(ctx, M, layout, B, T, curves):
    from libear_amd import capi
    names = LAYOUTS[layout]
    r = capi.Renderer(ctx, M, len(names), B, capi.design_decorrelators(names), 255, max_blocks=T)
    for i, (t, d, f) in enumerate(curves):
        r.set_object_points(i, t, d, f)
    r.commit()
    return r


def run_form(form, ctx, r, x, frames, call):
    """one process call of `form` on call's blocks -> (what the call handed back, as an array for a bitwise comparison;
    the float32 samples [N][n] the meter must have seen, or None where the form hands back no floats)"""
    import torch
    B, N, M = r.B, r.N, r.M
    n = NBLOCKS * B
    xs, fs = x[:, call * n:(call + 1) * n], frames[call * n:(call + 1) * n]
    if form == "process_device":
        xi = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
        o = torch.zeros((N, n + 5), dtype=torch.float32, device="cuda")
        r.process_device(NBLOCKS, xi.data_ptr(), n, o.data_ptr(), n + 5)
        ctx.synchronize()
        out = o.cpu().numpy()[:, :n]
        return out, out
    if form == "process":
        out = r.process(np.ascontiguousarray(xs))
        return out, out
    if form == "frames_planar":
        out = r.process_frames(fs, "s16")
        return out, out
    if form == "frames_interleaved":
        out = r.process_frames(fs, "s16", interleaved_out=True)
        return out, np.ascontiguousarray(out.T)
    if form == "frames_device":
        fi = torch.from_numpy(np.ascontiguousarray(fs)).cuda()
        o = torch.zeros((N, n), dtype=torch.float32, device="cuda")
        r.process_frames_device(NBLOCKS, fi.data_ptr(), "s16", M, 0, o.data_ptr(), n, False)
        ctx.synchronize()
        out = o.cpu().numpy()
        return out, out
    if form == "frames_pcm_s16_dither":
        return r.process_frames_pcm(fs, "s16", out_fmt="s16", dither=True, seed=77), None
    if form == "frames_pcm_s24":
        return r.process_frames_pcm(fs, "s16", out_fmt="s24"), None
    assert form == "frames_pcm_device"
    fi = torch.from_numpy(np.ascontiguousarray(fs)).cuda()
    o = torch.zeros((n, N), dtype=torch.int16, device="cuda")
    r.process_frames_pcm_device(NBLOCKS, fi.data_ptr(), "s16", M, 0, o.data_ptr(), 2 * N, 0, "s16")
    ctx.synchronize()
    return o.cpu().numpy(), None


# the form whose float samples a PCM-out form converts: the same bits, says the header
TWIN = {"frames_pcm_s16_dither": "frames_interleaved", "frames_pcm_s24": "frames_interleaved", "frames_pcm_device": "frames_device"}


@pytest.mark.parametrize("form", FORMS)
def test_attached_meter_through_every_form_of_process_call(ctx, form):
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    n = NBLOCKS * BLOCK
    assert 2 * n // STEP >= 24 and n // STEP >= 12
    r = make_renderer(ctx, M_OBJ, LAYOUT, BLOCK, NBLOCKS, scenes.ragged_curves(M_OBJ, N, 2 * n, seed=41))
    rng = np.random.default_rng(43)
    frames = pcm_model.random_frames(rng, "s16", 2 * n, M_OBJ)
    x = np.ascontiguousarray(pcm_model.rows(frames, "s16", 0, M_OBJ))  # the same programme as planar float rows
    m = capi.Loudness(ctx, N, RATE, max_steps=64)
    try:
        # without the meter: the render's own output, and the float samples of the form (or of its twin)
        r.reset(0)
        plain = [run_form(form, ctx, r, x, frames, k) for k in range(2)]
        if form in TWIN:
            r.reset(0)
            samples = [run_form(TWIN[form], ctx, r, x, frames, k)[1] for k in range(2)]
        else:
            samples = [p[1] for p in plain]
        samples = np.concatenate(samples, axis=1)
        assert samples.shape == (N, 2 * n) and np.isfinite(samples).all() and np.abs(samples).max() > 1e-3
        # with it
        r.reset(0)
        r.attach_loudness(m)
        metered = [run_form(form, ctx, r, x, frames, k) for k in range(2)]
        for a, b in zip(plain, metered):
            assert a[0].dtype == b[0].dtype and np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)), form  # the render is untouched
        assert m.num_steps() == 2 * n // STEP
        want = check_steps(m.steps(), samples, f"attached, {form}")
        w = capi.loudness_layout_weights(LAYOUT)
        got, model = m.result(w), lm.gate(want, w)
        print(f"attached, {form}: integrated {got[0]:.6f} LKFS (model {model[0]:.6f}), momentary {got[1]:.6f}, short-term {got[2]:.6f}")
        assert np.isfinite(model[0]) and np.isfinite(model[1])
        assert all(abs(g - v) <= 1e-6 or (g == v) for g, v in zip(got, model)), (got, model)
        assert r.scratch_regrows() == 0
    finally:
        r.attach_loudness(None)
        m.close()
        r.close()


def test_attached_meter_a_long_host_call_that_runs_as_a_pipeline(ctx):
    from libear_amd import capi
    M, B, T = 64, 512, 160
    N = len(LAYOUTS[LAYOUT])
    n = T * B
    assert M * n * 4 >= 16 << 20
    r = make_renderer(ctx, M, LAYOUT, B, T, scenes.ragged_curves(M, N, n, seed=45))
    x = scenes.audio(M, n, seed=46)
    m = capi.Loudness(ctx, N, RATE, max_steps=64)
    try:
        plain = r.process(x)
        assert r.last_host_chunks() > 1
        r.reset(0)
        r.attach_loudness(m)
        out = r.process(x)
        assert r.last_host_chunks() > 1, "precondition: the call ran as a pipeline of chunks"
        assert np.array_equal(plain.view(np.uint32), out.view(np.uint32))
        assert m.num_steps() == n // STEP  # once per sample
        check_steps(m.steps(), out, f"attached, pipeline of {r.last_host_chunks()} chunks")
        assert r.scratch_regrows() == 0
    finally:
        r.attach_loudness(None)
        m.close()
        r.close()


def test_attached_meter_a_call_that_runs_as_two_spans(ctx):
    import torch
    from libear_amd import capi
    layout, M, B, T = "4+5+0", 96, 512, 257
    N = len(LAYOUTS[layout])
    n = T * B
    r = make_renderer(ctx, M, layout, B, T, scenes.dense_curves(M, N, B, T))
    x = torch.from_numpy(scenes.audio(M, n, seed=99)).cuda()
    m = capi.Loudness(ctx, N, RATE, max_steps=64)
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
        assert m.num_steps() == n // STEP  # once per sample
        check_steps(m.steps(), out.cpu().numpy(), f"attached, two spans (tail {r.last_tail_blocks()} blocks)")
        assert r.scratch_regrows() == 0
    finally:
        r.attach_loudness(None)
        m.close()
        r.close()


def test_detach_render_reset_and_no_allocation_in_process_calls(ctx):
    import torch
    from libear_amd import capi
    N = len(LAYOUTS[LAYOUT])
    T, B, M = 24, 512, 16
    n = T * B
    r = make_renderer(ctx, M, LAYOUT, B, T, scenes.ragged_curves(M, N, 8 * n, seed=51))
    x = torch.from_numpy(scenes.audio(M, n, seed=52)).cuda()
    o = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    m = capi.Loudness(ctx, N, RATE, max_steps=64)
    wrong_n = capi.Loudness(ctx, N + 1, RATE, max_steps=4)
    other = capi.Context(0)
    foreign = capi.Loudness(other, N, RATE, max_steps=4)
    try:
        for bad in (wrong_n, foreign):
            with pytest.raises(capi.InvalidArgument):
                r.attach_loudness(bad)
        r.attach_loudness(m)
        outs = []

        def call():
            r.process_device(T, x.data_ptr(), n, o.data_ptr(), n)
            ctx.synchronize()
            outs.append(o.cpu().numpy())

        call()
        free0 = torch.cuda.mem_get_info()[0]
        call()
        call()
        assert torch.cuda.mem_get_info()[0] == free0, "a process call with a meter attached allocated device memory"
        assert m.num_steps() == 3 * n // STEP
        # earhip_render_reset leaves the meter alone: its clock and steps go on
        r.reset(0)
        assert m.num_steps() == 3 * n // STEP
        call()
        assert m.num_steps() == 4 * n // STEP
        check_steps(m.steps(), np.concatenate(outs, axis=1), "attached, across a render reset")
        # detached: the steps stop growing
        r.attach_loudness(None)
        call()
        assert m.num_steps() == 4 * n // STEP
        # a call that would overflow the meter fails before anything is rendered
        small = capi.Loudness(ctx, N, RATE, max_steps=1)
        r.attach_loudness(small)
        o.fill_(-3.0)
        with pytest.raises(capi.InvalidArgument):
            r.process_device(T, x.data_ptr(), n, o.data_ptr(), n)
        with pytest.raises(capi.InvalidArgument):
            r.process(np.zeros((M, n), np.float32))
        ctx.synchronize()
        assert float(o.min()) == -3.0 and float(o.max()) == -3.0 and small.num_steps() == 0
        r.attach_loudness(None)
        small.close()
        assert r.scratch_regrows() == 0
    finally:
        r.attach_loudness(None)
        r.close()
        for v in (m, wrong_n, foreign):
            v.close()
        other.close()


def test_two_meters_over_channel_halves_equal_one_over_all(ctx):
    """what a multi-GPU render does after the reduce-scatter: every rank meters the channels it owns, the columns are joined
    and gated once (earhip_loudness_gate)"""
    import torch
    from libear_amd import capi
    C_, n = 24, 4 * RATE + 999
    x = standalone_rows(n, C_, seed=21)
    dev = torch.from_numpy(x).cuda()
    whole, lo, hi = capi.Loudness(ctx, C_, RATE, max_steps=50), capi.Loudness(ctx, 11, RATE, max_steps=50), capi.Loudness(ctx, 13, RATE, max_steps=50)
    try:
        for at, k in ((0, 100_001), (100_001, n - 100_001)):
            whole.process_device(k, dev.data_ptr() + 4 * at, n)
            lo.process_device(k, dev.data_ptr() + 4 * at, n)
            hi.process_device(k, dev.data_ptr() + 4 * (11 * n + at), n)
        joined = np.concatenate([lo.steps(), hi.steps()], axis=1)
        assert joined.shape == (40, C_)
        assert np.array_equal(joined.view(np.uint64), whole.steps().view(np.uint64))
        w = capi.loudness_layout_weights("9+10+3")
        assert capi.loudness_gate(joined, w) == whole.result(w)
        assert np.isfinite(whole.result(w)[0])
    finally:
        for v in (whole, lo, hi):
            v.close()
