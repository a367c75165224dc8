"""The render path beyond 24 loudspeakers against libear (the CPU oracle) and a float64 evaluation: bus widths at which the gain
kernels run more than one column group (blockIdx.z > 0 in the split-operand and exact kernels, several groups per workgroup in the
slot and VALU kernels), the curve store pads its rows to 96 .. 768 columns, and K2, the output-bus taps and the frame converters
see more than 24 rows.  tests/wide_bus_cases.py has the cases and, written down from the planner's rules, the plan each must run;
tests/test_wide_bus_cpu.py the references' own figures and the column plans.

Every call of part (a) writes into a canary buffer of N + 2 rows of samples + 8 floats, filled with 7.0: rows N and N + 1 and the
8 floats behind every row's samples must still be 7.0 afterwards.  Bars (want: the oracle's render; truth: float64; e_lib =
rel_rms_per_channel(want, truth), e_gpu = rel_rms_per_channel(got, truth)):
  1. the plan of the call — kernel, tile, tiles, object splits across workgroups, list layout — is the one written down, and a
     hinge call was not handed to the lists standing by;
  2. every sample finite;
  3. rel_rms_per_channel(got, want) <= 1e-6;
  4. e_gpu <= max(1.25 e_lib, 1e-6);
  5. every sample within 1e-5 of its channel's largest magnitude of the oracle's (tests/test_gpu_gain_ref.py);
  6. the roll call (family `integer`): np.array_equal with the int64 answer;
  7. strict mode: kernel 0, bit for bit the oracle's — where the output is the gain stage's: one bus (every column plan of the table
     runs as one bus of that many columns too), and the roll call beside a silent diffuse bus.  Behind a diffuse bus the device's FFT
     rounds differently from the CPU's, strict mode or not: there the bar of test_strict_full_chain_matches_oracle_closely
     (tests/test_gpu_render.py), a relative RMS of 3e-7.
The figures of every case are printed; the last tests assert that every kernel kind ran at 50, 64 and 98 columns and print the
worst figures per kernel and width."""
import numpy as np
import pytest

import _oracle
import many_objects_cases as mc
import scenes
import wide_bus_cases as wc
from _hip import ctx, with_options

pytestmark = pytest.mark.gpu

CANARY, PAD = 7.0, 8
RAN = {}    # columns -> the kernel kinds the calls of part (a) reported
WORST = {}  # (kernel, columns) -> [e_gpu, e_lib, distance from the oracle, worst sample]


def make_renderer(s, M, N, block, buses, max_blocks):
    from libear_amd import capi
    r = capi.Renderer(ctx(), M, N, block, s.dec, s.delay, max_blocks=max_blocks)
    for m, (t, d, f) in enumerate(s.curves):
        r.set_object_points(m, t, d, f if buses == 2 else None)
    return r


def render_device(s, M, N, block, buses, calls):
    """the scene as calls of `calls` blocks each, from device memory into a canary buffer -> (output, what the last call ran)"""
    import torch
    total = block * sum(calls)
    stride = total + PAD
    r = make_renderer(s, M, N, block, buses, max(calls))
    try:
        xd = torch.from_numpy(s.x.copy()).cuda()
        yd = torch.full((N + 2, stride), CANARY, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ofs = 0
        for nb in calls:
            r.process_device(nb, xd.data_ptr() + 4 * ofs, total, yd.data_ptr() + 4 * ofs, stride)
            ofs += nb * block
        ctx().synchronize()
        y = yd.cpu().numpy()
        ran = dict(r.last_plan(), layout=r.last_list_layout())
        assert ran["kernel"] == r.gain_kernel()
        ran["standby"] = r.hinge_standby() if ran["kernel"] == mc.HINGE else False
    finally:
        r.close()
    assert np.all(y[N:] == CANARY), "rows behind the last loudspeaker's were written"
    assert np.all(y[:, total:] == CANARY), "samples behind a row's end were written"
    return y[:N, :total].copy(), ran


def render(case):
    return with_options(case.opts, lambda: render_device(wc.scene(case), case.M, case.layout, case.block, case.buses, [case.nblocks]))


def check_plan(case, ran):
    assert {k: ran[k] for k in case.plan} == case.plan, (case.id, ran)
    assert not ran["standby"], (case.id, ran)


def worst_channels(got, want, n=3):
    """(channel, relative RMS) of the channels furthest from `want`"""
    num = np.linalg.norm(got.astype(np.float64) - want, axis=1)
    den = np.maximum(np.linalg.norm(np.asarray(want, np.float64), axis=1), 1e-300)
    order = np.argsort(-num / den)[:n]
    return [(int(c), float(num[c] / den[c])) for c in order]


def check_bars(case, got, ran):
    s = wc.scene(case)
    assert np.isfinite(got).all(), case.id
    if case.family == "integer":
        bad = np.argwhere(got != s.answer)
        print(f"{case.id}: kernel {ran['kernel']} tile {ran['tile']} x {ran['ntiles']} gsplit {ran['gsplit']}: {len(bad)} samples off the answer")
        assert np.array_equal(got, s.answer), (case.id, ran, len(bad), bad[:6], [(got[c, i], s.answer[c, i]) for c, i in bad[:6]])
        return
    e_lib, e_gpu = scenes.rel_rms_per_channel(s.want, s.truth), scenes.rel_rms_per_channel(got, s.truth)
    d_cpu = scenes.rel_rms_per_channel(got, s.want)
    worst = mc.per_sample(got, s.want)
    print(f"{case.id}: kernel {ran['kernel']} tile {ran['tile']} x {ran['ntiles']} gsplit {ran['gsplit']}: e_gpu {e_gpu:.3g} e_lib {e_lib:.3g} "
          f"from the oracle {d_cpu:.3g} worst sample {worst:.3g}")
    w = WORST.setdefault((ran["kernel"], wc.columns(case)), [0.0, 0.0, 0.0, 0.0])
    w[:] = [max(a, b) for a, b in zip(w, (e_gpu, e_lib, d_cpu, worst))]
    assert d_cpu <= 1e-6, (case.id, d_cpu, worst_channels(got, s.want), ran)
    assert e_gpu <= max(1.25 * e_lib, 1e-6), (case.id, e_gpu, e_lib, ran)
    assert worst <= 1e-5, (case.id, worst, ran)


# ---- (a) every kernel at every width
@pytest.mark.parametrize("case", wc.CASES, ids=lambda c: c.id)
def test_gain_kernels_beyond_one_column_group(case):
    got, ran = render(case)
    RAN.setdefault(wc.columns(case), set()).add(ran["kernel"])
    check_plan(case, ran)
    check_bars(case, got, ran)


@pytest.mark.parametrize("case", wc.STRICT_CASES, ids=lambda c: c.id)
def test_strict_mode_bit_exact(case):
    """strict mode: the VALU kernel with ngroups waves per workgroup and nz super-groups, libear's own arithmetic bit for bit"""
    s = wc.scene(case)
    ctx().set_strict(True)
    try:
        got, ran = render(case)
    finally:
        ctx().set_strict(False)
    RAN.setdefault(wc.columns(case), set()).add(ran["kernel"])
    check_plan(case, ran)
    print(f"{case.id}: kernel {ran['kernel']} tile {ran['tile']} x {ran['ntiles']}: from the oracle {scenes.rel_rms_per_channel(got, s.want):.3g}")
    assert got.dtype == np.float32 and np.isfinite(got).all()
    if case.buses == 1 or case.family == "integer":
        assert np.array_equal(got, s.want), (case.id, worst_channels(got, s.want))
    else:  # (the decorrelators' FFT: bar 7)
        assert scenes.rel_rms(got, s.want) <= 3e-7, (case.id, scenes.rel_rms(got, s.want), worst_channels(got, s.want))
    if case.family == "integer":
        assert np.array_equal(got, s.answer)


# ---- (b) call partitions and state
def partitions(nblocks):
    return ([nblocks], [1] * nblocks, [1, nblocks - 1])


def render_host(s, M, N, block, buses, calls):
    """earhip_render_process from host rows, call by call"""
    r = make_renderer(s, M, N, block, buses, max(calls))
    try:
        out, ofs = [], 0
        for nb in calls:
            out.append(r.process(np.ascontiguousarray(s.x[:, ofs:ofs + nb * block])))
            ofs += nb * block
    finally:
        r.close()
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("family", ("grid", "holding", "ramping"))
@pytest.mark.parametrize("N", (32, 49))
def test_call_partitions_on_two_column_groups(N, family):
    """one stream of 4 blocks of 512 as one call, block by block and as [1, 3], from device rows and from host rows, on the library's
    own kernel choice: the double-buffered K2 state and the alternating level / mode / per-tile words with grid.z > 1.  As the
    partition tests of test_gpu_render.py: every partition within 1e-6 of the oracle (per channel here) and of the one call"""
    case = mc.Case(f"partition-{family}-{N}x2", "partition", 96, N, 2, 512, 4, family, wc.SEEDS[family] + N, {}, None)
    s = wc.scene(case)
    for how in (render_host, lambda *a: render_device(*a)[0]):
        first = None
        for calls in partitions(case.nblocks):
            got = how(s, case.M, N, case.block, 2, calls)
            d = scenes.rel_rms_per_channel(got, s.want)
            print(f"{case.id} {'host' if how is render_host else 'device'} {calls}: from the oracle {d:.3g}"
                  + ("" if first is None else f", from the one call {scenes.rel_rms_per_channel(got, first):.3g}"))
            assert np.isfinite(got).all() and d <= 1e-6, (case.id, calls, worst_channels(got, s.want))
            if first is None:
                first = got
            assert scenes.rel_rms_per_channel(got, first) <= 1e-6, (case.id, calls)


@pytest.mark.parametrize("N", (64, 98))
def test_call_partitions_strict_bit_exact(N):
    """strict mode, one bus of 64 / 98 columns (the column plans of 32 x 2 and 49 x 2; no FFT behind the gain stage): every partition
    bit for bit the oracle's, from device rows and from host rows"""
    case = mc.Case(f"partition-strict-{N}x1", "partition", 96, N, 1, 512, 4, "holding", wc.SEEDS["holding"] + N, {}, None)
    s = wc.scene(case)
    ctx().set_strict(True)
    try:
        for calls in partitions(case.nblocks):
            assert np.array_equal(render_host(s, case.M, N, case.block, 1, calls), s.want), (case.id, calls)
            assert np.array_equal(render_device(s, case.M, N, case.block, 1, calls)[0], s.want), (case.id, calls)
    finally:
        ctx().set_strict(False)


# ---- (d) the component forms
@pytest.mark.parametrize("m,n", ((7, 25), (64, 49), (32, 97)))
@pytest.mark.parametrize("strict", (True, False))
def test_gain_interp_matrix_wide(m, n, strict):
    """earhip_gain_interp (libear's LinearInterpMatrix) with more than 24 outputs: strict bit for bit, default within 1e-6"""
    from libear_amd import capi
    length = 1000
    rng = np.random.default_rng(m * 1000 + n)
    times = list(range(100, length, 100))
    vals = rng.uniform(0, 1, (len(times), m, n)).astype(np.float32)
    vals[2] = vals[1]  # one constant segment
    x = rng.uniform(-1, 1, (m, length)).astype(np.float32)
    want = _oracle.gain_interp("matrix", times, vals, x, [length])
    ctx().set_strict(strict)
    try:
        gi = capi.GainInterp(ctx(), m, n)
        try:
            gi.set_points(times, vals)
            got = np.concatenate([gi.process(0, x[:, :700]), gi.process(700, x[:, 700:])], axis=1)
        finally:
            gi.close()
    finally:
        ctx().set_strict(False)
    d = scenes.rel_rms_per_channel(got, want)
    print(f"gain_interp {m} -> {n} strict {strict}: from the oracle {d:.3g}")
    assert got.shape == (n, length) and np.isfinite(got).all()
    if strict:
        assert np.array_equal(got, want), worst_channels(got, want)
    else:
        assert d <= 1e-6, worst_channels(got, want)


@pytest.mark.parametrize("n", (25, 49))
def test_policies_one_to_n_wide(n):
    """apply_interp / apply_constant onto more than 24 outputs: no accumulation, bit for bit (tests/test_gpu_gain_interp.py)"""
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, (1, 300)).astype(np.float32)
    a, b = rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    out = np.full((n + 1, 300), CANARY, np.float32)
    ctx().apply_interp(x, out[:n], 0, 300, 150, 150, 450, a, b)  # (every sample inside the ramp: the policy alone extrapolates)
    want = _oracle.gain_interp("vector", [150, 450], np.stack([a, b]).reshape(2, 1, n), x[0], [300], t0=150)
    assert np.array_equal(out[:n], want) and np.all(out[n] == CANARY)
    out2 = np.full((n + 1, 300), CANARY, np.float32)
    ctx().apply_constant(x, out2[:n], 10, 290, a)
    assert np.all(out2[:, :10] == CANARY) and np.all(out2[:, 290:] == CANARY) and np.all(out2[n] == CANARY)
    assert np.array_equal(out2[:n, 10:290], a[:, None] * x[:, 10:290])


# ---- (c) rare paths with two column groups
RARE_N = 32
RARE_KERNELS = (("grid", {"EARHIP_MFMA": None, "EARHIP_H2_TILE": "256"}, mc.GRID, 256, None),
                ("pieces", {"EARHIP_MFMA": "5", "EARHIP_P2_TILE": "256", "EARHIP_P2_PAIRS": "0"}, mc.PIECES, 256, False),
                ("pieces", {"EARHIP_MFMA": "5", "EARHIP_P2_TILE": "256", "EARHIP_P2_PAIRS": "1"}, mc.PIECES, 256, True),
                ("hinge", {"EARHIP_MFMA": "6", "EARHIP_HG_TILE": "512"}, mc.HINGE, 512, False))
RARE_IDS = ("grid", "pieces-packed", "pieces-paired", "hinge")
QUIET = 2.0 ** -24          # the quiet objects' level against everybody else's: beyond the 20 binades of level_is_quiet (gain_kernels.h:188-193)
QUIET_SPEAKERS = (5, 20)    # their own loudspeakers: columns 5 | 37 (both in column group 0) and 20 | 52 (diffuse: group 1)
_rare = {}


def rare_scene(kind, path):
    """scenes.split_paths_scene on 32 loudspeakers and two buses (128 objects, 5 blocks of 256 rendered from sample 37; objects 17 and
    90 on curves off the grid: points inside tiles), `redo`: with its bursts 10^4 above the probed level; `quiet`: objects 0 and 1
    2^-24 below the others, each alone on a loudspeaker (what it renders there is all that loudspeaker plays)"""
    if (kind, path) not in _rare:
        curves, x = scenes.split_paths_scene(kind, RARE_N, path == "redo", 256)
        if path == "quiet":
            curves = scenes.solo_curves(curves, RARE_N, list(QUIET_SPEAKERS))
            x = x.copy()
            x[:len(QUIET_SPEAKERS)] *= np.float32(QUIET)
        _rare[(kind, path)] = mc.build_scene("rare", curves, x, mc.speakers(RARE_N), 2, scenes.SPLIT_PATHS["block"])
    return _rare[(kind, path)]


@pytest.mark.parametrize("path", ("inside", "redo", "quiet"))
@pytest.mark.parametrize("kind,opts,kernel,tile,paired", RARE_KERNELS, ids=RARE_IDS)
def test_rare_paths_on_two_column_groups(kind, opts, kernel, tile, paired, path):
    """The exact paths of the split-operand kernels with grid.z = 2 (32 loudspeakers x 2 buses), as test_split_kernels_exact_paths_vs_oracle
    runs them on one group: a curve point inside a tile (`inside`), the overflow redo (`redo`: without it the tile's totals are not
    finite, and so is the output), an object quiet enough for the exact path (`quiet`: on the split operands 2^-24 of the call's level
    keeps no low piece — its loudspeakers would miss 1e-6 by orders of magnitude, and a path that only column group 0 takes leaves
    loudspeaker 20 without its diffuse part).  A redo or a per-tile word that only blockIdx.z == 0 handles fails here.  The call
    is short: the wide form; the hinge call stays on the hinge kernel's own form.  Bars 2, 3 and 5."""
    from libear_amd import capi
    sp = scenes.SPLIT_PATHS
    s = rare_scene(kind, path)
    if path == "redo":  # (the bursts are there, where no probe reads them: scenes.split_paths_scene)
        assert np.abs(s.x).max() > 5e3 * np.median(np.abs(s.x))
    if path == "quiet":
        assert all(np.abs(s.x[q]).max() * 2.0 ** 21 < np.abs(s.x[len(QUIET_SPEAKERS):]).max() for q in range(len(QUIET_SPEAKERS)))

    def run():
        import torch
        c = capi.Context(0)  # (the kernel choice is read when a context is created)
        try:
            r = capi.Renderer(c, sp["m"], RARE_N, sp["block"], s.dec, s.delay, max_blocks=sp["nblocks"])
            try:
                for m, (t, d, f) in enumerate(s.curves):
                    r.set_object_points(m, t + sp["start"], d, f)
                r.reset(sp["start"])
                total = sp["block"] * sp["nblocks"]
                xd = torch.from_numpy(s.x.copy()).cuda()
                yd = torch.full((RARE_N + 2, total + PAD), CANARY, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                r.process_device(sp["nblocks"], xd.data_ptr(), total, yd.data_ptr(), total + PAD)
                c.synchronize()
                y = yd.cpu().numpy()
                ran = dict(r.last_plan(), lists=r.last_list_layout(), wide=r.wide_form())
                if kernel == mc.HINGE:
                    ran.update(standby=r.hinge_standby(), robust=r.hinge_robust())
            finally:
                r.close()
        finally:
            c.close()
        return y, ran

    y, ran = with_options(opts, run)
    total = sp["block"] * sp["nblocks"]
    got = y[:RARE_N, :total]
    d, worst = scenes.rel_rms_per_channel(got, s.want), mc.per_sample(got, s.want)
    print(f"rare {RARE_IDS[RARE_KERNELS.index((kind, opts, kernel, tile, paired))]} {path}: {ran}: from the oracle {d:.3g} worst sample {worst:.3g}")
    assert ran["kernel"] == kernel and ran["tile"] == tile and ran["lists"] == paired and ran["wide"] is True, ran
    if kernel == mc.HINGE:
        assert not ran["standby"] and not ran["robust"], ran
    assert np.all(y[RARE_N:] == CANARY) and np.all(y[:, total:] == CANARY)
    assert np.isfinite(got).all()
    assert d <= 1e-6, (d, worst_channels(got, s.want), ran)
    assert worst <= 1e-5, (worst, ran)


# ---- (e) behind the gain stage
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_meter_fir_matrix_and_limiter_on_a_bus_of_32():
    """one renderer of 32 loudspeakers with a meter, a 32 -> 2 FIR matrix and a limiter attached at once (the structure of
    test_a_meter_a_matrix_and_a_limiter_together_and_refused_calls, tests/test_gpu_limiter.py): the render is the bits of a renderer
    without taps, and every sink holds the bits of the stand-alone stage fed the rows the calls returned"""
    import torch
    import loudness_model as lm
    from libear_amd import capi
    c = ctx()
    N, M, B, T = 32, 96, 512, 3
    n = T * B
    case = mc.Case("taps-32x2", "taps", M, N, 2, B, 2 * T, "holding", wc.SEEDS["holding"] + N, {}, None)
    s = wc.scene(case)
    h = (np.random.default_rng(9).uniform(-1, 1, (2, N, 700)) * np.exp(-np.arange(700) / 150.0)).astype(np.float32)
    ceiling = 0.05
    made = []

    def make(v):
        made.append(v)
        return v
    try:
        r, never = (make(make_renderer(s, M, N, B, 2, T)) for _ in range(2))
        fm, fm2 = (make(capi.FirMatrix(c, h, B, max_blocks=2 * T)) for _ in range(2))
        # (a sample rate of 1280: a 100 ms step is 128 samples, a quarter of a block — as test_every_tap_refuses_..., test_gpu_render.py)
        meter, meter2 = (make(capi.Loudness(c, N, 1280, max_steps=64, coeffs=lm.COEFFS)) for _ in range(2))
        lim, lim2 = (make(capi.Limiter(c, N, ceiling, 64, 480, max_samples=2 * n)) for _ in range(2))
        fsink = torch.full((3, 2 * n + PAD), CANARY, dtype=torch.float32, device="cuda")
        lsink = torch.full((N + 1, 2 * n + PAD), CANARY, dtype=torch.float32, device="cuda")
        r.attach_loudness(meter)
        r.attach_fir_matrix(fm, fsink.data_ptr(), 2 * n + PAD, 2 * n)
        r.attach_limiter(lim, lsink.data_ptr(), 2 * n + PAD, 2 * n)
        rows = np.concatenate([r.process(s.x[:, :n]), r.process(s.x[:, n:])], axis=1)
        c.synchronize()
        plain = np.concatenate([never.process(s.x[:, :n]), never.process(s.x[:, n:])], axis=1)
        assert np.array_equal(bits(rows), bits(plain))
        assert scenes.rel_rms_per_channel(rows, s.want) <= 1e-6
        assert (r.fir_matrix_position(), r.limiter_position()) == (2 * n, 2 * n)
        mix, limited = fsink.cpu().numpy(), lsink.cpu().numpy()
        assert np.all(mix[2] == CANARY) and np.all(mix[:, 2 * n:] == CANARY) and np.all(limited[N] == CANARY) and np.all(limited[:, 2 * n:] == CANARY)
        assert np.array_equal(bits(mix[:2, :2 * n]), bits(fm2.process(rows)))
        assert np.abs(mix[:2, :2 * n]).max() > 1e-3
        want_lim = lim2.process(rows)
        assert lim2.stats()[1] > 1000, "precondition: the bus is over the ceiling"
        assert np.array_equal(bits(limited[:N, :2 * n]), bits(want_lim)) and lim.stats() == lim2.stats()
        meter2.process(rows)
        assert meter.num_steps() == meter2.num_steps() == 2 * n // 128
        steps = meter.steps()
        assert steps.shape == (2 * n // 128, N) and (steps > 0).all()
        # (step energies are float64 sums whose order follows the calls' cutting: the meter's own bound, tests/test_gpu_loudness.py)
        ok, worst = lm.within_bound(steps, meter2.steps())
        print(f"attached meter on 32 channels against the stand-alone meter: worst relative difference {worst:.3e}")
        assert ok, worst
    finally:
        if made:
            made[0].attach_loudness(None), made[0].attach_fir_matrix(None), made[0].attach_limiter(None)
        for v in made:
            v.close()


@pytest.mark.parametrize("two_bus", (True, False))
def test_frames_in_and_out_at_25_channels(two_bus):
    """process_frames to interleaved float and process_frames_pcm to s24 on 25 loudspeakers — 75-byte frames, no dword multiple —
    as tests/test_gpu_render_frames.py and tests/test_gpu_render_pcm_out.py hold them up to 24: the planar float call of the same
    rows bit for bit, and byte for byte the model of the header's conversion applied to the float frames"""
    import pcm_model
    import pcm_out_model as om
    N, M, B, T = 25, 13, 512, 3
    case = mc.Case("frames-25", "frames", M, N, 2 if two_bus else 1, B, T, "holding", wc.SEEDS["holding"] + N, {}, None)
    s = wc.scene(case)
    x = pcm_model.random_frames(np.random.default_rng(23), "s24", T * B, M + 4)
    rows = pcm_model.rows(x, "s24", 3, M)
    r = make_renderer(s, M, N, B, case.buses, T)
    try:
        r.reset(0)
        planar = r.process(np.ascontiguousarray(rows))
        r.reset(0)
        frames = r.process_frames(x, "s24", 3, interleaved_out=True)
        assert frames.shape == (T * B, N) and np.array_equal(bits(frames.T), bits(planar))
        r.reset(0)
        same = r.process_frames(x, "s24", 3, interleaved_out=False)
        assert np.array_equal(bits(same), bits(planar))
        assert np.isfinite(planar).all() and (np.abs(planar).max(axis=1) > 0).all()
        for out_fmt in ("s24", "s16"):
            want, clip = om.from_float(frames, out_fmt)
            r.reset(0)
            got = r.process_frames_pcm(x, "s24", 3, out_fmt)
            assert om.as_bytes(np.array(got)).shape[1] == N * (3 if out_fmt == "s24" else 2)
            assert np.array_equal(om.as_bytes(np.array(got)), om.as_bytes(want)), out_fmt
            peak, clipped = r.output_levels(reset=True)
            assert np.array_equal(bits(peak), bits(om.peak(frames))) and np.array_equal(clipped, clip.sum(axis=0).astype(np.uint64))
    finally:
        r.close()


# ---- (f) end to end on a defined layout of 32 channels
def layout_32():
    """10 LFE channels first, then the dome of tests/custom_layout_model.py (a ring of 12 at elevation 0, a ring of 8 at 35, T+000)
    and B+000 at (0, -30): 22 loudspeakers — the objects kernels' limit — on channels 10 .. 31"""
    import custom_layout_model as model
    lfe = [(f"LFE{i + 1}", -162.0 + 36.0 * i, -30.0, True) for i in range(10)]
    return lfe + list(model.LAYOUT_DOME) + [("B+000", 0.0, -30.0, False)]


def test_defined_layout_of_32_channels_end_to_end():
    """64 moving objects panned by the device producer on a defined layout of 32 channels — a third of them with a zone mask over
    loudspeakers on bits 10 .. 31 of the full layout — and their curves rendered on 32 channels x 2 buses: the oracle's render of the
    same curves (bar 3), and the ten LFE rows exactly zero.  Not a judgement of the producer's gains (tests/test_gpu_custom_layout.py,
    tests/test_gpu_objects.py): that a 32-wide layout's curves come out on the right 32 rows."""
    from libear_amd import capi
    from test_gpu_custom_layout import device_gains
    channels = layout_32()
    N, M, B, T = len(channels), 64, 512, 4
    assert N == 32 and [c[3] for c in channels] == [True] * 10 + [False] * 22
    capi.define_layout("wide:10lfe+dome+b", channels)
    rng = np.random.default_rng(32)
    times = np.arange(-100, T * B + 300, 300, dtype=np.int64)  # (a point every 300 samples, off every tile grid)
    k = np.arange(len(times))[:, None]
    az = (rng.uniform(-180, 180, M)[None, :] + rng.uniform(-8, 8, M)[None, :] * k + 180.0) % 360.0 - 180.0
    el = np.clip(rng.uniform(-30, 90, M)[None, :] + rng.uniform(-3, 3, M)[None, :] * k, -30.0, 90.0)
    diffuse = np.broadcast_to(rng.choice([0.0, 0.3, 1.0], M)[None, :], az.shape)
    real = list(range(10, 32))
    zone = sum(1 << i for i in real[::3]) | 1 << 31  # (the ring at 0, 90, 180, -90, two of the upper ring, and B+000 on bit 31)
    assert zone >> 10 << 10 == zone and zone < 1 << 32
    excluded = np.broadcast_to(np.where(np.arange(M) % 3 == 2, zone, 0).astype(np.uint32)[None, :], az.shape)
    p = capi.Panner(ctx(), "wide:10lfe+dome+b")
    try:
        assert p.n_out == N
        d, f = device_gains(p, az.ravel(), el.ravel(), objects=True, diffuse=diffuse.ravel(), excluded=excluded.ravel())
    finally:
        p.close()
    d, f = d.reshape(len(times), M, N), f.reshape(len(times), M, N)
    assert np.isfinite(d).all() and np.isfinite(f).all() and not d[:, :, :10].any() and not f[:, :, :10].any()
    assert (np.abs(d).max(axis=(0, 1))[10:] > 0).all(), "every loudspeaker gets something"
    masked = np.arange(M) % 3 == 2
    assert not d[:, masked][:, :, [i for i in range(N) if zone >> i & 1]].any()
    curves = [(times, np.ascontiguousarray(d[:, m]), np.ascontiguousarray(f[:, m])) for m in range(M)]
    x = scenes.audio(M, T * B, seed=33)
    s = mc.build_scene("panned", curves, x, [c[0] for c in channels], 2, B)
    got, ran = render_device(s, M, N, B, 2, [T])
    dist = scenes.rel_rms_per_channel(got[10:], s.want[10:])
    print(f"defined layout of 32: {ran}: from the oracle {dist:.3g} (the worst of the 22 loudspeakers)")
    assert np.isfinite(got).all()
    assert not got[:10].any() and not s.want[:10].any(), "an LFE row is not silent"
    assert (np.abs(got[10:]).max(axis=1) > 0).all()
    assert scenes.rel_rms_per_channel(got, s.want) <= 1e-6, worst_channels(got, s.want)


# ---- what ran
def test_every_kernel_kind_ran_at_every_coverage_width():
    """from what the calls above reported: each of the six kernel kinds ran at 50, 64 and 98 columns (run after them, in one session)"""
    print({cols: sorted(k) for cols, k in sorted(RAN.items())})
    for cols in wc.COVERAGE_COLUMNS:
        assert RAN.get(cols, set()) == set(range(6)), (cols, RAN.get(cols))


def test_measured_table():
    """prints what the tests above measured (nothing to assert: the bars are theirs)"""
    print("kernel columns | worst e_gpu, e_lib, distance from the oracle, sample")
    for (kernel, cols), w in sorted(WORST.items()):
        print(f"{kernel} {cols} | {w[0]:.3g} {w[1]:.3g} {w[2]:.3g} {w[3]:.3g}")
