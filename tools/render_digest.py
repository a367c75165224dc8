"""SHA-256 of the outputs of a fixed list of renders that between them pass the branches of the gain stage's launch code:
    python tools/render_digest.py            (EARHIP_LIB=<another build of libearhip.so>: the same list through that build)
    python tools/render_digest.py k2         (the second list: the decorrelator stage and the transforms' launch layer, at the end)
    python tools/render_digest.py paths      (the third list: the rare paths of the split-operand gain kernels, at the end)
    python tools/render_digest.py bus        (the fourth list: the output-bus stages alone and attached, and their refusals, at the end)
One line per case: its name, what the renderer reports about the call (gain kernel, tile, tiles, object splits, list layout, whether
the device handed the call to the stand-by lists or ran the robust form) and the digest of the output rows.  Two builds whose host
code enqueues the same kernels on the same data print the same lines; a refactor of the launch code is compared this way.

128 objects (short calls split the objects across workgroups), 24 and 5 loudspeakers on two buses (three column tiles and one), 8
blocks of 512 samples, and one call of 33 tiles that starts off the tile grid.  Every case has its own context with its own options.
Short calls never let the device pick the kernel's form (that takes two rounds of workgroups: 512 tile-splits), so four calls of
512 tiles follow, rendered in one piece (HOST_CHUNK_MB = 0), for the grid kernel's device-picked launches, and one case on one bus (two column tiles, the object splits summed
behind the gain kernel).  Not reached: tuning knobs of the builders and grids (HBUILD_TPW, BUILD_TPW, H2_WGS, PROBE_RUNS), the
growth of a context's words by a gain stage without a renderer, calls of more than 2048 tiles (k_seg_prep<4>)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenes  # noqa: E402
from libear_amd import capi  # noqa: E402

M, B, NB = 128, 512, 8


def ramping_curves(n_out, total, period=600, seed=41):
    """every object always on its way to its next target, the points at a per-object phase (the hinge kernel's curves)"""
    rng = np.random.default_rng(seed)
    curves = []
    for _ in range(M):
        t = np.arange(int(rng.integers(0, period)) - period, total + 2 * period, period, dtype=np.int64)
        curves.append((t, rng.uniform(0.0, 1.0, (len(t), n_out)).astype(np.float32),
                       rng.uniform(0.0, 1.0, (len(t), n_out)).astype(np.float32)))
    return curves


def curves_of(kind, n_out, block, nblocks, t0):
    total = block * nblocks
    if kind == "grid":
        return scenes.dense_curves(M, n_out, block, nblocks, t0=t0)
    if kind == "const":
        return scenes.constant_curves(M, n_out)
    if kind == "adm":
        return [(t + t0, d, f) for t, d, f in scenes.adm_curves(M, n_out, total)]
    if kind == "ragged":
        return [(t + t0, d, f) for t, d, f in scenes.ragged_curves(M, n_out, total)]
    return [(t + t0, d, f) for t, d, f in ramping_curves(n_out, total)]


# (name, curves, options, extras: n_out 24 / 5, strict, block / blocks / start of the call, input levels spread over 120 dB)
CASES = []


def case(name, curves, opts=None, **kw):
    CASES.append((name, curves, opts or {}, kw))


for n_out in (24, 5):
    s = f"_{n_out}ch"
    case("valu" + s, "grid", {"MFMA": 0}, n_out=n_out)
    case("valu_spl2" + s, "ragged", {"MFMA": 0, "SPL": 2}, n_out=n_out)
    case("strict" + s, "adm", {}, n_out=n_out, strict=True)
    case("slots" + s, "adm", {"MFMA": 2}, n_out=n_out)
    case("slots_short_curves" + s, "const", {"MFMA": 2}, n_out=n_out)
    case("slots_nrt4" + s, "ragged", {"MFMA": 2, "NRT": 4}, n_out=n_out)
    case("f32grid" + s, "grid", {"MFMA": 1}, n_out=n_out)
    case("grid" + s, "grid", {}, n_out=n_out)
    for tile in (256, 512):
        case(f"grid_tile{tile}" + s, "grid", {"H2_TILE": tile}, n_out=n_out)
        for pairs in (0, 1):
            case(f"pieces_tile{tile}_pairs{pairs}" + s, "adm", {"MFMA": 5, "P2_TILE": tile, "P2_PAIRS": pairs}, n_out=n_out)
        case(f"hinge_tile{tile}" + s, "ramping", {"MFMA": 6, "HG_TILE": tile}, n_out=n_out)
    case("pieces" + s, "adm", {}, n_out=n_out)
    case("hinge" + s, "ramping", {}, n_out=n_out)
case("grid_h2_pair", "grid", {"H2_TILE": 512, "H2_PAIR": 1})
case("grid_h2_runs", "grid", {"H2_RUNS": 1})
case("grid_no_probe", "grid", {"XSCALE": 12})
case("grid_few_off_grid", "grid", {"MFMA": 4}, off_grid=2)
for b2k in (0, 1):
    case(f"pieces_packed_build2k{b2k}", "adm", {"MFMA": 5, "P2_PAIRS": 0, "BUILD_2K": b2k})
    case(f"pieces_paired_build2k{b2k}", "adm", {"MFMA": 5, "P2_PAIRS": 1, "BUILD_2K": b2k})
    for robust in (0, 1):
        case(f"hinge_robust{robust}_build2k{b2k}", "ramping", {"MFMA": 6, "HG_ROBUST": robust, "BUILD_2K": b2k})
        case(f"hinge_robust{robust}_build2k{b2k}_levels", "ramping", {"MFMA": 6, "HG_ROBUST": robust, "BUILD_2K": b2k}, levels=True)
case("hinge_tile256_robust0_levels", "ramping", {"MFMA": 6, "HG_ROBUST": 0, "HG_TILE": 256}, levels=True)
case("pieces_levels", "adm", {"MFMA": 5}, levels=True)
case("pieces_wgs0", "adm", {"MFMA": 5, "P2_WGS": 0})
case("grid_gsplit1", "grid", {"GSPLIT": 1})
case("grid_one_bus", "grid", {}, one_bus=True)
case("pieces_one_bus", "adm", {"MFMA": 5}, one_bus=True)
# the device picks the form: calls of 512 tiles, as one piece (option HOST_CHUNK_MB = 0: no host chunks) (the 4-wave pair of launches, the 8-wave kernel with both forms, the same as a pair)
case("grid_tile256_long", "grid", {"H2_TILE": 256, "HOST_CHUNK_MB": 0}, nblocks=256)
case("grid_tile512_long", "grid", {"H2_TILE": 512, "HOST_CHUNK_MB": 0}, nblocks=512)
case("grid_tile512_long_h2_pair", "grid", {"H2_TILE": 512, "H2_PAIR": 1, "HOST_CHUNK_MB": 0}, nblocks=512)
case("grid_tile256_long_5ch_levels", "grid", {"H2_TILE": 256, "HOST_CHUNK_MB": 0}, n_out=5, nblocks=256, levels=True)
# the lists standing by behind 512-sample hinge tiles, an odd number of their own 256-sample tiles
case("hinge_robust0_levels_33_tiles_from_37", "ramping", {"MFMA": 6, "HG_ROBUST": 0}, block=256, nblocks=33, t0=37, levels=True)
# one call of 33 tiles that starts at sample 37
for name, curves, opts in (("valu", "ragged", {"MFMA": 0}), ("slots", "ragged", {"MFMA": 2}), ("grid", "grid", {"H2_TILE": 256}),
                           ("pieces", "adm", {"MFMA": 5}), ("hinge", "ramping", {"MFMA": 6, "HG_TILE": 256})):
    case(name + "_33_tiles_from_37", curves, opts, block=256, nblocks=33, t0=37)
case("f32grid_33_tiles_from_37", "grid", {"MFMA": 1}, block=512, nblocks=33, t0=37)


def run(name, curves, opts, n_out=24, strict=False, block=B, nblocks=NB, t0=0, levels=False, off_grid=0, one_bus=False):
    rng = np.random.default_rng(5)
    dec = None if one_bus else rng.uniform(-0.1, 0.1, (n_out, 512)).astype(np.float32)
    x = scenes.audio(M, block * nblocks)
    if levels:
        x *= scenes.object_levels(M, span_db=120.0)[0][:, None]
    ctx = capi.Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_strict(strict)
    r = capi.Renderer(ctx, M, n_out, block, dec, 0 if one_bus else 255, max_blocks=nblocks)
    r.reset(t0)
    cs = curves_of(curves, n_out, block, nblocks, t0)
    for m in range(off_grid):  # (a few objects with their points off the grid: the grid kernel's exact path)
        cs[m] = (cs[m][0] + 5, cs[m][1], cs[m][2])
    for m, (t, d, f) in enumerate(cs):
        r.set_object_points(m, t, d, None if one_bus else f)
    out = r.process(x)
    plan = r.last_plan()
    what = (f"kernel {plan['kernel']} tile {plan['tile']} ntiles {plan['ntiles']} gsplit {plan['gsplit']} paired {r.last_list_layout()} "
            f"standby {int(r.hinge_standby())} robust {int(r.hinge_robust())} wide {r.wide_form()} regrows {r.scratch_regrows()}")
    out2 = r.process(x)  # (the second call: the other level words, the state of the first)
    r.close()
    ctx.close()
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(out2)), name
    print(f"{name:42s} {what}\n    {hashlib.sha256(out.tobytes()).hexdigest()} {hashlib.sha256(out2.tobytes()).hexdigest()}")


# ---- the second list (argument "k2"): what launches a transform -----------------------------------------------------------
# The decorrelator stage at every block size that takes another kernel or partitioning, its options, FIRs of several partitions,
# object splits summed in front of the wave kernel, a call cut into a main span and a tail (with and without the call timer); then
# the FFT plugin, a BlockConvolver and a FIR matrix at their smallest, an odd and their largest sizes.
K2_CASES = []


def k2_case(name, block, opts=None, **kw):
    for n_out in kw.pop("n_outs", (5, 24)):
        K2_CASES.append((f"{name}_{n_out}ch", block, opts or {}, dict(kw, n_out=n_out)))


for b in (48, 64, 128, 256, 512):
    k2_case(f"k2_block{b}", b)
k2_case("k2_block512_wg", 512, {"K2_WG": 1})
k2_case("k2_block512_run3", 512, {"RUN": 3})
k2_case("k2_block512_taps700", 512, n_taps=700)
k2_case("k2_block512_taps700_delay0", 512, n_taps=700, delay=0)
for b in (1024, 2048):
    k2_case(f"k2_block{b}", b)
    k2_case(f"k2_block{b}_own_block", b, {"K2_OWN_BLOCK": 1})
k2_case("k2_block4096_taps4096", 4096, n_taps=4096)
k2_case("k2_sum_parts", 512, m=128, nblocks=2)
# (96 objects: from 128 on the planner splits the objects of a call of so few tiles, and a call with object splits is not cut)
k2_case("k2_tail_cut", 512, {"H2_TILE": 512, "HOST_CHUNK_MB": 0}, m=96, nblocks=264, calls=1, n_outs=(24,))
k2_case("k2_tail_cut_timed", 512, {"H2_TILE": 512, "HOST_CHUNK_MB": 0}, m=96, nblocks=264, calls=1, timing=True, n_outs=(24,))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_k2(name, block, opts, n_out, m=16, nblocks=4, n_taps=512, delay=255, calls=2, timing=False):
    rng = np.random.default_rng(6)
    dec = rng.uniform(-0.1, 0.1, (n_out, n_taps)).astype(np.float32)
    x = scenes.audio(m, block * nblocks)
    ctx = capi.Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    r = capi.Renderer(ctx, m, n_out, block, dec, delay, max_blocks=nblocks)
    for i, (t, d, f) in enumerate(scenes.dense_curves(m, n_out, block, nblocks)):
        r.set_object_points(i, t, d, f)
    if timing:
        r.enable_timing(1)
    outs, what = [], ""
    for _ in range(calls):
        outs.append(r.process(x))
        plan = r.last_plan()
        what += f" [kernel {plan['kernel']} tile {plan['tile']} ntiles {plan['ntiles']} gsplit {plan['gsplit']} tail {r.last_tail_blocks()}]"
    if timing:
        tm = r.get_timing()
        what += f" timed calls: gain {tm['gain_mix_launches']:g} decor {tm['decor_launches']:g} prep {tm['prep_launches']:g}"
    r.close()
    ctx.close()
    assert all(np.all(np.isfinite(o)) for o in outs), name
    print(f"{name:42s}{what}\n    {' '.join(sha(o) for o in outs)}")


def run_transforms():
    rng = np.random.default_rng(9)
    ctx = capi.Context(0)
    for n in (64, 96, 8192):
        p = capi.FFTPlan(ctx, n)
        X = p.forward(rng.uniform(-1.0, 1.0, n).astype(np.float32))
        y = p.reverse(X)
        p.close()
        assert np.all(np.isfinite(y)), n
        print(f"{'fft_%d' % n:42s}\n    {sha(X)} {sha(y)}")
    for b in (48, 512):
        cc = capi.ConvCtx(ctx, b)
        fa = capi.ConvFilter(cc, rng.uniform(-0.1, 0.1, 2 * b + 5).astype(np.float32))
        fb = capi.ConvFilter(cc, rng.uniform(-0.1, 0.1, b).astype(np.float32))
        conv = capi.BlockConvolver(cc, fa)
        x = rng.uniform(-1.0, 1.0, (9, b)).astype(np.float32)
        outs = []
        for i in range(9):  # (a crossfade, silence until the tail has run out, input again)
            if i == 2:
                conv.crossfade_filter(fb)
            outs.append(conv.process(None if 4 <= i < 8 else x[i]))
        assert np.all(np.isfinite(outs)), b
        print(f"{'block_convolver_%d' % b:42s}\n    {sha(np.stack(outs))}")
    for b in (64, 4096):
        taps = rng.uniform(-0.1, 0.1, (2, 3, b + 7)).astype(np.float32)
        taps[1, 2] = 0.0
        fm = capi.FirMatrix(ctx, taps, b, max_blocks=3)
        x = rng.uniform(-1.0, 1.0, (3, 3 * b)).astype(np.float32)
        y1, y2 = fm.process(x), fm.process(x[:, :b])
        fm.close()
        assert np.all(np.isfinite(y1)) and np.all(np.isfinite(y2)), b
        print(f"{'firmix_%d' % b:42s}\n    {sha(y1)} {sha(y2)}")
    ctx.close()


# ---- the third list (argument "paths"): the rare paths of the split-operand gain kernels (gain_split.h) --------------------
# scenes.split_paths_scene (tests/test_gpu_render.py, test_split_kernels_*) with each kernel forced, on one and on several column
# tiles: through the host form with bursts above the probed level (the exact path inside tiles, the overflow redo, a ragged last
# tile), and without them on the direct bus alone from device buffers whose output rows are unaligned (every object on the exact
# path, scalar stores).
PATH_KERNELS = [("grid", {"H2_TILE": 256}), ("grid", {"H2_TILE": 512}), ("pieces", {"MFMA": 5, "P2_TILE": 256}),
                ("pieces", {"MFMA": 5, "P2_TILE": 512}), ("hinge", {"MFMA": 6, "HG_TILE": 256}), ("hinge", {"MFMA": 6, "HG_TILE": 512})]


def run_paths(kind, opts, n_out, unaligned):
    sp = scenes.SPLIT_PATHS
    m, block, nblocks, t0 = sp["m"], sp["block"], sp["nblocks"], sp["start"]
    total = block * nblocks
    tile = list(opts.values())[-1]  # (the grid kernel's curves: their points on the grid of the tile asked for)
    curves, x = scenes.split_paths_scene(kind, n_out, not unaligned, tile)
    dec = None if unaligned else np.random.default_rng(5).uniform(-0.1, 0.1, (n_out, 512)).astype(np.float32)
    ctx = capi.Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    if unaligned:
        ctx.set_option("GSPLIT", 1)  # (the gain kernel writes the output rows itself)
    r = capi.Renderer(ctx, m, n_out, block, dec, 0 if unaligned else 255, max_blocks=nblocks)
    r.reset(t0)
    for i, (t, d, f) in enumerate(curves):
        r.set_object_points(i, t + t0, d, None if unaligned else f)
    outs = []
    for _ in range(2):  # (the second call: the other level words, the state of the first)
        if unaligned:
            import torch
            xin = torch.from_numpy(x).cuda()
            o = torch.full((n_out, total + 1), 7.5, dtype=torch.float32, device="cuda")
            r.process_device(nblocks, xin.data_ptr(), total, o.data_ptr(), total + 1)
            ctx.synchronize()
            outs.append(o.cpu().numpy())
        else:
            outs.append(r.process(x))
        if not outs[1:]:
            plan = r.last_plan()
            what = (f"kernel {plan['kernel']} tile {plan['tile']} ntiles {plan['ntiles']} gsplit {plan['gsplit']} paired {r.last_list_layout()} "
                    f"standby {int(r.hinge_standby())} robust {int(r.hinge_robust())} wide {r.wide_form()} regrows {r.scratch_regrows()}")
    r.close()
    ctx.close()
    name = f"paths_{kind}_tile{tile}_{n_out}ch" + ("_unaligned" if unaligned else "")
    assert all(np.all(np.isfinite(o)) for o in outs), name
    print(f"{name:42s} {what}\n    {sha(outs[0])} {sha(outs[1])}")


# ---- the fourth list (argument "bus"): the stages of the output bus (bus_stage.h) --------------------------------------------
# Every stage alone, in its device form and its host form: three consecutive calls of unequal lengths (1 sample, a tile + 3, two
# tiles + 331; the FIR matrix: 1, 2 and 3 blocks of 64), reset, the first call again; an input row nothing reads where the stage
# has that notion.  A call one sample longer than a launch (delay matrix, biquad matrix, converter).  A renderer of 16 objects and 5
# outputs in blocks of 64 with meter, matrix and limiter attached, through every form of call and a host call that runs as a pipeline
# of chunks, one stage detached at the end; the same with 32 objects (the fewest the split-operand gain kernels take) for a call cut
# into a main span and a tail.  Every call the stages' shared checks refuse:
# its status and message, and behind each a valid call in the same form whose digest is that of a stage never refused anything.
def bus_stages(ctx):
    """name -> (make(), rows in, the tile the call lengths are built on); made anew for each form"""
    rng = np.random.default_rng(12)
    fir = rng.uniform(-0.1, 0.1, (2, 3, 64 + 7)).astype(np.float32)
    fir[:, 2] = 0.0  # (input 2 has no pair)
    lp, hs = capi.iir_design("lowpass", 48000, 1000.0), capi.iir_design("high_shelf", 48000, 4000.0, gain_db=3.0)
    src_taps = capi.src_design(3, 2, 8)
    dly = rng.uniform(-0.5, 0.5, 2).astype(np.float32)
    return {
        "loudness": (lambda: capi.Loudness(ctx, 2, 48000, max_steps=8, true_peak=True), 2, 4800),
        "firmix": (lambda: capi.FirMatrix(ctx, fir, 64, max_blocks=3), 3, 64),
        "limiter": (lambda: capi.Limiter(ctx, 2, 0.5, max_samples=4096), 2, 1024),
        "iir": (lambda: capi.IirBank(ctx, 3, 2, [(0, 0, 1.0, [lp]), (1, 1, 0.5, None), (2, 1, 0.25, [lp, hs])], max_samples=4096), 3, 256),
        "src": (lambda: capi.SampleRateConverter(ctx, 2, 3, 2, 8, src_taps, max_samples=4096), 2, 1024),
        "delaymix": (lambda: capi.DelayMatrix(ctx, 3, 2, [(0, 0, 5, dly), (1, 1, 0, [-0.5])], max_samples=4096), 3, 1024),
    }


def bus_lengths(name, tile):
    return [64, 128, 192] if name == "firmix" else [1, tile + 3, 2 * tile + 331]


def stage_call(name, st, x, device, ctx):
    """one call of the stage on x [rows][n] -> what it hands back (the meter: its step energies and peaks so far)"""
    import torch
    n = x.shape[1]
    if not device:
        if name == "loudness":
            st.process(x)
        elif name == "limiter":
            out, gain = st.process(x, with_gain=True)
            return np.concatenate([out.reshape(-1), gain])
        else:
            return st.process(x)
    else:
        xi = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        rows_out = st.K if name == "firmix" else getattr(st, "n_out", x.shape[0])  # (the others: as many as come in)
        cap = st.next_out(n) if name == "src" else n
        o = torch.full((rows_out, cap + 3), 7.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (torch's fill, on its own stream, is done before the context's stream writes there)
        if name == "loudness":
            st.process_device(n, xi.data_ptr(), n)
        elif name == "firmix":
            st.process_device(n // 64, xi.data_ptr(), n, o.data_ptr(), cap + 3)
        elif name == "src":
            assert st.process_device(n, xi.data_ptr(), n, o.data_ptr(), cap + 3, cap) == cap
        else:
            st.process_device(n, xi.data_ptr(), n, o.data_ptr(), cap + 3)
        ctx.synchronize()
        if name != "loudness":
            return o.cpu().numpy()
    return np.concatenate([st.steps().reshape(-1), np.concatenate(st.peaks()).astype(np.float64)])


def run_bus_stages(ctx):
    for name, (make, rows, tile) in bus_stages(ctx).items():
        lengths = bus_lengths(name, tile)
        x = scenes.audio(rows, sum(lengths), seed=51)
        for device in (True, False):
            st = make()
            outs, at = [], 0
            for n in lengths:
                outs.append(stage_call(name, st, x[:, at:at + n], device, ctx))
                at += n
            st.reset()
            outs.append(stage_call(name, st, x[:, :lengths[0]], device, ctx))
            st.close()
            print(f"{'bus_%s_%s' % (name, 'device' if device else 'host'):42s}\n    {' '.join(sha(o) for o in outs)}")
    # one sample more than a launch, where a stage says what its launch holds (the delay matrix: launch_in; the biquad matrix: a
    # chunk in front of and behind scan_groups x scan_lanes whole ones) or its tests reach it (the converter: 2^20 inputs); the
    # meter's and the limiter's launches are longer than any call of the tests, the FIR matrix does not cut its calls
    probe = capi.DelayMatrix(ctx, 1, 1, [(0, 0, 0, [1.0])], 1)
    dly_launch = probe.info()["launch_in"]
    probe.close()
    lp = capi.iir_design("lowpass", 48000, 1000.0)
    probe = capi.IirBank(ctx, 1, 1, [(0, 0, 1.0, [lp])], max_samples=1)
    info = probe.info()
    probe.close()
    iir_launch = (info["scan_groups"] * info["scan_lanes"] + 1) * info["chunk"]
    src_launch, src_taps = 1 << 20, capi.src_design(2, 3, 8)
    longer = {
        "delaymix": (dly_launch, lambda n: capi.DelayMatrix(ctx, 1, 1, [(0, 0, 5, [0.75, -0.25])], max_samples=n)),
        "iir": (iir_launch, lambda n: capi.IirBank(ctx, 1, 1, [(0, 0, 0.5, [lp])], max_samples=n)),
        "src": (src_launch, lambda n: capi.SampleRateConverter(ctx, 1, 2, 3, 8, src_taps, max_samples=n)),
    }
    for name, (launch, make) in longer.items():
        x = scenes.audio(1, launch + 1, seed=52)
        for device in (True, False):
            st = make(launch + 1)
            out = stage_call(name, st, x, device, ctx)
            st.close()
            print(f"{'bus_%s_launch_plus_1_%s' % (name, 'device' if device else 'host'):42s} launch {launch}\n    {sha(out)}")


def run_bus_renderer(M, tail_cut):
    """M = 16: every form of call and the pipeline.  The tail cut is the split-operand gain kernels', which take 32 objects or more:
    the call of two spans goes through a second renderer of 32"""
    import torch
    N, B, T, TAIL = 5, 64, 4096, 2112  # (T: a host call of 16 MB of input rows; TAIL: 264 tiles of 512)
    if tail_cut:
        T = TAIL
    rng = np.random.default_rng(13)
    dec = rng.uniform(-0.1, 0.1, (N, 512)).astype(np.float32)
    fir = rng.uniform(-0.1, 0.1, (2, N, B + 7)).astype(np.float32)
    ctx = capi.Context(0)
    ctx.set_option("H2_TILE", 512)
    r = capi.Renderer(ctx, M, N, B, dec, 255, max_blocks=T)
    for i, (t, d, f) in enumerate(scenes.dense_curves(M, N, 512, 2 * T * B // 512)):
        r.set_object_points(i, t, d, f)
    r.commit()
    cap = 2 * T * B
    meter = capi.Loudness(ctx, N, 48000, max_steps=cap // 4800 + 1, true_peak=True)
    matrix = capi.FirMatrix(ctx, fir, B, max_blocks=T)
    lim = capi.Limiter(ctx, N, 0.25, max_samples=T * B)
    sink_m = torch.zeros((2, cap), dtype=torch.float32, device="cuda")
    sink_l = torch.zeros((N, cap), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (torch's fill, on its own stream, is done before the context's stream writes there)
    r.attach_loudness(meter)
    r.attach_fir_matrix(matrix, sink_m.data_ptr(), cap, cap)
    r.attach_limiter(lim, sink_l.data_ptr(), cap, cap)

    def report(name, out, seen):
        """the call's rows, what the taps wrote for it, and where they stand"""
        ctx.synchronize()
        a, b = r.fir_matrix_position(), r.limiter_position()
        print(f"{name:42s} matrix at {a} limiter at {b} meter steps {meter.num_steps()} chunks {r.last_host_chunks()} "
              f"tail {r.last_tail_blocks()} kernel {r.last_plan()['kernel']}\n    {sha(out)} {sha(sink_m[:, seen[0]:a].cpu().numpy())} {sha(sink_l[:, seen[1]:b].cpu().numpy())} "
              f"{sha(np.concatenate(meter.peaks()))}")
        seen[0], seen[1] = a, b

    seen = [0, 0]
    x = scenes.audio(M, T * B, seed=53)
    n = 8 * B  # (the short calls end on the grid of the gain kernel's tiles)
    if not tail_cut:
        report("bus_render_process", r.process(x[:, :n]), seen)
        xi = torch.from_numpy(np.ascontiguousarray(x[:, :n])).cuda()
        o = torch.zeros((N, n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (torch's fill, on its own stream, is done before the context's stream writes there)
        r.process_device(8, xi.data_ptr(), n, o.data_ptr(), n)
        ctx.synchronize()
        report("bus_render_process_device", o.cpu().numpy(), seen)
        frames = rng.integers(-20000, 20000, (n, M)).astype(np.int16)
        report("bus_render_process_frames", r.process_frames(frames, "s16"), seen)
        ctx.set_option("HOST_CHUNK_MB", 4)  # 16 MB of input rows: a pipeline of four chunks
        report("bus_render_host_pipeline", r.process(x), seen)
        assert r.last_host_chunks() >= 3
    else:
        ctx.set_option("HOST_CHUNK_MB", 0)  # 264 tiles of 512 in one piece: a whole round and a few tiles behind it
        xi = torch.from_numpy(x).cuda()
        o = torch.zeros((N, TAIL * B), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (torch's fill, on its own stream, is done before the context's stream writes there)
        r.process_device(TAIL, xi.data_ptr(), T * B, o.data_ptr(), TAIL * B)
        ctx.synchronize()
        report("bus_render_32_objects_tail_cut", o.cpu().numpy(), seen)
        assert r.last_tail_blocks() > 0
    r.attach_fir_matrix(None)
    report(f"bus_render_{M}_objects_matrix_detached", r.process(x[:, :n]), seen)
    print(f"{'bus_render_%d_objects_meter' % M:42s}\n    {sha(meter.steps())}")
    for st in (meter, matrix, lim):
        st.close()
    r.close()
    ctx.close()


WIDE = 49152  # (samples per row behind the refused calls' pointers: more than any of them names)


def refusal(what, rc):
    msg = capi.load().earhip_last_error().decode() if rc else ""
    print(f"    {what:34s} status {rc} {msg!r}")


def run_bus_refusals(ctx):
    """the calls the shared checks refuse, through the library's own symbols (the wrapper cannot pass a NULL handle or row)"""
    import ctypes as C
    import torch
    lib = capi.load()
    sz, vp = C.c_size_t, C.c_void_p
    for name, (make, rows, tile) in bus_stages(ctx).items():
        unit = 64 if name == "firmix" else 1
        n = 2 * unit  # (a call of two units)
        rows_out = {"firmix": 2, "iir": 2, "delaymix": 2, "loudness": 0}.get(name, rows)
        x = scenes.audio(rows, WIDE, seed=54)
        xi = torch.from_numpy(x).cuda()
        o = torch.zeros((max(rows_out, 1), WIDE), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (torch's fill, on its own stream, is done before the context's stream writes there)
        host_out = np.zeros((max(rows_out, 1), WIDE), np.float32)
        stride = x.shape[1]
        dev_fn, host_fn = getattr(lib, f"earhip_{name}_process_device"), getattr(lib, f"earhip_{name}_process")
        got = sz(0)
        tail = {"limiter": (None,), "src": (sz(stride), C.byref(got))}.get(name, ())

        def dev(h, units, i, istride, out, ostride, tail=tail):
            if name == "loudness":
                return dev_fn(h, sz(units), vp(i), sz(istride))
            return dev_fn(h, sz(units), vp(i), sz(istride), vp(out), sz(ostride), *tail)

        def host(h, units, ins, outs, tail=tail):
            if name == "loudness":
                return host_fn(h, sz(units), ins)
            return host_fn(h, sz(units), ins, outs, *tail)

        st = make()
        over = {"loudness": 10 * 4800, "firmix": 4}.get(name, 4097)
        read_row = 0
        print(f"bus_refusals_{name}")
        twin, at = make(), [0]  # (the twin takes the valid calls alone)

        def refuse(what, rc, st=st, twin=twin, at=at, name=name, x=x):
            """the refusal, and behind it a valid call in the refused call's form: its digest, and whether a stage that was never
            refused anything gives the same"""
            refusal(what, rc)
            device = what.startswith("device")
            seg = np.ascontiguousarray(x[:, at[0]:at[0] + (64 if name == "firmix" else 96)])
            at[0] += seg.shape[1]
            got, want = stage_call(name, st, seg, device, ctx), stage_call(name, twin, seg, device, ctx)
            print(f"        the next call ({'device' if device else 'host'}): untouched {sha(got) == sha(want)} {sha(got)[:16]}")

        refuse("device: NULL handle", dev(None, n // unit, xi.data_ptr(), stride, o.data_ptr(), stride))
        refuse("device: over room", dev(st.h, over, xi.data_ptr(), stride, o.data_ptr(), stride))
        refuse("device: NULL in", dev(st.h, n // unit, None, stride, o.data_ptr(), stride))
        if rows_out:
            refuse("device: NULL out", dev(st.h, n // unit, xi.data_ptr(), stride, None, stride))
        refuse("device: short in stride", dev(st.h, n // unit, xi.data_ptr(), n - 1, o.data_ptr(), stride))
        if rows_out:
            refuse("device: short out stride", dev(st.h, n // unit, xi.data_ptr(), stride, o.data_ptr(), 0))
        refuse("host: NULL handle", host(None, n // unit, capi._chan_ptrs(x), capi._chan_ptrs(host_out)))
        refuse("host: over room", host(st.h, over, capi._chan_ptrs(x), capi._chan_ptrs(host_out)))
        refuse("host: NULL in", host(st.h, n // unit, None, capi._chan_ptrs(host_out)))
        if rows_out:
            refuse("host: NULL out", host(st.h, n // unit, capi._chan_ptrs(x), None))
        ins = capi._chan_ptrs(x)
        ins[read_row] = None
        refuse("host: NULL row that is read", host(st.h, n // unit, ins, capi._chan_ptrs(host_out)))
        if rows_out:
            outs = capi._chan_ptrs(host_out)
            outs[rows_out - 1] = None
            refuse("host: NULL row that is written", host(st.h, n // unit, capi._chan_ptrs(x), outs))
        if name == "src":
            refuse("device: short out_capacity", dev(st.h, n, xi.data_ptr(), stride, o.data_ptr(), stride, tail=(sz(1), C.byref(got))))
            refuse("host: short out_capacity", host(st.h, n, capi._chan_ptrs(x), capi._chan_ptrs(host_out), tail=(sz(1), C.byref(got))))
        refuse("reset: NULL handle", getattr(lib, f"earhip_{name}_reset")(None))
        refuse("destroy: NULL handle", getattr(lib, f"earhip_{name}_destroy")(None))
        ctx.synchronize()
        assert not o.any() and not host_out.any(), name
        st.close()
        twin.close()
    # the renderer's taps
    M, N, B, T = 16, 5, 64, 4
    dec = np.random.default_rng(14).uniform(-0.1, 0.1, (N, 512)).astype(np.float32)
    fir = np.random.default_rng(15).uniform(-0.1, 0.1, (2, N, B)).astype(np.float32)
    r = capi.Renderer(ctx, M, N, B, dec, 255, max_blocks=T)
    for i, (t, d, f) in enumerate(scenes.dense_curves(M, N, B, 2 * T)):
        r.set_object_points(i, t, d, f)
    other = capi.Context(0)
    sink = torch.zeros((N, 2 * T * B), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (torch's fill, on its own stream, is done before the context's stream writes there)
    cap = 2 * T * B
    makers = {
        "loudness": lambda c, rows, b: capi.Loudness(c, rows, 48000, max_steps=4),
        "firmix": lambda c, rows, b: capi.FirMatrix(c, fir[:, :rows] if rows <= N else np.concatenate([fir, fir[:, :1]], axis=1), b, max_blocks=T),
        "limiter": lambda c, rows, b: capi.Limiter(c, rows, 0.25, max_samples=T * B),
    }

    def attach(name, st, sink_ptr, stride, capacity):
        if name == "loudness":
            return lib.earhip_render_attach_loudness(r.h, st.h)
        return getattr(lib, f"earhip_render_attach_{name}")(r.h, st.h, vp(sink_ptr), sz(stride), sz(capacity))

    x = scenes.audio(M, 2 * T * B, seed=55)
    print("bus_refusals_attach")
    for name, make in makers.items():
        for what, c, rows, b in (("another context", other, N, B), ("other rows", ctx, N + 1, B), ("another block size", ctx, N, 2 * B)):
            if what == "another block size" and name != "firmix":
                continue
            st = make(c, rows, b)
            refusal(f"{name}: {what}", attach(name, st, sink.data_ptr(), cap, cap))
            st.close()
        if name == "loudness":
            continue
        st = make(ctx, N, B)
        refusal(f"{name}: NULL sink", attach(name, st, None, cap, cap))
        refusal(f"{name}: stride < capacity", attach(name, st, sink.data_ptr(), cap - 1, cap))
        refusal(f"{name}: attached", attach(name, st, sink.data_ptr(), cap, T * B + B))
        first = r.process(x[:, :T * B])
        unwritten = np.zeros((N, T * B), np.float32)
        rc = lib.earhip_render_process(r.h, sz(T), capi._chan_ptrs(x, T * B), capi._chan_ptrs(unwritten))
        refusal(f"{name}: past the sink's capacity", rc)
        pos = sz(0)
        getattr(lib, f"earhip_render_{name}_position")(r.h, C.byref(pos))
        getattr(r, {"firmix": "attach_fir_matrix", "limiter": "attach_limiter"}[name])(None)
        second = r.process(np.ascontiguousarray(x[:, T * B:]))  # (the refused call rendered nothing: this is the stream's second call)
        print(f"    {name}: position {pos.value}, the calls around the refusal\n    {sha(first)} {sha(second)}")
        r.reset(0)
        st.close()
    refusal("position: NULL", lib.earhip_render_firmix_position(r.h, None))
    r.close()
    other.close()


if __name__ == "__main__":
    if sys.argv[1:] == ["bus"]:
        import torch  # noqa: F401  (before the library touches the device: one HIP runtime per process, torch's)
        ctx = capi.Context(0)
        run_bus_stages(ctx)
        run_bus_refusals(ctx)
        ctx.close()
        run_bus_renderer(16, False)
        run_bus_renderer(32, True)
    elif sys.argv[1:] == ["k2"]:
        for name, block, opts, kw in K2_CASES:
            run_k2(name, block, opts, **kw)
        run_transforms()
        print(f"{len(K2_CASES)} renders, the transforms")
    elif sys.argv[1:] == ["paths"]:
        import torch  # noqa: F401  (before the library touches the device: one HIP runtime per process, torch's — as bench.py does)
        for unaligned in (False, True):
            for kind, opts in PATH_KERNELS:
                for n_out in (5, 24):
                    run_paths(kind, opts, n_out, unaligned)
        print(f"{4 * len(PATH_KERNELS)} cases")
    else:
        for name, curves, opts, kw in CASES:
            run(name, curves, opts, **kw)
        print(f"{len(CASES)} cases")
