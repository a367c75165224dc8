"""SHA-256 of the outputs of a fixed list of renders that between them pass the branches of the gain stage's launch code:
    python tools/render_digest.py            (EARHIP_LIB=<another build of libearhip.so>: the same list through that build)
    python tools/render_digest.py k2         (the second list: the decorrelator stage and the transforms' launch layer, at the end)
    python tools/render_digest.py paths      (the third list: the rare paths of the split-operand gain kernels, at the end)
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


if __name__ == "__main__":
    if sys.argv[1:] == ["k2"]:
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
