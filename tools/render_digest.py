"""SHA-256 of the outputs of a fixed list of renders that between them pass the branches of the gain stage's launch code:
    python tools/render_digest.py            (EARHIP_LIB=<another build of libearhip.so>: the same list through that build)
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


if __name__ == "__main__":
    for name, curves, opts, kw in CASES:
        run(name, curves, opts, **kw)
    print(f"{len(CASES)} cases")
