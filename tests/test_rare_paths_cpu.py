"""The conditions that keep the cases of tests/rare_path_cases.py honest, without a device: what tests/test_gpu_rare_paths.py (and
the two rare-path tests of tests/test_gpu_render.py, group A) take for granted about their scenes.

  * probe: every burst and every non-finite sample lies where k_level_probe does not read, under every cutting of the call;
  * overflow: the input scale of every call follows probed_input_scale's rule, every burst times that scale is at least 65520 (it
    rounds to an infinite f16), and no other sample reaches that;
  * EARHIP_XSCALE: the share of 64-sample wave spans with a sample beyond the f16 range is 0 at 2^7, strictly between 0 and 1 at
    2^16 and 1 at 2^18;
  * the busy objects have more ramps in a tile than a list takes per object; the bursts sit in the call's first and last tile and
    in interior tiles of a workgroup's run; a case whose P2_WGS sweep really carries a pipeline exists per tile size, layout and form;
  * e_lib, the oracle's own distance from a float64 evaluation, is printed per scene and at most 5e-7: 1e-6 against the oracle
    is reachable at these sizes;
  * every case id is unique and names kernel, tile, layout and form."""
import functools

import numpy as np
import pytest

import rare_path_cases as rc
import scenes

CUTTINGS = rc.long_calls()


def _check_overflow(x, bursts, calls, name, every_sample=True):
    """the scale of each call by the rule; bursts beyond the f16 range at that scale, everything else within it"""
    burst = np.zeros(x.shape, bool)
    for obj, s in bursts:
        burst[obj, s:s + 3] = True
    for start, n in calls:
        k = rc.probed_scale_log2(x, start, n)
        mag = np.abs(x[:, start:start + n].astype(np.float64)) * 2.0 ** k
        b = burst[:, start:start + n]
        print(f"{name} call [{start}, {start + n}): scale 2^{k}, bursts scaled to {mag[b].min():.3g} .. {mag[b].max():.3g}, "
              f"the rest up to {mag[~b].max():.3g}")
        # (a burst is three samples; scenes.split_paths_scene multiplies what is there by 10^4, so one of its six samples stays
        # small: every burst's PEAK is beyond the range — its wave's totals are not finite; the long scenes' every sample is)
        peaks = [mag[obj, s - start:s - start + 3].max() for obj, s in bursts if start <= s < start + n]
        assert peaks and min(peaks) >= rc.F16_OVERFLOW, (name, start, n, peaks)
        if every_sample:
            assert mag[b].min() >= rc.F16_OVERFLOW, (name, start, n)
        assert mag[~b].max() < rc.F16_OVERFLOW, (name, start, n)


def test_bursts_and_non_finite_samples_are_not_probed():
    bursts = rc.long_bursts()
    assert len(bursts) >= 6
    for cutting in CUTTINGS:
        for obj, s in bursts:
            assert not any(rc.probed_in(obj, s + i, cutting) for i in range(3)), (obj, s, cutting)
    for _, obj in rc.NON_FINITE:
        s = rc.non_finite_sample(obj)
        total = rc.long_blocks(256) * 512
        assert not rc.probed_in(obj, s, [(0, total)])
        assert 512 <= s < total - 512  # an interior tile of either tile size


def test_long_scene_bursts_overflow_and_nothing_else_does():
    x = rc.long_inputs(rc.CUS, True)
    bursts = rc.long_bursts()
    for cutting in CUTTINGS:
        end = cutting[-1][0] + cutting[-1][1]
        _check_overflow(x, [b for b in bursts if b[1] < end], cutting, "long scene")
    clean = rc.long_inputs(rc.CUS, False)  # (group E: nothing overflows before the non-finite sample goes in)
    k = rc.probed_scale_log2(clean, 0, rc.long_blocks(256) * 512)
    assert np.abs(clean).max() * 2.0 ** k < rc.F16_OVERFLOW


@pytest.mark.parametrize("kind,tile", [("grid", 256), ("grid", 512), ("pieces", 256), ("hinge", 256)])
def test_split_paths_scene_bursts_overflow(kind, tile):
    """group A's scene, scenes.split_paths_scene(..., bursts=True): the same conditions"""
    sp = scenes.SPLIT_PATHS
    total = sp["block"] * sp["nblocks"]
    _, x = scenes.split_paths_scene(kind, 6, True, tile)
    _, clean = scenes.split_paths_scene(kind, 6, False, tile)
    where = np.argwhere(x != clean)
    bursts = sorted({(int(o), int(s)) for o, s in where})
    firsts = [(o, s) for o, s in bursts if (o, s - 1) not in bursts]
    assert len(firsts) == 2 and len(bursts) == 6
    for o, s in bursts:
        assert s not in scenes.probed_samples(o, total)
    _check_overflow(x, firsts, [(0, total)], f"split_paths_scene {kind}", every_sample=False)


def test_xscale_shares():
    """EARHIP_XSCALE = 7 / 16 / 18 on the full-scale inputs of group C: no / some / every wave span holds a sample beyond f16"""
    seen = set()
    for c in rc.BY_GROUP["C"]:
        x = rc.small_scene(*c.scene).x
        if x.tobytes() in seen:
            continue
        seen.add(x.tobytes())
        shares = {k: rc.overflow_share(x, k) for k in rc.XSCALES}
        print(f"group C inputs {x.shape}: shares of overflowing wave spans {shares}")
        assert shares[7] == 0.0 and 0.0 < shares[16] < 1.0 and shares[18] == 1.0, shares
    assert {c.extra["k"] for c in rc.BY_GROUP["C"]} == set(rc.XSCALES)


def test_busy_objects_exceed_the_lists_capacity_and_bursts_sit_where_they_should():
    n = rc.n_out(rc.LONG["layout"])
    bursts = rc.long_bursts()
    busy = dict(rc.BUSY)
    total = rc.long_blocks(512) * 512
    curves = rc.long_curves("pieces", n, total)
    for tile in (256, 512):
        ntiles = rc.long_blocks(tile) * 512 // tile
        end = ntiles * tile
        ramps = {o: [rc.ramps_in_tile(curves[o][0], t * tile, (t + 1) * tile) for t in range(ntiles)] for o in busy}
        for paired, cap in rc.LIST_CAPACITY.items():
            over = {o: sum(r > cap for r in ramps[o]) for o in busy}
            print(f"tile {tile} {'paired' if paired else 'packed'} (capacity {cap}): tiles of {ntiles} in which a busy object takes the exact path {over}")
            # a point every 5, 11, 16 samples: more ramps than either layout holds in EVERY tile of either size.  (A point every 37,
            # 45, 70 samples is 4 .. 14 ramps per tile: beyond the paired lists' 7 in 512-sample tiles, the list builder's second
            # walk elsewhere — the "busy" family of test_piece_list_kernel_vs_oracle as it stands.)
            for o in (3, 40, 69):
                assert over[o] == ntiles, (tile, paired, o)
            if paired and tile == 512:
                assert all(over[o] > 0 for o in busy), over
        assert all(max(ramps[o]) > rc.LIST_CAPACITY[True] for o in busy if tile == 512)
        # ---- where the bursts are, in tiles of this size of the call of this size
        inside = [(o, s) for o, s in bursts if s + 3 <= end]
        tiles = {}
        for o, s in inside:
            assert s // tile == (s + 2) // tile and s // 64 == (s + 2) // 64  # (one wave's span)
            tiles.setdefault(s // tile, []).append(o)
        assert len(tiles) >= 6, tiles
        assert 0 in tiles and ntiles - 1 in tiles
        kinds = {t: ({o in busy for o in objs}) for t, objs in tiles.items()}
        assert any(k == {True} for k in kinds.values()) and any(k == {False} for k in kinds.values()) and any(k == {True, False} for k in kinds.values())
        # the tile of the busy object's burst is one in which it takes the exact path, in both layouts
        for t, objs in tiles.items():
            for o in objs:
                if o in busy and kinds[t] == {True}:
                    assert ramps[o][t] > max(rc.LIST_CAPACITY.values())
        for wgs in (1, 3, 8):
            seqs = rc.workgroup_tiles(ntiles, wgs)
            assert sorted(t for s in seqs for t in s) == list(range(ntiles))
            interior = {t for s in seqs for t in s[1:-1]}
            assert len(interior & set(tiles)) >= 2, (tile, wgs)
            if wgs > 1:  # a tile that holds an ordinary object's burst (its wave is redone) in the middle of a workgroup's run
                assert any(t in interior and False in kinds[t] for t in tiles), (tile, wgs)


# ---- the oracle's own error -----------------------------------------------------------------------------------------------------
def _f64(s, n):
    """float64 evaluation of a scene whose curves have no two points at one time: every gain is the linear interpolation of its
    curve, held outside it (what scenes.render_f64 computes, test below)"""
    t = np.arange(s.total, dtype=np.float64)
    direct, diffuse = np.zeros((n, s.total)), np.zeros((n, s.total))
    for m, (times, d, f) in enumerate(s.curves):
        keep = np.concatenate([[True], np.diff(times) > 0])  # (a point restated at the same time restates its gains: no step)
        assert np.all(np.diff(times) >= 0) and np.array_equal(d[1:][~keep[1:]], d[:-1][~keep[1:]]) and np.array_equal(f[1:][~keep[1:]], f[:-1][~keep[1:]])
        times, d, f = times[keep], d[keep], f[keep]
        tt = times.astype(np.float64)
        xm = s.x[m].astype(np.float64)
        for c in range(n):
            direct[c] += np.interp(t, tt, d[:, c].astype(np.float64)) * xm
            if s.dec is not None:
                diffuse[c] += np.interp(t, tt, f[:, c].astype(np.float64)) * xm
    if s.dec is None:
        return direct
    out = np.zeros((n, s.total))
    for c in range(n):
        out[c] = np.convolve(diffuse[c], s.dec[c].astype(np.float64))[:s.total] + np.concatenate([np.zeros(s.delay), direct[c]])[:s.total]
    return out


def test_interpolated_float64_evaluation_is_the_suites_own():
    n = 6
    for kind in ("pieces", "hinge"):
        curves = rc.long_curves(kind, n, 2048)
        x = scenes.audio(rc.M, 2048, seed=6)
        s = rc.Scene(curves, x, None, 0, None, 512, 2048, 0)
        a, b = _f64(s, n), scenes.render_f64([(t, d, None) for t, d, _ in curves], x, n)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), kind


def _scene_list():
    out = [("long-pieces-bursts-2bus", lambda: rc.long_scene("pieces"), True), ("long-hinge-bursts-2bus", lambda: rc.long_scene("hinge"), True),
           ("long-pieces-bursts-2bus-blocks-of-128", lambda: rc.long_scene("pieces", block=rc.LONG["cut_block"]), True),
           ("long-pieces-bursts-2bus-0+5+0", lambda: rc.long_scene("pieces", layout="0+5+0"), True),
           ("long-pieces-bursts-2bus-0+5+0-blocks-of-128", lambda: rc.long_scene("pieces", block=rc.LONG["cut_block"], layout="0+5+0"), True),
           ("long-pieces-1bus", lambda: rc.long_scene("pieces", rc.CUS, False, 1, rc.long_blocks(256)), False),
           ("long-hinge-1bus", lambda: rc.long_scene("hinge", rc.CUS, False, 1, rc.long_blocks(256)), False)]
    seen = set()
    for c in rc.BY_GROUP["C"] + rc.BY_GROUP["D"]:
        key = c.scene if c.scene[0] == "grid" else (c.scene[0], 256) + c.scene[2:]
        if key not in seen:
            seen.add(key)
            out.append(("small-" + "-".join(str(v) for v in c.scene), functools.partial(rc.small_scene, *c.scene), False))
    return out


@pytest.mark.parametrize("name,make,bursts", _scene_list(), ids=[s[0] for s in _scene_list()])
def test_oracle_distance_from_float64(name, make, bursts):
    s = make()
    n = s.want.shape[0]
    truth = _f64(s, n)
    e_lib = scenes.rel_rms_per_channel(s.want, truth)
    line = f"{name}: e_lib {e_lib:.3g}"
    assert np.isfinite(truth).all() and 0 < e_lib <= 5e-7, line
    if bursts:  # the samples no burst reaches carry 1 / 200 of the energy: held on their own as well
        quiet = rc.burst_mask(s.total, rc.long_bursts(), 512, 1024)
        e_quiet = scenes.rel_rms_per_channel(s.want[:, quiet], truth[:, quiet])
        line += f", over the samples no burst reaches {e_quiet:.3g}"
        assert e_quiet <= 5e-7, line
    print(line)


def test_the_p2_wgs_sweeps_are_not_all_vacuous():
    """k_gain_mix_p2 carries a pipeline through a workgroup's tiles only where p2_persistent (gain_p2.h:517) says so — not on 256-sample
    tiles with three column tiles, where launch_pieces keeps a workgroup per tile whatever P2_WGS says.  Every piece-list case says
    what it runs, by that rule, and for every tile size, list layout and kind of B case (plain, gsplit1, cut) one case carries."""
    assert rc.column_tiles("9+10+3", 2) == 3 and rc.column_tiles("9+10+3", 1) == 2 and rc.column_tiles("0+5+0", 2) == 1
    pieces = [c for c in rc.BY_GROUP["B"] if c.kernel == rc.PIECES]
    for c in pieces:
        assert c.extra["carried"] == rc.carried(c.layout, c.buses, c.tile), c.id
        assert c.extra["carried"] == (not (c.tile == 256 and c.layout == "9+10+3")), c.id
    for tile in (256, 512):
        for paired in (False, True):
            for calls, form in (("whole", "plain"), ("whole", "wide"), ("cut", "wide")):
                assert any(c.extra["carried"] for c in pieces if (c.tile, c.paired, c.extra["calls"], c.form) == (tile, paired, calls, form)), (tile, paired, calls, form)
    for paired in (False, True):  # group E, two column tiles: P2_WGS 1 and 8 carry, the launch's own count is a workgroup per tile
        e = [c for c in rc.BY_GROUP["E"] if c.kernel == rc.PIECES and c.paired == paired]
        assert sum(c.extra["carried"] for c in e) == 2 and rc.carried(e[0].layout, 1, 256)
        auto = [c for c in e if not c.extra["carried"]]
        assert len(auto) == 1 and auto[0].opts["EARHIP_P2_WGS"] is None
        gsplit, ntiles = 2, rc.long_blocks(256) * 2
        assert max(8, (rc.CUS * 2 // gsplit) & ~7) >= ntiles  # (launch_pieces, api_core.hip:363: not fewer workgroups than tiles)


def test_case_ids_name_what_they_run():
    ids = [c.id for c in rc.CASES]
    assert len(set(ids)) == len(ids)
    for c in rc.CASES:
        assert c.id.startswith(c.group + "-") and rc.KNAME[c.kernel] in c.id and c.layout in c.id and c.id.endswith("-" + c.form), c.id
        assert f"-t{c.tile}" in c.id or c.kernel < rc.GRID, c.id  # (the kernels below 3 have one tile size each)
        assert c.form == ("none" if c.kernel < rc.GRID else c.form) and c.form in ("wide", "plain", "none"), c.id
    # every kernel kind in group D, every split-operand kernel in B and C, the list kernels in both forms
    assert {c.kernel for c in rc.BY_GROUP["D"]} == set(range(6))
    assert {c.kernel for c in rc.BY_GROUP["C"]} == {rc.GRID, rc.PIECES, rc.HINGE}
    assert {(c.kernel, c.form) for c in rc.CASES if c.kernel in (rc.PIECES, rc.HINGE)} == {(k, f) for k in (rc.PIECES, rc.HINGE) for f in ("wide", "plain")}
    for c in rc.BY_GROUP["D"]:
        assert {"ostride", "obase", "istride", "ibase"} >= {c.extra["way"]}
    assert {c.extra["way"] for c in rc.BY_GROUP["D"] if c.kernel == rc.SLOTS} == set(rc.WAYS)
