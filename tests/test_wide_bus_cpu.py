"""The references of tests/wide_bus_cases.py against each other and the column plans of its widths, without a device: what
tests/test_gpu_wide_bus.py holds the render path to beyond 24 loudspeakers.

  * ColumnPlan::make at 48, 49, 50, 64, 96, 98, 194 and 386 columns against answers typed in by hand (tests/cpp/test_column_plan.cpp),
    and the same numbers in the case table;
  * every scene but the roll call: e_lib, the oracle's distance from scenes.render_f64 (largest relative RMS of a channel), printed
    and held to 6.2e-7 — the project's figure for libear at 1024 objects: with at most 288 objects the oracle stays well
    inside it (measured 2.0e-7 .. 3.2e-7), which keeps the 1e-6 the kernels are held to against the oracle meaningful;
  * the roll call (family `integer`): the oracle returns the int64 answer bit for bit, as in tests/test_many_objects_cpu.py;
  * the `scales` and `tiles` scenes do to the columns what their descriptions say."""
import os
import subprocess

import numpy as np
import pytest

import many_objects_cases as mc
import scenes
import wide_bus_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sid(c):
    return f"{c.family}-{c.layout}x{c.buses}-M{c.M}-{c.nblocks}x{c.block}"


def test_column_plans_known_answers(tmp_path):
    exe = tmp_path / "test_column_plan"
    src = os.path.join(ROOT, "tests", "cpp", "test_column_plan.cpp")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "libear_amd", "csrc"), src,
                    "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    # the program's table is the case table's (its lines: "<cols> columns: nout a ngroups b nz c nct d mgroups e mnz f row g")
    seen = {}
    for line in res.stdout.splitlines():
        w = line.split()
        if len(w) == 16:
            seen[int(w[0])] = tuple(int(v) for v in w[3::2])
    assert seen == wc.COLUMN_PLANS
    assert {wc.columns(c) for c in wc.CASES} == set(wc.COLUMN_PLANS) - {48}


def test_the_case_table_is_whole():
    """every width with every family on every kernel, no case whose plan names a kernel the rules do not give it, and each of
    the six kernel kinds planned at 50, 64 and 98 columns"""
    for N, K in wc.WIDTHS:
        for family in wc.FAMILIES:
            got = [c for c in wc.CASES if (c.layout, c.buses, c.family, c.group) == (N, K, family, "width")]
            assert [c.opts["EARHIP_MFMA"] for c in got] == list(mc.KERNELS)
            assert all(c.M == 96 and c.block * c.nblocks == 1024 for c in got)
    for c in wc.CASES + wc.STRICT_CASES:
        assert set(c.plan) == {"kernel", "tile", "ntiles", "gsplit", "layout"}, c.id
        assert c.plan["ntiles"] * c.plan["tile"] >= c.block * c.nblocks > (c.plan["ntiles"] - 1) * c.plan["tile"], c.id
        forced = c.opts.get("EARHIP_MFMA")
        if forced in (4, 5, 6):  # (a forced split-operand kernel is the one that runs: nothing here is beyond its limits)
            assert c.plan["kernel"] == {4: mc.GRID, 5: mc.PIECES, 6: mc.HINGE}[forced], c.id
        if forced == 1:
            assert c.plan["kernel"] in (mc.SLOTS, mc.F32GRID), c.id
    for cols in wc.COVERAGE_COLUMNS:
        kinds = {c.plan["kernel"] for c in wc.CASES + wc.STRICT_CASES if wc.columns(c) == cols}
        assert kinds == set(range(6)), (cols, kinds)


@pytest.mark.parametrize("case", wc.distinct_scenes(False), ids=_sid)
def test_oracle_distance_from_float64(case):
    s = wc.scene(case)
    e_lib = scenes.rel_rms_per_channel(s.want, s.truth)
    print(f"{_sid(case)}: e_lib {e_lib:.3g}, worst sample {mc.per_sample(s.want, s.truth):.3g} of the channel's peak")
    assert s.want.shape == (case.layout, case.block * case.nblocks) and np.isfinite(s.truth).all()
    assert 0 < e_lib <= 6.2e-7


@pytest.mark.parametrize("case", wc.distinct_scenes(True), ids=_sid)
def test_roll_call_is_exact_in_the_oracle(case):
    s = wc.scene(case)
    print(f"{_sid(case)}: largest sum of magnitudes {s.magnitude}")
    assert s.magnitude < 2 ** 24
    assert s.want.dtype == np.float32 and np.array_equal(s.want, s.answer)
    # (every channel is fed where there are objects enough, and at least a quarter of the objects step inside the call)
    assert np.count_nonzero(np.abs(s.answer).sum(axis=1)) == min(case.layout, case.M)
    inside = sum(1 for t, _, _ in s.curves if len(t) > 1 and 0 < t[0] < case.block * case.nblocks)
    assert 4 * inside >= case.M


@pytest.mark.parametrize("N,K", ((25, 2), (32, 2)))
def test_scales_scene_separates_neighbouring_columns(N, K):
    """the largest gain of a column, as a power of two, left and right of the boundaries the case table names: 2^12 apart"""
    curves = wc.make_curves("holding+scales", 96, N, K, 512, 2, 11)
    cmax = np.max([np.max(np.abs(np.concatenate([d, f], axis=1)), axis=0) for _, d, f in curves], axis=0)
    e = np.floor(np.log2(cmax)).astype(int)  # (the largest of some hundred uniform(0, 1) gains is in [0.5, 1): the binade is the factor's)
    boundaries = ((15, 16), (31, 32), (47, 48)) if N == 32 else ((15, 16), (24, 25))
    print(N, K, e.tolist())
    assert len(e) == N * K
    for a, b in boundaries:
        assert abs(e[a] - e[b]) == 12, (N, a, b, e[a], e[b])


@pytest.mark.parametrize("N,K", ((25, 2), (32, 2), (49, 2)))
def test_tiles_scene_gives_every_column_tile_its_own_scale(N, K):
    """the binade of a column's largest gain is constant over a 16-column tile, 4 apart between neighbouring tiles of a group and
    12 or 8 apart between the same tile of two groups"""
    curves = wc.make_curves("ramping+tiles", 96, N, K, 512, 2, 13)
    cmax = np.max([np.max(np.abs(np.concatenate([d, f], axis=1)), axis=0) for _, d, f in curves], axis=0)
    e = np.floor(np.log2(cmax)).astype(int)
    print(N, K, e.tolist())
    assert len(e) == N * K
    for j in range(N * K):
        assert e[j] == -1 - 4 * ((j // 16) % 4), j
    for j in range(48, N * K):  # (the column one and two groups back)
        assert abs(e[j] - e[j - 48]) in (4, 12) and (j < 96 or abs(e[j] - e[j - 96]) == 8), j


def test_written_down_plans_are_the_host_planners():
    """the plans written down in wide_bus_cases.py for 96 objects on 2 blocks of 512 at 50, 64 and 98 columns equal the rows of
    tests/golden/plan_table.txt that tests/cpp/test_plan_table.cpp makes for the same sizes from the statistics of the family (the
    roll call has no row: its statistics are its own)"""
    rows = {}
    with open(os.path.join(ROOT, "tests", "golden", "plan_table.txt")) as f:
        for line in f:
            if line.startswith("wide_"):
                w = line.split()
                rows[(w[0],) + tuple(int(v) for v in w[1:5])] = tuple(int(w[i]) for i in (6, 7, 8, 10, 12))
    checked = 0
    for c in wc.CASES:
        if c.family not in ("grid", "holding", "ramping") or c.group != "width" or wc.columns(c) not in wc.COVERAGE_COLUMNS:
            continue
        mfma = c.opts["EARHIP_MFMA"]
        kind, tile, ntiles, gsplit, paired = rows[(f"wide_{c.family}", c.M, wc.columns(c), c.block * c.nblocks, 3 if mfma is None else mfma)]
        layout = bool(paired) if kind in (mc.PIECES, mc.HINGE) else None
        assert c.plan == dict(kernel=kind, tile=tile, ntiles=ntiles, gsplit=gsplit, layout=layout), c.id
        checked += 1
    assert checked == 3 * 3 * 6
