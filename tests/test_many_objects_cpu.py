"""The references of tests/many_objects_cases.py against each other, without a device: what tests/test_gpu_many_objects.py holds
the gain kernels to above 1024 objects.

  * the roll call (family `integer`): the CPU oracle returns the int64 numpy answer bit for bit, and the largest sum of
    |gain x| over a channel's objects stays below 2^24 — every partial sum of every summation order is an integer that
    float32 holds exactly, so a kernel that differs from the answer has lost, doubled or misaddressed an object;
  * every other case: e_lib, the oracle's distance from a float64 evaluation of the same curves (largest relative RMS of a
    channel), printed with the oracle's worst per-sample distance, and held to 2^-24 sqrt(M): a float32 running total of M
    terms of similar size takes M roundings of at most 2^-24 of its value each, which add up like a random walk.  Measured:
    6.2e-7 at 1024 objects, 1.7e-6 at 8193, 4.7e-6 at 65537 — a third of that bound, and far above the 1e-6 the kernels
    are held to against the oracle below 1024 objects, which is why the bars above 1024 are stated against float64."""
import numpy as np
import pytest

import many_objects_cases as mc
import scenes


def _scenes(integer):
    seen, out = set(), []
    for c in mc.CASES + [mc.builder_case(M) for M in mc.BUILDER]:
        if (c.family == "integer") == integer and mc.scene_key(c) not in seen:
            seen.add(mc.scene_key(c))
            out.append(c)
    return out


def _sid(c):
    return f"{c.family}-M{c.M}-{c.nblocks}x{c.block}-{c.layout}-{c.buses}bus"


@pytest.mark.parametrize("case", _scenes(True), ids=_sid)
def test_roll_call_is_exact_in_the_oracle(case):
    s = mc.scene(case)
    print(f"{_sid(case)}: largest sum of magnitudes {s.magnitude}")
    assert s.magnitude < 2 ** 24
    assert s.want.dtype == np.float32 and np.array_equal(s.want, s.answer)
    # (at least a quarter of the objects step inside the call)
    inside = sum(1 for t, _, _ in s.curves if len(t) > 1 and 0 < t[0] < case.block * case.nblocks)
    assert 4 * inside >= case.M


@pytest.mark.parametrize("case", _scenes(False), ids=_sid)
def test_oracle_distance_from_float64(case):
    s = mc.scene(case)
    e_lib = scenes.rel_rms_per_channel(s.want, s.truth)
    print(f"{_sid(case)}: e_lib {e_lib:.3g}, worst sample {mc.per_sample(s.want, s.truth):.3g} of the channel's peak")
    assert np.isfinite(s.truth).all() and 0 < e_lib <= 2.0 ** -24 * np.sqrt(case.M)


def test_float64_evaluation_is_the_suites_own():
    """the vectorised float64 evaluation equals scenes.render_f64 (object by object) on a small scene of every family"""
    for family, block, nb in (("grid", 256, 3), ("holding", 512, 2), ("ramping", 512, 2), ("mostly", 512, 2), ("integer", 512, 2)):
        curves = mc.make_curves(family, 37, 6, block, nb, 5)
        x = scenes.audio(37, block * nb, seed=6)
        a = mc.bus_f64(curves, x, 6, 0, chunk=16)
        b = scenes.render_f64([(t, d, None) for t, d, _ in curves], x, 6)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), family


def test_written_down_plans_are_the_host_planners():
    """the plans written down in many_objects_cases.py equal the rows of tests/golden/plan_table.txt that
    tests/cpp/test_plan_table.cpp makes for the same sizes from the statistics of the family (the roll call has no row: its
    statistics are its own)"""
    import os
    rows = {}
    with open(os.path.join(os.path.dirname(__file__), "golden", "plan_table.txt")) as f:
        for line in f:
            if line.startswith("many_"):
                w = line.split()
                rows[(w[0],) + tuple(int(v) for v in w[1:5])] = tuple(int(w[i]) for i in (6, 7, 8, 10, 12))
    checked = 0
    for c in mc.CASES:
        assert set(c.plan) == {"kernel", "tile", "ntiles", "gsplit", "layout"}, c.id
        assert c.M > 1024 or c.group == "edge"
        if c.family not in ("grid", "holding", "ramping") or c.group not in ("full", "gsplit1", "index16"):
            continue
        name = "many_holding_index16" if c.group == "index16" else f"many_{c.family}" + ("_gsplit1" if c.group == "gsplit1" else "")
        mfma = c.opts["EARHIP_MFMA"]
        kind, tile, ntiles, gsplit, paired = rows[(name, c.M, mc.n_out(c), c.block * c.nblocks, 3 if mfma is None else mfma)]
        layout = bool(paired) if kind in (mc.PIECES, mc.HINGE) else None
        assert c.plan == dict(kernel=kind, tile=tile, ntiles=ntiles, gsplit=gsplit, layout=layout), c.id
        checked += 1
    assert checked
