"""CPU oracle GainInterpolator vs the reference tests' expectations
(reference tests/gain_interpolator_tests.cpp:58-257)."""
import os

import numpy as np
import pytest

import _oracle
from refcases import chunks, expected_single, gain_interp_cases, is_approx, single_interp_expected


def test_linear_interp_single_apply_interp_closed_form():
    # :58-70  block_start=100, curve 50..250, 0.2 -> 0.8
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, 100).astype(np.float32)
    got = _oracle.gain_interp("single", [50, 250], np.float32([0.2, 0.8]).reshape(2, 1, 1), x, [100], t0=100)[0]
    want = single_interp_expected(x, 100, 50, 250, np.float64(np.float32(0.2)), np.float64(np.float32(0.8)))
    assert is_approx(got, want)
    # bit-level: same arithmetic in numpy float32
    t = np.arange(100, 200)
    p = ((t - 50).astype(np.float32) * (np.float32(1.0) / np.float32(200))).astype(np.float32)
    g = ((np.float32(1) - p) * np.float32(0.2) + p * np.float32(0.8)).astype(np.float32)
    assert np.array_equal(got, x * g)


def test_linear_interp_single_apply_constant():
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, 100).astype(np.float32)
    got = _oracle.gain_interp("single", [1000], np.float32([0.3]).reshape(1, 1, 1), x, [100])[0]
    assert np.array_equal(got, np.float32(0.3) * x)


@pytest.mark.parametrize("case", gain_interp_cases(), ids=lambda c: c[0])
def test_segmentation(case):
    name, pts, length, segs, block_sizes = case
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, length).astype(np.float32)
    want = expected_single(x, segs)
    times = [t for t, _ in pts]
    vals = np.float32([v for _, v in pts]).reshape(-1, 1, 1)
    outs = []
    for bs in block_sizes:
        got = _oracle.gain_interp("single", times, vals, x, chunks(length, bs))[0]
        assert is_approx(got, want), (name, bs)
        outs.append(got)
    for o in outs[1:]:  # chunking never changes a single bit
        assert np.array_equal(o, outs[0])


def test_vector_equals_sum_of_singles():
    # :187-219
    a, b = [0.0, 1.0], [1.0, 0.0]
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, 300).astype(np.float32)
    got = _oracle.gain_interp("vector", [100, 200], np.float32([a, b]).reshape(2, 1, 2), x, [300])
    for o in range(2):
        single = _oracle.gain_interp("single", [100, 200], np.float32([a[o], b[o]]).reshape(2, 1, 1), x, [300])[0]
        assert np.array_equal(got[o], single)


def test_matrix_equals_sum_of_singles():
    # :221-257, 3 -> 2
    a = [[0.0, 0.3], [0.5, 0.0], [0.4, 1.0]]
    b = [[0.6, 0.0], [0.0, 0.7], [1.0, 0.2]]
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (3, 300)).astype(np.float32)
    got = _oracle.gain_interp("matrix", [100, 200], np.float32([a, b]), x, [300])
    want = np.zeros((2, 300), np.float32)
    for i in range(3):
        for o in range(2):
            want[o] += _oracle.gain_interp("single", [100, 200],
                                           np.float32([a[i][o], b[i][o]]).reshape(2, 1, 1), x[i], [300])[0]
    assert np.array_equal(got, want)  # same accumulation order -> identical


def test_unsorted_points_follow_reference_search():
    # The reference's "interpolation points are not sorted" throw (gain_interpolator.hpp:123-124)
    # is unreachable: its cached linear search can never reverse direction.  Unsorted times are
    # therefore processed with whatever segment the search lands on; the restatement does the same.
    x = np.ones(400, np.float32)
    got = _oracle.gain_interp("single", [100, 300, 200], np.float32([0.0, 1.0, 0.5]).reshape(3, 1, 1), x, [400])[0]
    assert np.all(got[:100] == 0.0) and np.all(got[300:] == 0.5)
    assert np.allclose(got[100:300], np.arange(200) / 200.0, atol=1e-6)


def test_empty_points_are_an_error():
    x = np.zeros(10, np.float32)
    with pytest.raises(_oracle.OracleError):
        _oracle.gain_interp("single", [], np.zeros((0, 1, 1), np.float32), x, [10])


def test_config1_one_object_to_0_5_0_vector_closed_form():
    """BASELINE config 1 as written: 1 object -> 0+5+0 (6 channels incl. LFE1), block 512, a full-length ramp per
    block through GainInterpolator<LinearInterpVector> (gain_interpolator.hpp:53-87,214-241), against the closed
    form of the reference's own test (tests/gain_interpolator_tests.cpp:58-70: p = (float)(t - start) * (1.0f /
    (float)(end - start)), g = (1 - p) s + p e, out = in * g), bit for bit, for several chunkings of the stream."""
    from layouts import LAYOUTS
    n, block, nblocks = len(LAYOUTS["0+5+0"]), 512, 4
    assert n == 6
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, block * nblocks).astype(np.float32)
    times = [block * k for k in range(nblocks + 1)]
    vals = rng.uniform(0, 1, (nblocks + 1, 1, n)).astype(np.float32)
    vals[:, 0, 3] = 0.0  # LFE1: the gain calculators leave it at exactly zero (gain_calculator_objects.cpp:51-52)
    want = np.zeros((n, block * nblocks), np.float32)
    for k in range(nblocks):
        t = np.arange(block * k, block * (k + 1))
        p = ((t - block * k).astype(np.float32) * (np.float32(1.0) / np.float32(block))).astype(np.float32)
        for c in range(n):
            g = ((np.float32(1) - p) * vals[k, 0, c] + p * vals[k + 1, 0, c]).astype(np.float32)
            want[c, t] = x[t] * g
    for sizes in ([block] * nblocks, [block * nblocks], chunks(block * nblocks, 100)):
        got = _oracle.gain_interp("vector", times, vals, x, sizes)
        assert np.array_equal(got, want)
    assert not want[3].any()


# ---- pinned to libear's own GainInterpolator -------------------------------------------------------------------------
# (1) the committed fixture generated from it (tests/golden/make_interp_golden.py): always, so the suite checks the
#     oracle against libear where the reference is absent; (2) live, against oracle/_ref/libref_interp.so
#     (oracle/ref_interp_capi.cpp) where it was built: every fixture case, regeneration of the fixture, and a seeded
#     fuzz of ragged curves.  All bit for bit (value equality; NaN equals NaN).
from refcases import interp_golden  # noqa: E402

GEN, GOLD = interp_golden()


def same(a, b):
    nan = np.issubdtype(a.dtype, np.floating)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=nan)


def needs_ref():
    ref = _oracle.load_ref_interp()
    if ref is None:
        pytest.skip("oracle/_ref/libref_interp.so not built (reference tree absent)")
    return ref


def policy_run(lib_, g, name):
    m = GEN.meta(g, name)
    out = np.zeros_like(g[name + ".want"])
    return _oracle.ref_policy(lib_, m["kind"], g[name + ".x"], out, m["r0"], m["r1"], m["block_start"], m["start"],
                              m["end"], g[name + ".sp"], g[name + ".ep"] if m["interp"] else None)


def gi_run(lib_, g, name):
    m = GEN.meta(g, name)
    sets = GEN.gi_point_sets(g, name)
    x = g[name + ".x"]
    out = np.zeros_like(g[name + ".want"])
    gi = _oracle.RefGainInterp(lib_, m["n_in"], m["n_out"])
    ofs = 0
    for bs, n, ps in g[name + ".calls"]:
        if ps >= 0:
            gi.set_points(*sets[ps])
        if n:
            out[:, ofs:ofs + n] = gi.process(int(bs), x[:, ofs:ofs + n])
        ofs += int(n)
    return out


def render_oracle(g, name):
    """the oracle's ObjectsRenderer, direct bus only (zero decorrelators, no delay: out == direct bus), clock at t0"""
    m = GEN.meta(g, name)
    o = _oracle.ObjectsRenderer(m["M"], m["N"], m["B"], np.zeros((m["N"], 1), np.float32), 0)
    for i, (t, gains) in enumerate(GEN.render_curves(g, name)):
        o.set_points(i, 0, t, gains)
        o.set_points(i, 1, t[:1], np.zeros((1, m["N"]), np.float32))
    o.set_time(m["t0"])
    return o.process(g[name + ".x"])


def render_ref(ref, g, name):
    m = GEN.meta(g, name)
    objs = _oracle.RefObjects(ref, m["M"], m["N"])
    for i, (t, gains) in enumerate(GEN.render_curves(g, name)):
        objs.set_points(i, t, gains)
    x, B = g[name + ".x"], m["B"]
    out = np.zeros_like(g[name + ".want"])
    for b in range(m["nblocks"]):
        out[:, b * B:(b + 1) * B] = objs.process(m["t0"] + b * B, x[:, b * B:(b + 1) * B])
    return out


@pytest.mark.parametrize("name", GEN.cases(GOLD, "pol"))
def test_policy_matches_libear_fixture(name):
    assert same(policy_run(_oracle.lib(), GOLD, name), GOLD[name + ".want"])


@pytest.mark.parametrize("name", GEN.cases(GOLD, "gi"))
def test_gain_interpolator_matches_libear_fixture(name):
    assert same(gi_run(_oracle.lib(), GOLD, name), GOLD[name + ".want"])


@pytest.mark.parametrize("name", GEN.cases(GOLD, "rn"))
def test_objects_gain_stage_matches_libear_fixture(name):
    assert same(render_oracle(GOLD, name), GOLD[name + ".want"])


def test_fixture_covers_the_edges():
    """the cases the fixture must hold (a regenerated fixture that lost some would pass the comparisons above)"""
    names = set(GEN.cases(GOLD, "pol")) | set(GEN.cases(GOLD, "gi")) | set(GEN.cases(GOLD, "rn"))
    for L in GEN.RAMPS:
        assert any(n.startswith(f"rn.ramp{L}_") for n in names), L
        assert any(n.startswith(f"pol.ramp{L}_") for n in names), L
    for n_in in (1, 2, 3, 33, 64, 257):
        for n_out in (1, 2, 7, 24, 64):
            assert f"pol.shape_{n_in}x{n_out}_interp" in names and f"pol.shape_{n_in}x{n_out}_const" in names
    blocks = {GEN.meta(GOLD, n)["B"] for n in GEN.cases(GOLD, "rn")}
    objects = {GEN.meta(GOLD, n)["M"] for n in GEN.cases(GOLD, "rn")}
    assert {16, 45, 64, 480, 512, 1000, 4096} <= blocks and {1, 33, 257} <= objects
    times = {GEN.meta(GOLD, n)["t0"] for n in GEN.cases(GOLD, "rn")}
    assert min(times) < -(1 << 40) + (1 << 32) and max(times) > (1 << 40) and any(-(1 << 20) < t < 0 for t in times)
    sizes = {int(n) for c in GEN.cases(GOLD, "gi") for n in GOLD[c + ".calls"][:, 1]}
    assert {0, 1, 2, 3} <= sizes
    assert np.isnan(GOLD["rn.nan_gains.want"]).any() and np.isinf(GOLD["rn.overflow.want"]).any()
    den = GOLD["rn.denormals.want"]
    assert ((den != 0) & (np.abs(den) < np.finfo(np.float32).tiny)).any()


def test_fixture_regenerates_identically():
    ref = needs_ref()
    fresh = GEN.generate(ref)
    committed = np.load(os.path.join(os.path.dirname(os.path.abspath(GEN.__file__)), GEN.NAME))
    assert sorted(fresh) == sorted(committed.files)
    for k, v in fresh.items():
        assert same(np.asarray(v), committed[k]), k


def test_every_fixture_case_live_against_libear():
    """the oracle and the compiled reference agree on every fixture case, computed afresh on both sides"""
    ref = needs_ref()
    o = _oracle.lib()
    for name in GEN.cases(GOLD, "pol"):
        assert same(policy_run(o, GOLD, name), policy_run(ref, GOLD, name)), name
    for name in GEN.cases(GOLD, "gi"):
        assert same(gi_run(o, GOLD, name), gi_run(ref, GOLD, name)), name
    for name in GEN.cases(GOLD, "rn"):
        assert same(render_oracle(GOLD, name), render_ref(ref, GOLD, name)), name


def _fuzz_points(rng, npts, n_in, n_out, t_lo, t_hi):
    t = np.sort(rng.integers(t_lo, t_hi, npts)).astype(np.int64)
    rep = rng.random(npts) < 0.25  # steps: a time repeated
    for k in range(1, npts):
        if rep[k]:
            t[k] = t[k - 1]
    v = rng.uniform(-1, 1, (npts, n_in, n_out)).astype(np.float32)
    for k in range(1, npts):
        r = rng.random()
        if r < 0.2:
            v[k] = v[k - 1]  # bit-equal neighbours
        elif r < 0.25:
            v[k] = -v[k - 1] * 0.0  # zeros of the other sign than the previous point's
            v[k - 1] = 0.0
        elif r < 0.28:
            v[k] = np.nan
    return t, v


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_ragged_curves_against_libear(seed):
    ref = needs_ref()
    rng = np.random.default_rng(9000 + seed)
    kind = ("single", "vector", "matrix")[seed % 3]
    n_in = 1 if kind != "matrix" else int(rng.integers(1, 6))
    n_out = 1 if kind == "single" else int(rng.integers(1, 9))
    base = int(rng.choice([0, -700, 1 << 40, -(1 << 40), 123456789]))
    t, v = _fuzz_points(rng, int(rng.integers(1, 30)), n_in, n_out, base - 100, base + 900)
    sizes = [int(s) for s in rng.choice([0, 1, 2, 3, 17, 64, 129], int(rng.integers(1, 14)))]
    total = sum(sizes)
    x = rng.uniform(-1, 1, (n_in, total)).astype(np.float32)
    t0 = base + int(rng.integers(-200, 200))
    got = _oracle.gain_interp(kind, t, v, x, sizes, t0=t0)
    assert same(got, _oracle.ref_gain_interp(ref, kind, t, v, x, sizes, t0=t0))
    # a live interpolator whose points change between calls, against libear's (its search cache included)
    t2, v2 = _fuzz_points(rng, int(rng.integers(1, 30)), n_in, n_out, base - 100, base + 900)
    a, b = _oracle.RefGainInterp(_oracle.lib(), n_in, n_out), _oracle.RefGainInterp(ref, n_in, n_out)
    for gi in (a, b):
        gi.set_points(t, v)
    ofs, starts = 0, [t0 + int(s) for s in rng.integers(-300, 900, len(sizes))]
    for k, (n, bs) in enumerate(zip(sizes, starts)):
        if k == len(sizes) // 2:
            for gi in (a, b):
                gi.set_points(t2, v2)
        xs = x[:, ofs:ofs + n]
        assert same(a.process(bs, xs), b.process(bs, xs)), k
        ofs += n
    # the objects gain stage
    M, N, B, nblocks = int(rng.integers(1, 12)), int(rng.integers(1, 9)), int(rng.choice([16, 45, 64])), 4
    objs = _oracle.RefObjects(ref, M, N)
    o = _oracle.ObjectsRenderer(M, N, B, np.zeros((N, 1), np.float32), 0)
    for i in range(M):
        ti, vi = _fuzz_points(rng, int(rng.integers(1, 12)), 1, N, base - 50, base + B * nblocks + 50)
        objs.set_points(i, ti, vi[:, 0])
        o.set_points(i, 0, ti, vi[:, 0])
        o.set_points(i, 1, ti[:1], np.zeros((1, N), np.float32))
    xr = rng.uniform(-1, 1, (M, B * nblocks)).astype(np.float32)
    o.set_time(base)
    want = np.concatenate([objs.process(base + k * B, xr[:, k * B:(k + 1) * B]) for k in range(nblocks)], axis=1)
    assert same(o.process(xr), want)


def test_fixture_refuses_inputs_it_was_not_made_from(tmp_path):
    """the fixture holds libear's outputs and the digests of the inputs behind them; inputs built differently (another
    generator, another random stream) must stop the tests, not be compared with outputs of other inputs"""
    import json
    committed = np.load(os.path.join(os.path.dirname(os.path.abspath(GEN.__file__)), GEN.NAME))
    index = json.loads(str(committed["index"]))
    index[len(index) // 2]["inputs"] = "0" * 64
    path = tmp_path / "tampered.npz"
    np.savez_compressed(path, index=np.array(json.dumps(index)), want=committed["want"])
    with pytest.raises(AssertionError, match="inputs differ"):
        GEN.load(str(path))
