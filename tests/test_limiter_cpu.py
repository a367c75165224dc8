"""CPU checks of the look-ahead limiter (include/earhip.h, group N): the float64 model (tests/limiter_model.py) against known
answers, the guarantee |out| <= c (1 + 2^-22) on the model and on the shared maths header (libear_amd/csrc/limiter.h: what the
device kernels run) compiled for the host under ASan and UBSan, the header against the model under the model's bound and
bit-identical however the stream is cut, and the new symbols declared, exported and bound.

Measured by these tests (the model's output rounded to float32, its true peak over c; the cap asserted is 1.01, for L >= 64
with detect = 1):
                                                      L, H = 8, 0     64, 0     64, 480   240, 2400
    cpu_signal() of test_true_peak_cpu.py, c = 0.5:       1.02944    1.00166   1.00083   1.00010
    2-channel Gaussian noise, sigma 0.5, c = 0.891:       1.02493    1.00204   1.00067   1.00006
    the same two with detect = 0 (sample peak only):      1.708 1.488   1.676 1.445   1.674 1.199   1.671 1.172
detect = 0 promises nothing about inter-sample peaks (cpu_signal's channel 1 has a sample peak of 0.95 under a true peak of
1.35): its figures are printed and not asserted, like those of L = 8.
The host build of limiter.h lies at most at 0.108 of the bound from the model with detect = 1 (0.280 with detect = 0, where the
bound has no interpolator term), for out and for g alike."""
import os
import re
import subprocess

import numpy as np
import pytest

import limiter_model as lm
import true_peak_model as tm
from test_true_peak_cpu import cpu_signal, cuttings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 0), (64, 0), (64, 480), (240, 2400)]


def gaussian(n=48000 + 777, seed=5):
    return (0.5 * np.random.default_rng(seed).standard_normal((2, n))).astype(np.float32)


SIGNALS = {"cpu_signal": (cpu_signal, 0.5), "gaussian": (gaussian, 0.891)}
_cache = {}


def case(name, detect, L, H):
    """(x, c, the model's result, the host build's result in one call), computed once"""
    key = (name, detect, L, H)
    if key not in _cache:
        if name not in _cache:
            _cache[name] = SIGNALS[name][0]()
        x, c = _cache[name], SIGNALS[name][1]
        _cache[key] = (x, c, lm.limit(x, c, L, H, detect), lm.host_run(x, c, L, H, detect))
    return _cache[key]


def test_model_step_known_answer():
    L, H, a, b, n = 8, 5, 40, 70, 140
    x = np.zeros((1, n), np.float32)
    x[0, a:b] = 2.0
    m = lm.limit(x, 0.5, L, H, detect=False)
    g, K = m["g"], L + 1
    assert m["latency"] == L and np.all(g[:a] == 1.0)
    # from 1 to 0.25 in exactly L + 1 equal steps, ending the sample the step arrives at the output
    assert np.allclose(g[a - 1:a + L + 1], 1.0 - 0.75 * np.arange(K + 1) / K, rtol=0, atol=1e-14)
    assert g[a + L] == 0.25 and m["out"][0, a + L] == 0.5 and m["out"][0, a + L - 1] == 0.0
    # it holds H + 1 samples past the step's end (the last 2.0 leaves at b - 1 + L) and returns in L + 1 steps
    assert np.all(g[a + L:b + L + H + 1] == 0.25) and g[b + L + H + 1] > 0.25
    assert np.allclose(g[b + L + H:b + L + H + K + 1], 0.25 + 0.75 * np.arange(K + 1) / K, rtol=0, atol=1e-14)
    assert np.all(g[b + L + H + K:] == 1.0)
    assert np.all(np.abs(m["out"]) <= 0.5) and m["limited"] == (b + L + H + K) - a and m["min_gain"] == 0.25
    h = lm.host_run(x, 0.5, L, H, detect=False)
    assert np.array_equal(h["g"].astype(np.float64)[a + L:b + L + H + 1], g[a + L:b + L + H + 1]) and h["limited"] == m["limited"]


@pytest.mark.parametrize("detect", [False, True])
def test_under_the_ceiling_is_a_delay_bit_for_bit(detect):
    x = (0.3 * cpu_signal(n=9000)).astype(np.float32)  # true peak 0.3 * 1.35 * 1.4 < 0.8
    assert tm.peaks(x)["tp"].max() < 0.8
    m, h = lm.limit(x, 0.8, 64, 100, detect), lm.host_run(x, 0.8, 64, 100, detect, calls=[1, 4000, 4999])
    d = m["latency"]
    assert d == 64 + (6 if detect else 0)
    for got in (m, h):
        assert np.all(got["g"] == 1.0) and got["limited"] == 0 and got["min_gain"] == 1.0
        assert np.array_equal(np.asarray(got["out"], np.float32)[:, d:].view(np.uint32), x[:, :-d].view(np.uint32))
        assert np.all(got["out"][:, :d] == 0)
    z = np.zeros((3, 500), np.float32)
    for got in (lm.limit(z, 0.1, 8, 0, detect), lm.host_run(z, 0.1, 8, 0, detect)):
        assert np.all(got["g"] == 1.0) and np.all(got["out"] == 0)  # e = 0 throughout


@pytest.mark.parametrize("L,H", SHAPES)
@pytest.mark.parametrize("detect", [False, True])
@pytest.mark.parametrize("name", list(SIGNALS))
def test_guarantee_overshoot_and_the_header_against_the_model(name, detect, L, H):
    x, c, m, h = case(name, detect, L, H)
    assert m["limited"] > 1000 and m["min_gain"] < 0.8  # the case limits
    top = lm.guarantee(c)
    peak_m, peak_h = float(np.abs(m["out"]).max()), float(np.abs(h["out"]).max())
    print(f"{name} detect={int(detect)} L={L} H={H}: max |out| / c model {peak_m / np.float32(c):.9f} header {peak_h / np.float32(c):.9f}")
    assert peak_m <= top and peak_h <= top
    over = lm.true_peak_of(m["out"]) / float(np.float32(c))
    print(f"    true peak of the model's output over c: {over:.5f}")
    if L >= 64 and detect:
        assert over <= 1.01
    ro, rg = lm.worst_ratios(h["out"], h["g"], m, x, c, L, H, detect)
    print(f"    limiter.h on the host: worst error {ro:.3f} of the bound (out), {rg:.3f} (g)")
    assert ro <= 1.0 and rg <= 1.0
    assert abs(float(h["min_gain"]) - m["min_gain"]) <= lm.gain_bound(x, c, L, H, detect)
    assert h["min_gain"] == h["g"].min() and h["limited"] == int((h["g"] < 1).sum())


@pytest.mark.parametrize("L,H", SHAPES)
@pytest.mark.parametrize("detect", [False, True])
def test_the_cutting_changes_no_bit(detect, L, H):
    x = cpu_signal(n=40_000, seed=3)
    D, M, _, taps, _ = lm.shape(L, H, detect)
    cuts = cuttings(x.shape[1], max(taps, 2), 4)
    special = [1, 0, L, D + L, M - 1, 1]
    cuts["the histories' lengths"] = special + [x.shape[1] - sum(special)]
    runs = {name: lm.host_run(x, 0.5, L, H, detect, calls) for name, calls in cuts.items()}
    one = runs["one call"]
    assert one["limited"] > 1000
    for name, r in runs.items():
        assert np.array_equal(r["out"].view(np.uint32), one["out"].view(np.uint32)), name
        assert np.array_equal(r["g"].view(np.uint32), one["g"].view(np.uint32)), name
        assert r["min_gain"] == one["min_gain"] and r["limited"] == one["limited"], name


def test_another_table_and_non_finite_input():
    rng = np.random.default_rng(8)
    table = rng.uniform(-0.3, 0.3, (2, 24))
    table[:, 11] += 1.0
    x = rng.uniform(-1.5, 1.5, (3, 6000)).astype(np.float32)
    m, h = lm.limit(x, 0.7, 16, 30, True, table), lm.host_run(x, 0.7, 16, 30, True, [100, 5900], table)
    assert m["latency"] == 12 + 16
    ro, rg = lm.worst_ratios(h["out"], h["g"], m, x, 0.7, 16, 30, True, table)
    print(f"2 x 24 table: worst error {ro:.3f} of the bound (out), {rg:.3f} (g)")
    assert ro <= 1.0 and rg <= 1.0 and np.abs(h["out"]).max() <= lm.guarantee(0.7)
    # a NaN is ignored by the detector and stays in its own channel; an infinity gives r = 0
    x = (0.2 * rng.uniform(-1, 1, (2, 3000))).astype(np.float32)
    x[0, 500], x[1, 2000] = np.nan, np.inf
    h = lm.host_run(x, 0.5, 8, 4, True)
    d = 8 + 6
    assert np.isnan(h["out"][0, 500 + d]) and np.isfinite(h["out"][1, :2000 + d]).all() and np.isfinite(h["out"][0, :500 + d]).all()
    assert np.array_equal(h["out"][0, 501 + d:1900], x[0, 501:1900 - d]) and np.all(h["g"][:1900] == 1.0)
    assert h["min_gain"] == 0.0 and h["g"][2000 + d] == 0.0 and np.isnan(h["out"][1, 2000 + d]) and h["out"][0, 2000 + d] == 0.0


NEW_SYMBOLS = ["earhip_limiter_create", "earhip_limiter_destroy", "earhip_limiter_reset", "earhip_limiter_latency",
               "earhip_limiter_process_device", "earhip_limiter_process", "earhip_limiter_process_pcm_device",
               "earhip_limiter_output_levels", "earhip_limiter_stats", "earhip_render_attach_limiter",
               "earhip_render_limiter_position"]


def test_new_symbols_are_declared_and_exported():
    from libear_amd import build as build_lib
    path = build_lib()
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\b(earhip_\w+)\b", out))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in exported, s
    assert "typedef struct earhip_limiter_config" in header


def test_bindings_refuse_bad_arguments_without_a_device():
    """the configuration is checked before the context is looked at: every refusal of earhip_limiter_create on any machine"""
    from libear_amd import capi
    good = dict(n_channels=2, ceiling=0.5, lookahead=64, hold=480, sample_rate=48000, true_peak=True, max_samples=1000)
    bad = [dict(n_channels=0), dict(n_channels=65), dict(sample_rate=0), dict(ceiling=0.0), dict(ceiling=-1.0),
           dict(ceiling=float("inf")), dict(ceiling=float("nan")), dict(lookahead=7), dict(lookahead=1025), dict(hold=-1),
           dict(hold=8193), dict(max_samples=0), dict(max_samples=-1), dict(lookahead=64.5), dict(n_channels=True),
           dict(true_peak=(2, 3, np.zeros(5)))]
    for kw in bad:
        with pytest.raises(capi.InvalidArgument):
            capi.Limiter(None, **dict(good, **kw))
    with pytest.raises(capi.InvalidArgument, match="ctx"):
        capi.Limiter(None, **good)  # (a good configuration gets as far as the missing context)
    assert capi.load().earhip_limiter_reset(None) == capi.INVALID_ARGUMENT and capi.load().earhip_limiter_destroy(None) == capi.OK
