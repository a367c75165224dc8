"""CPU checks of the true-peak meter and the loudness range (include/earhip.h, group L: ITU-R BS.1770-4 annex 2, EBU Tech 3342):
the float64 model (tests/true_peak_model.py) against known answers, the shared maths header (libear_amd/csrc/true_peak.h: what
the device kernels run) compiled for the host against the model, earhip_loudness_range against the model, and the new symbols
declared and exported.

Measured by these tests: the header's float32 interpolator lies at 0.098 of the bound (taps + 1) 2^-24 A X_c from the model
(worst channel of full-scale noise, inter-sample overs, a quiet tone on DC, bursts; default table), 0.062 with a 2 x 24 table
at 96 kHz, 0.333 with a single tap; the model reads -5.932 and -5.938 dBTP for the 0.5-amplitude quarter-rate sine at 0 and
45 degrees; the four Tech 3342 programmes give 10, 5, 20 and 15 LU within 1e-7."""
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_model as lm
import true_peak_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, STEP = 48000, 4800


def quarter_rate_sine(phase_deg, n=RATE):
    return (0.5 * np.sin(2 * np.pi * np.arange(n) / 4.0 + np.deg2rad(phase_deg))).astype(np.float32)


def test_default_table_is_annex_2():
    h = tm.default_table()
    assert h.shape == (4, 12)
    full = h.T.reshape(-1)  # interleaved: tap 4 k + p
    assert np.array_equal(full, full[::-1])  # the 48-tap filter is symmetric
    assert np.array_equal(h * 8192, np.round(h * 8192)) and np.array_equal(h.astype(np.float32).astype(np.float64), h)
    assert abs(tm.table_gain(h) - 2.023) < 5e-4
    w = 2 * np.pi * np.arange(0, 24001, 250) / (4 * RATE)
    gain = np.abs(np.exp(-1j * np.outer(w, np.arange(48))) @ full)
    f = np.arange(0, 24001, 250)
    assert gain[f <= 20000].min() >= 3.949 and gain[f <= 20000].max() <= 4.05  # (3.9492 at DC: the coefficients sum to 32353 / 8192)
    w = 2 * np.pi * np.arange(30000, 96001, 250) / (4 * RATE)
    assert np.abs(np.exp(-1j * np.outer(w, np.arange(48))) @ full).max() < 0.041
    got = np.zeros(48)
    tm.host_lib().tp_default_table(got.ctypes.data)
    assert np.array_equal(got.reshape(4, 12), h)


def test_model_known_answers():
    for deg in (0.0, 45.0):
        p = tm.peaks(quarter_rate_sine(deg)[None])
        db = float(tm.dbtp(p["tp"][0]))
        print(f"quarter-rate sine, amplitude 0.5, {deg:g} degrees: {db:.3f} dBTP, sample peak {float(tm.dbtp(p['sp'][0])):.3f} dBFS")
        assert -6.0 - 0.4 <= db <= -6.0 + 0.2  # EBU Tech 3341's tolerance
        assert p["step_tp"].shape == (10, 1) and p["tp"][0] == max(p["step_tp"].max(), p["open_tp"][0])
    assert abs(float(tm.dbtp(p["sp"][0])) - (-9.03)) <= 0.005  # (the 45 degree tone: every sample is 0.5 sin 45)
    # a tone that is not at a quarter of the rate, faded in: the true peak is the amplitude
    n = RATE
    x = 0.5 * np.sin(2 * np.pi * 6000.0 * np.arange(n) / RATE + np.deg2rad(67.5)) * np.minimum(np.arange(n) / 4800.0, 1.0)
    db = float(tm.dbtp(tm.peaks(x.astype(np.float32)[None])["tp"][0]))
    assert -6.0 - 0.4 <= db <= -6.0 + 0.2, db


def cpu_signal(n=3 * RATE + 1234, seed=11):
    """uniform noise at full scale; inter-sample overs (sample peak < 1, true peak > 1); a quiet tone on a DC offset; digital
    silence between two bursts"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    x = np.zeros((4, n), np.float32)
    x[0] = rng.uniform(-1.0, 1.0, n)
    x[1] = 1.35 * np.sin(2 * np.pi * np.arange(n) / 4.0 + np.pi / 4) * np.minimum(np.arange(n) / 2000.0, 1.0)
    x[2] = 0.25 + 1e-3 * np.sin(2 * np.pi * 997.0 * t)
    x[3, 1000:9000] = rng.uniform(-0.3, 0.3, 8000)
    x[3, -3000:] = rng.uniform(-0.6, 0.6, 3000)
    return x


def cuttings(n, taps, seed):
    rng = np.random.default_rng(seed)
    cuts = [1, 0, taps - 1, taps, STEP - taps - 1, 1, STEP, STEP - 1]
    while sum(cuts) < n - 30_000:
        cuts.append(int(rng.integers(1, 30_000)))
    cuts.append(n - sum(cuts))
    short = [int(v) for v in rng.integers(0, taps, size=300)]
    return {"one call": [n], "random calls": cuts, "calls shorter than taps first": short + [n - sum(short)]}


@pytest.mark.parametrize("table,rate", [(None, 48000), ("2x24", 96000), ("1x1", 48000)])
def test_header_interpolator_against_the_model(table, rate):
    if table == "2x24":
        rng = np.random.default_rng(5)
        table = rng.uniform(-0.4, 0.4, (2, 24))
        table[:, 11] += 1.0
    elif table == "1x1":
        table = np.array([[-0.75]])
    taps = 12 if table is None else table.shape[1]
    x = cpu_signal()
    want = tm.peaks(x, table, rate)
    assert want["sp"][1] < 1.0 < want["tp"][1] or table is not None  # the overs channel
    runs = {}
    for name, calls in cuttings(x.shape[1], taps, 3).items():
        got = [tm.host_run(x[c], calls, table, rate) for c in range(x.shape[0])]
        tp, sp = np.stack([g[0] for g in got], 1), np.stack([g[1] for g in got], 1)
        op = np.stack([g[2] for g in got], 1)  # [2][C]
        runs[name] = (tp, sp, op)
        assert np.array_equal(sp.astype(np.float64), want["step_sp"]) and np.array_equal(op[1].astype(np.float64), want["open_sp"])
        r = max(tm.worst_ratio(tp, want["step_tp"], table, want["sp"]), tm.worst_ratio(op[0], want["open_tp"], table, want["sp"]))
        print(f"true_peak.h on the host, {name}: worst error {r:.3f} of the bound")
        assert r <= 1.0, (name, r)
    for name in runs:
        for a, b in zip(runs[name], runs["one call"]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name  # the cutting changes no bit


def test_nan_and_infinity_in_the_header_and_the_model():
    x = np.zeros(2 * STEP, np.float32)
    x[100], x[200] = 0.5, np.nan
    x[STEP + 50] = -np.inf
    tp, sp, _ = tm.host_run(x, [x.size])
    want = tm.peaks(x[None])
    assert sp[0] == 0.5 and np.isfinite(tp[0]) and tp[0] >= 0.48  # the NaN and every y it touches are ignored
    assert sp[1] == np.inf and tp[1] == np.inf
    assert np.array_equal(sp.astype(np.float64), want["step_sp"][:, 0]) and want["step_tp"][1, 0] == np.inf
    assert tm.worst_ratio(tp[:1], want["step_tp"][:1, 0], None, 0.5) <= 1.0


def test_table_setup_shared_by_the_meter_and_the_limiter_on_cpu(tmp_path):
    """libear_amd/csrc/true_peak.h, tp_table_make (what earhip_loudness_create_tp and earhip_limiter_create are made with): the
    built-in table, callers' tables of the extreme shapes, h for 4 x 12 alone, every refusal's message — under ASan + UBSan"""
    exe = tmp_path / "test_tp_table"
    src = os.path.join(ROOT, "tests", "cpp", "test_tp_table.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libear_amd", "csrc"), src, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(res.stdout)
    assert res.returncode == 0, res.stdout


# ---- loudness range ---------------------------------------------------------------------------------------------------------------
def programme(levels, seconds=20.0):
    t = np.arange(int(round(RATE * seconds))) / RATE
    x = np.concatenate([10.0 ** (db / 20.0) * np.sin(2 * np.pi * 1000.0 * t) for db in levels]).astype(np.float32)
    return np.stack([x, x])


@pytest.mark.parametrize("levels,lra", [((-20, -30), 10.0), ((-20, -15), 5.0), ((-40, -20), 20.0), ((-50, -35, -20, -35, -50), 15.0)])
def test_range_of_the_tech_3342_programmes(levels, lra):
    from libear_amd import capi
    z = lm.step_energies(programme(levels))
    want = tm.loudness_range(z, [1.0, 1.0])
    got = capi.loudness_range(z, [1.0, 1.0])
    print(f"levels {levels}: model LRA {want[0]:.9f} LU ({want[1]:.4f} .. {want[2]:.4f} LKFS), library {got[0]:.9f}")
    assert abs(want[0] - lra) <= 1.0  # EBU's tolerance, for the model
    assert all(abs(g - v) <= 1e-9 for g, v in zip(got, want)), (got, want)


def random_energies(seed, steps, channels):
    rng = np.random.default_rng(seed)
    z = 10.0 ** (rng.uniform(-6.0, 0.0, size=(steps, channels)))
    for _ in range(4):  # programme-like level changes, some below the relative gate, one stretch below the absolute gate
        lo = int(rng.integers(0, steps - 40))
        z[lo:lo + int(rng.integers(20, 80))] *= 10.0 ** rng.uniform(-4.0, 0.0)
    lo = int(rng.integers(0, steps - 50))
    z[lo:lo + 50] *= 1e-9
    return z


@pytest.mark.parametrize("seed,steps,channels", [(1, 200, 1), (2, 333, 6), (3, 600, 24), (4, 64, 2), (5, 30, 3)])
def test_range_against_the_model(seed, steps, channels):
    from libear_amd import capi
    z = random_energies(seed, steps, channels) if steps > 90 else 10.0 ** np.random.default_rng(seed).uniform(-3, 0, (steps, channels))
    w = np.where(np.arange(channels) % 3 == 1, 1.41, 1.0)
    if channels > 3:
        w[3] = 0.0
    assert tm.range_margin(z, w) > 1e-6, "pick another seed: a window of the model lies on a gate"
    _, l, gamma = tm.range_details(z, w)
    if steps > 90:
        assert (l < -70.0).any() and ((l > -70.0) & (l <= gamma)).any() and (l > gamma).any()
    want = tm.loudness_range(z, w)
    got = capi.loudness_range(z, w)
    assert np.isfinite(want).all() and all(abs(g - v) <= 1e-9 for g, v in zip(got, want)), (got, want)


def test_range_with_nothing_to_measure():
    from libear_amd import capi
    z = random_energies(7, 120, 3)
    w = [1.0, 1.0, 1.41]
    empty = (0.0, -np.inf, -np.inf)
    assert capi.loudness_range(z[:29], w) == empty and tm.loudness_range(z[:29], w) == empty
    assert capi.loudness_range(z[:0], w) == empty
    assert capi.loudness_range(np.zeros((50, 3)), w) == empty and tm.loudness_range(np.zeros((50, 3)), w) == empty
    assert capi.loudness_range(z * 1e-12, w) == empty  # everything under the absolute gate
    assert capi.loudness_range(z, [0.0, 0.0, 0.0]) == empty
    got = capi.loudness_range(z[:30], w)  # one window: low = high
    assert got[0] == 0.0 and np.isfinite(got[1]) and got[1] == got[2]


NEW_SYMBOLS = ["earhip_loudness_create_tp", "earhip_loudness_peaks", "earhip_loudness_step_peaks", "earhip_loudness_range",
               "earhip_loudness_result_range"]


def test_new_symbols_are_declared_and_exported():
    from libear_amd import build as build_lib
    path = build_lib()
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\b(earhip_\w+)\b", out))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in exported, s
    assert "typedef struct earhip_true_peak" in header
