"""CPU checks of the programme loudness meter (include/earhip.h, group L: ITU-R BS.1770-4): the float64 model
(tests/loudness_model.py) against known answers, the host functions earhip_loudness_gate and earhip_loudness_layout_weights
against the model, the shared maths header (libear_amd/csrc/loudness.h: the code the device kernels run — the sequential cascade
and the chunked decomposition) compiled for the host against the model's step energies, and the new symbols declared and
exported.

Worst relative differences measured by test_header_cascade_and_chunked_form_against_the_model (scipy.signal.lfilter as the
model), against the bound of 1e-9: sequential 4.8e-13, chunked 2.4e-12 (L = 240, one call), 2.2e-12 (random calls), 2.1e-12
(L = 480), 9.9e-13 (L = 1): DESIGN.md section 5."""
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_model as lm
from layouts import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 48000


def tone(seconds, dbfs, hz=1000.0):
    t = np.arange(int(round(RATE * seconds))) / RATE
    return (10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * hz * t)).astype(np.float32)


def test_model_997_hz_full_scale_is_minus_3_01():
    z = lm.step_energies(tone(20, 0.0, 997.0)[None])
    assert z.shape == (200, 1)
    assert abs(lm.gate(z, [1.0])[0] - (-3.0103)) <= 0.001


def test_model_ebu_3341_case_1():
    x = tone(20, -23.0)
    got = lm.gate(lm.step_energies(np.stack([x, x])), [1.0, 1.0])[0]
    assert abs(got - (-22.9933)) <= 0.001
    assert abs(got - (-23.0)) <= 0.1


def test_model_relative_gate_drops_the_quiet_parts():
    x = np.concatenate([tone(10, -36.0), tone(60, -23.0), tone(10, -36.0)])
    z = lm.step_energies(np.stack([x, x]))
    got = lm.gate(z, [1.0, 1.0])[0]
    assert abs(got - (-23.0139)) <= 0.001
    P, l, gamma = lm.gate_details(z, [1.0, 1.0])
    dropped = (l > -70.0) & (l <= gamma)
    assert dropped.sum() >= 150  # (most of the 2 x 10 s at -36 dBFS: 97 blocks each, less those that straddle the change)
    ungated = -0.691 + 10 * np.log10(P[l > -70.0].mean())
    assert ungated < got - 0.3


def random_energies(seed, steps, channels):
    rng = np.random.default_rng(seed)
    z = 10.0 ** (rng.uniform(-10.0, 0.0, size=(steps, channels)))
    # stretches that lie below the absolute gate, and programme-like level changes
    lo = rng.integers(0, steps - 12)
    z[lo:lo + 12] *= 1e-9
    z[steps // 2:] *= 10.0 ** rng.uniform(-2.0, 0.0)
    return z


@pytest.mark.parametrize("seed,steps,channels,lfe", [(1, 40, 1, False), (2, 120, 6, True), (3, 333, 24, True), (4, 31, 2, False),
                                                     (5, 64, 5, False)])
def test_gate_against_the_model(seed, steps, channels, lfe):
    from libear_amd import capi
    z = random_energies(seed, steps, channels)
    w = np.where(np.arange(channels) % 3 == 1, 1.41, 1.0)
    if lfe:
        w[3] = 0.0
    assert lm.gate_margin(z, w) > 1e-6, "pick another seed: a block of the model lies on a gate"
    _, l, _ = lm.gate_details(z, w)
    assert (l < -70.0).any() and (l > -70.0).any()
    want = lm.gate(z, w)
    got = capi.loudness_gate(z, w)
    for g, v in zip(got, want):
        assert np.isfinite(v) and abs(g - v) <= 1e-9, (got, want)


def test_gate_with_nothing_to_measure_is_minus_infinity():
    from libear_amd import capi
    z = random_energies(7, 40, 3)
    w = [1.0, 1.0, 1.41]
    assert capi.loudness_gate(z[:3], w) == (-np.inf, -np.inf, -np.inf)
    assert capi.loudness_gate(z[:0], w) == (-np.inf, -np.inf, -np.inf)
    assert capi.loudness_gate(np.zeros((50, 3)), w) == (-np.inf, -np.inf, -np.inf)
    assert lm.gate(np.zeros((50, 3)), w) == (-np.inf, -np.inf, -np.inf)
    # 4 .. 29 steps: integrated and momentary exist, short-term does not
    got = capi.loudness_gate(z[:29], w)
    assert np.isfinite(got[0]) and np.isfinite(got[1]) and got[2] == -np.inf
    # an all-LFE programme
    assert capi.loudness_gate(z, [0.0, 0.0, 0.0]) == (-np.inf, -np.inf, -np.inf)


def test_layout_weights_follow_the_rule():
    from libear_amd import capi
    for layout, names in LAYOUTS.items():
        w = capi.loudness_layout_weights(layout)
        ch = capi.layout_channels(layout)
        assert len(w) == len(names) == len(ch)
        assert [c[0] for c in ch] == names
        want = [lm.channel_weight(az, el, lfe) for _, az, el, lfe in ch]
        assert w.tolist() == want, layout
    assert capi.loudness_layout_weights("0+5+0").tolist() == [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]
    w = dict(zip(LAYOUTS["9+10+3"], capi.loudness_layout_weights("9+10+3")))
    for name, g in w.items():
        if name.startswith("LFE"):
            assert g == 0.0
        elif name in ("M+060", "M-060", "M+090", "M-090"):
            assert g == 1.41
        else:
            assert g == 1.0, name
    assert w["M+135"] == 1.0 and w["U+090"] == 1.0 and w["B+045"] == 1.0 and w["T+000"] == 1.0
    with pytest.raises(capi.UnknownLayout):
        capi.loudness_layout_weights("1+2+3")


def cpu_signal():
    """3 channels of about 3.3 s: noise; a 40 Hz tone on a DC offset of 0.5; noise 80 dB down with 0.5 s of digital silence"""
    n = 158_761
    rng = np.random.default_rng(11)
    t = np.arange(n) / RATE
    x = np.empty((3, n), np.float32)
    x[0] = rng.uniform(-0.5, 0.5, n)
    x[1] = 0.5 + 0.25 * np.sin(2 * np.pi * 40.0 * t)
    x[2] = 1e-4 * rng.uniform(-0.5, 0.5, n)
    x[2, 60_000:84_000] = 0.0
    return x


def run_host(x, chunked, calls, chunk=240):
    lib = lm.host_lib()
    calls = np.asarray(calls, np.uint64)
    assert int(calls.sum()) == x.shape[1]
    cap = x.shape[1] // 4800 + 1
    z = np.zeros((cap, x.shape[0]))
    for c in range(x.shape[0]):
        row = np.ascontiguousarray(x[c])
        col = np.zeros(cap)
        n = lib.loud_run(int(chunked), 4800, chunk, row.ctypes.data, calls.ctypes.data, calls.size, col.ctypes.data, cap)
        assert n == x.shape[1] // 4800
        z[:, c] = col
    return z[:x.shape[1] // 4800]


def test_header_cascade_and_chunked_form_against_the_model():
    assert lm._lfilter is not None, "the reference of this test is scipy.signal.lfilter itself (the CPU suite has scipy)"
    x = cpu_signal()
    want = lm.step_energies(x)
    assert want.shape == (33, 3)
    n = x.shape[1]
    rng = np.random.default_rng(3)
    cuts = [1, 239, 241, 0, 4800, 4799]
    while sum(cuts) < n - 30_000:
        cuts.append(int(rng.integers(1, 30_000)))
    cuts.append(n - sum(cuts))
    for name, chunked, calls, chunk in (("sequential", 0, [n], 240), ("chunked, one call", 1, [n], 240),
                                        ("chunked, random calls", 1, cuts, 240), ("chunked, L = 480", 1, cuts, 480),
                                        ("chunked, L = 1", 1, [n], 1)):
        ok, worst = lm.within_bound(run_host(x, chunked, calls, chunk), want)
        print(f"{name}: worst relative difference {worst:.3e} ({worst / 1e-9:.2%} of the bound)")
        assert ok, (name, worst)
    assert lm.host_lib().loud_chunk_length(4800, 240) == 240 and lm.host_lib().loud_chunk_length(4410, 240) == 210


def test_host_cascade_that_stands_in_for_scipy_is_pinned_to_it():
    assert lm._lfilter is not None, "the CPU suite has scipy"
    x = cpu_signal()
    for c in range(3):
        a, b = lm.k_weight(x[c], use_scipy=True), lm.k_weight(x[c], use_scipy=False)
        assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(a))


NEW_SYMBOLS = ["earhip_loudness_create", "earhip_loudness_destroy", "earhip_loudness_reset", "earhip_loudness_process_device",
               "earhip_loudness_process", "earhip_loudness_num_steps", "earhip_loudness_steps", "earhip_loudness_result",
               "earhip_loudness_gate", "earhip_loudness_layout_weights", "earhip_render_attach_loudness"]


def test_new_symbols_are_declared_and_exported():
    from libear_amd import build as build_lib
    path = build_lib()
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\b(earhip_\w+)\b", out))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in exported, s
