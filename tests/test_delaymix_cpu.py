"""CPU checks of the delay matrix (include/earhip.h, group S): the host form of the shared maths header
(libear_amd/csrc/delaymix.h: the checks, the tables, the history rule and the fmaf chain the device kernel runs) compiled for the
host under ASan and UBSan against the float64 model under the derived bound of tests/delaymix_model.py, the same bits under
every cutting of the stream, the exact properties of the header (a pure delay, silence, the order of the sum, the NaN rule),
the two designers against numpy, every refusal that needs no device, and the new symbols declared, exported and bound.

Measured by these tests (worst |y - ref| as a share of the bound gamma_K S + K 2^-149, 607 samples): 0.996 for the delayed gains
(K = 1, one product: half an ulp against gamma_1 = u / (1 - u), as close as any correct form gets), 0.979 for T = 1, 2, 16, 32
(its T = 1 row again), 0.152 for 18 products into one output, 0.434 for the full matrix; the same for every cutting (the bits
are)."""
import os
import re
import subprocess

import numpy as np
import pytest

import delaymix_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 607


@pytest.mark.parametrize("name", list(dm.CASES))
def test_host_form_against_the_model_and_the_same_bits_under_every_cutting(name):
    n_in, n_out, routes = dm.CASES[name]
    x = dm.noise(n_in, N, seed=len(name))
    for c in dm.unread(n_in, routes):
        x[c] = np.nan  # an input without a route is never read
    ref, S, K = dm.model(x, n_out, routes)
    one = None
    for cut, calls in dm.cuttings(N, dm.history(routes)).items():
        y = dm.host_run(x, n_out, routes, calls)
        worst = dm.worst_ratio(y, ref, S, K)
        print(f"{name}, {cut}: worst error {worst:.3f} of the bound")
        assert worst <= 1.0, cut
        one = y if one is None else one
        assert np.array_equal(dm.bits(y), dm.bits(one)), cut


def test_a_unit_tap_returns_the_inputs_bits_behind_d_zeros_and_silence_gives_zero():
    x = dm.noise(3, N, seed=7)
    x[0, 5], x[0, 6], x[0, 7] = -0.0, 1e-42, -1e-45  # a negative zero and subnormals keep their bits
    x[2] = 0.0
    D = (0, 37, 64)
    y = dm.host_run(x, 3, [(c, c, D[c], [1.0]) for c in range(3)], [100, 1, N - 101])
    for c in range(2):
        # (+0.0 + -0.0 is +0.0: the chain starts from +0.0, so a negative zero comes out positive; every other sample keeps its bits)
        want = np.concatenate([np.zeros(D[c], np.float32), x[c, :N - D[c]]]) + np.float32(0.0)
        assert np.array_equal(y[c].view(np.uint32), want.view(np.uint32)), c
        assert not y[c, :D[c]].view(np.uint32).any()
    assert not y[2].view(np.uint32).any()  # silence in, +0.0 out


def test_routes_into_one_output_are_summed_in_list_order():
    """fmaf(1, c, fmaf(1, b, fmaf(1, a, +0))) = (a + b) + c: with a = 1, b = 2^-24, c = 2^-24 the list order a, b, c gives 1
    (each half-ulp tie rounds to even) and c, b, a gives 1 + 2^-23"""
    x = np.zeros((3, 4), np.float32)
    x[0], x[1], x[2] = 1.0, 2.0 ** -24, 2.0 ** -24
    fwd = dm.host_run(x, 1, [(0, 0, 0, [1.0]), (1, 0, 0, [1.0]), (2, 0, 0, [1.0])])
    rev = dm.host_run(x, 1, [(2, 0, 0, [1.0]), (1, 0, 0, [1.0]), (0, 0, 0, [1.0])])
    assert (fwd == np.float32(1.0)).all() and (rev == np.float32(1.0 + 2.0 ** -23)).all()
    assert not np.array_equal(dm.bits(fwd), dm.bits(rev))


def test_a_nan_reaches_exactly_the_outputs_whose_window_holds_it():
    n_in, n_out, routes = dm.CASES["a full matrix"]
    x = dm.noise(n_in, N, seed=5)
    clean = dm.host_run(x, n_out, routes)
    for c, s in ((0, 200), (1, 0), (2, N - 140)):
        bad = x.copy()
        bad[c, s] = np.nan
        y = dm.host_run(bad, n_out, routes, [150, 100, 57, N - 307])
        hit = np.zeros((n_out, N), bool)
        n = np.arange(N)
        for i, o, d, h in dm.routes32(routes):
            if i == c:
                hit[o] |= (n - d - h.size + 1 <= s) & (s <= n - d)
        assert hit.any() and not np.isfinite(y[hit]).any(), (c, s)
        assert np.array_equal(dm.bits(y[~hit]), dm.bits(clean[~hit])), (c, s)


def np_fractional(delay, T, beta):
    if T == 1:
        return int(np.floor(delay + 0.5)), np.array([1.0])
    c = T // 2 - 1
    whole = int(np.floor(delay - c))
    mu = delay - c - whole
    t = np.arange(T) - c - mu
    h = np.sinc(t) * np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * t / T) ** 2))) / np.i0(beta)
    return whole, h / h.sum()


def test_fractional_designer_against_numpy():
    from libear_amd import capi
    for delay, T, beta in ((20.3, 16, 8.0), (100.999, 32, 10.0), (0.0, 2, 0.0), (0.5, 2, 3.0), (7.0, 16, 8.0), (65536.0 + 15.25, 32, 6.0),
                           (3.49, 1, 8.0), (3.5, 1, 8.0), (0.0, 1, 0.0), (65536.4, 1, 1.0), (1.75, 4, 5.0)):
        whole, h = capi.delaymix_fractional(delay, T, beta)
        want_whole, want = np_fractional(delay, T, beta)
        assert whole == want_whole and h.shape == want.shape, (delay, T)
        assert np.abs(h - want).max() <= 1e-12 * np.abs(want).max(), (delay, T, beta, np.abs(h - want).max())
        assert abs(h.sum() - 1.0) <= 1e-12
    assert capi.delaymix_fractional(20.3, 16, 8.0)[0] == 13 and capi.delaymix_fractional(100.999, 32, 10.0)[0] == 85
    # the group delay of these two designs over [0, fs / 4], in samples (measured: 6.4e-4 and 7.0e-7)
    for delay, T, beta, tol in ((20.3, 16, 8.0, 1e-3), (100.999, 32, 10.0, 1e-6)):
        whole, h = capi.delaymix_fractional(delay, T, beta)
        w = np.linspace(1e-3, np.pi / 2, 512)
        e = np.exp(-1j * np.outer(w, np.arange(T)))
        gd = np.real((e * (np.arange(T) * h)).sum(axis=1) / (e * h).sum(axis=1)) + whole
        print(f"T={T} beta={beta} delay={delay}: group-delay error {np.abs(gd - delay).max():.1e} samples")
        assert np.abs(gd - delay).max() <= tol


def test_align_designer_against_numpy():
    from libear_amd import capi
    d = np.array([2.0, 3.5, 1.25, 3.5, 0.8])
    for rate, speed in ((48000.0, 343.0), (44100.0, 340.29)):
        delay, gain = capi.delaymix_align(d, rate, speed)
        want_delay, want_gain = (d.max() - d) / speed * rate, d / d.max()
        assert np.abs(delay - want_delay).max() <= 1e-12 * want_delay.max() and np.abs(gain - want_gain).max() <= 1e-12
        assert delay[1] == 0.0 and gain[1] == 1.0
    assert capi.delaymix_align([2.0], 48000.0)[0].tolist() == [0.0]


def test_designer_refusals():
    from libear_amd import capi
    nan, inf = float("nan"), float("inf")
    for args in ((1.0, 3), (1.0, 0), (1.0, 33), (1.0, 34), (1.0, -2), (-0.5, 1), (nan, 1), (inf, 1), (65536.6, 1), (1.0, 16, -1.0),
                 (1.0, 16, nan), (1.0, 16, inf), (6.9, 16), (0.9, 4), (65536.0 + 16.0, 32), (1.0, 2.5), (1.0, True)):
        with pytest.raises(capi.InvalidArgument):
            capi.delaymix_fractional(*args)
    lib = capi.load()
    assert lib.earhip_delaymix_fractional(1.0, 1, 8.0, None, None) == capi.INVALID_ARGUMENT
    for args in (([], 48000.0), ([1.0, 0.0], 48000.0), ([1.0, -1.0], 48000.0), ([1.0, nan], 48000.0), ([1.0, inf], 48000.0),
                 ([1.0], 0.0), ([1.0], -48000.0), ([1.0], nan), ([1.0], 48000.0, 0.0), ([1.0], 48000.0, -1.0), ([1.0], 48000.0, inf)):
        with pytest.raises(capi.InvalidArgument):
            capi.delaymix_align(*args)
    assert lib.earhip_delaymix_align(1, None, 48000.0, 343.0, None, None) == capi.INVALID_ARGUMENT


def test_host_program_refuses_what_create_refuses():
    x = np.zeros((2, 8), np.float32)
    one = np.ones(1, np.float32)
    ok = (0, 1, 5, 1, one)
    for n_out, raw, word in ((65, [ok], "n_out must"), (2, [ok] * 513, "n_routes must"), (2, [], "n_routes must"),
                             (2, [(2, 1, 5, 1, one)], "in must"), (2, [(-1, 1, 5, 1, one)], "in must"), (2, [(0, 2, 5, 1, one)], "out must"),
                             (2, [(0, 1, -1, 1, one)], "delay must"), (2, [(0, 1, 65537, 1, one)], "delay must"),
                             (2, [(0, 1, 5, 0, one)], "n_taps must"), (2, [(0, 1, 5, 33, one)], "n_taps must"),
                             (2, [ok, (0, 1, 5, 2, [1.0, np.nan])], "finite"), (2, [(0, 1, 5, 3, [1.0, 2.0, np.inf])], "finite")):
        assert word in dm.host_run(x, n_out, None, expect=3, raw_routes=raw), (n_out, raw)
    assert "n_in must" in dm.host_run(np.zeros((65, 8), np.float32), 2, None, expect=3, raw_routes=[ok])
    # the limits themselves are fine: a tap beyond n_taps is not looked at
    y = dm.host_run(x, 2, None, raw_routes=[(0, 1, 65536, 32, np.ones(32, np.float32)), (1, 0, 0, 1, [1.0, np.nan])])
    assert not y.any()


NEW_SYMBOLS = ["earhip_delaymix_create", "earhip_delaymix_destroy", "earhip_delaymix_reset", "earhip_delaymix_info",
               "earhip_delaymix_process_device", "earhip_delaymix_process", "earhip_delaymix_fractional", "earhip_delaymix_align"]


def test_new_symbols_are_declared_exported_and_bound():
    from libear_amd import build as build_lib
    path = build_lib()
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\b(earhip_\w+)\b", out))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in exported, s
    for t in ("earhip_delaymix_route", "earhip_delaymix_config", "earhip_delaymix_properties"):
        assert "typedef struct " + t in header
    from libear_amd import capi
    assert hasattr(capi, "DelayMatrix") and hasattr(capi, "delaymix_fractional") and hasattr(capi, "delaymix_align")
    mirror = open(os.path.join(ROOT, "libear_amd", "host", "ear", "hip_delaymix.hpp")).read()
    assert "class DelayMatrix" in mirror and "struct Route" in mirror and "alignment(" in mirror


def test_bindings_refuse_bad_arguments_without_a_device():
    """the configuration is checked before the context is looked at: every refusal of earhip_delaymix_create on any machine"""
    from libear_amd import capi
    nan, inf = float("nan"), float("inf")
    ok = [(0, 1, 5, [0.5, 0.25]), (1, 0, 0, [1.0])]
    good = dict(n_in=2, n_out=2, routes=ok, max_samples=1000)
    bad = [dict(n_in=0), dict(n_in=65), dict(n_in=-1), dict(n_in=True), dict(n_in=2.5), dict(n_out=0), dict(n_out=65), dict(n_out=1),
           dict(n_in=1), dict(routes=[]), dict(routes=ok * 257), dict(routes=[(0, 1, 5)]), dict(routes=[(0, 1, 5, [])]),
           dict(routes=[(0, 1, 5, np.ones(33))]), dict(routes=[(0, 1, -1, [1.0])]), dict(routes=[(0, 1, 65537, [1.0])]),
           dict(routes=[(0, 1, 2.5, [1.0])]), dict(routes=[(-1, 1, 5, [1.0])]), dict(routes=[(0, 2, 5, [1.0])]),
           dict(routes=[(0, 1, 5, [1.0, nan])]), dict(routes=[(0, 1, 5, [inf])]), dict(routes=[(0, 1, 5, [-inf])]),
           dict(routes=[(0, 1, 5, [1e39])]), dict(max_samples=0), dict(max_samples=-1), dict(max_samples=True)]
    for kw in bad:
        with pytest.raises(capi.InvalidArgument):
            capi.DelayMatrix(None, **dict(good, **kw))
    for kw in (dict(), dict(routes=ok * 256), dict(routes=[(0, 1, 65536, np.ones(32))]), dict(n_in=64, n_out=64)):
        with pytest.raises(capi.InvalidArgument, match="ctx"):
            capi.DelayMatrix(None, **dict(good, **kw))  # (a good configuration gets as far as the missing context)
    lib = capi.load()
    assert lib.earhip_delaymix_reset(None) == capi.INVALID_ARGUMENT and lib.earhip_delaymix_destroy(None) == capi.OK
    assert lib.earhip_delaymix_info(None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_delaymix_create(None, None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_delaymix_process(None, 0, None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_delaymix_process_device(None, 0, None, 0, None, 0) == capi.INVALID_ARGUMENT
