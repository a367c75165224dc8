"""CPU checks of the polyphase sample-rate converter (include/earhip.h, group P): the host form of the shared maths header
(libear_amd/csrc/src.h: the index arithmetic, the history rule and the fmaf chain the device kernel runs) compiled for the host
under ASan and UBSan against scipy.signal.upfirdn under the derived bound of tests/src_model.py, the output counts and the bits
under every cutting of the stream, the designer against scipy's firwin, every refusal that needs no device, and the new
symbols declared, exported and bound.

Measured by these tests (worst |y - ref| as a share of the bound gamma_T S + T 2^-149, 4 channels x 1,213 samples): 0.999 for
1/1 T=1 (one product: half an ulp against gamma_1 = u / (1 - u), as close as any correct form gets), 0.27 .. 0.38 for T = 8,
0.07 .. 0.17 for T = 24 and 48; the same for every cutting (the bits are)."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.signal import firwin

import src_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1213


@pytest.mark.parametrize("case", sm.CASES, ids=sm.case_id)
def test_host_form_against_upfirdn_counts_and_bits_under_every_cutting(case):
    L, M, T = case
    h = sm.taps_for(L, M, T)
    x = sm.signals(N)
    ref, S = sm.model(x, h, L, M)
    one = None
    for cut, calls in sm.cuttings(N, 1).items():
        y, counts = sm.host_run(x, h, L, M, T, calls)
        fed = np.cumsum(calls)
        assert [int(v) for v in np.cumsum(counts)] == [sm.n_outputs(int(v), L, M) for v in fed], cut  # ceil(N L / M) after every call
        worst = sm.worst_ratio(y, ref, S, T)
        print(f"{sm.case_id(case)}, {cut}: worst error {worst:.3f} of the bound")
        assert worst <= 1.0, cut
        assert np.all(y[3].view(np.uint32) == 0), cut  # silence in, +0.0 out
        one = y if one is None else one
        assert np.array_equal(sm.bits(y), sm.bits(one)), cut
    if case == (1, 1, 1):
        assert np.array_equal(one, np.float32(h[0]) * x)  # a gain of h[0]
    if case == (1, 2, 8):
        assert sm.host_run(x[:, :2], h, L, M, T, [1, 1])[1] == [1, 0]  # the header's example of a call without an output


def test_a_nan_reaches_exactly_the_outputs_whose_window_holds_it():
    for L, M, T in ((3, 2, 8), (147, 160, 48)):
        h = sm.taps_for(L, M, T)
        x = sm.signals(N)[:1]
        clean, _ = sm.host_run(x, h, L, M, T)
        s = 500
        bad = x.copy()
        bad[0, s] = np.nan
        y, _ = sm.host_run(bad, h, L, M, T, [300, 150, 100, N - 550])
        i = (np.arange(y.shape[1]) * M) // L
        hit = (i - T + 1 <= s) & (s <= i)
        assert hit.any() and not np.isfinite(y[0, hit]).any()
        assert np.array_equal(sm.bits(y[0, ~hit]), sm.bits(clean[0, ~hit]))


@pytest.mark.parametrize("L,M,T", [(160, 147, 48), (1, 2, 96), (3, 2, 8)])
def test_designer_is_L_times_firwin(L, M, T):
    from libear_amd import capi
    for beta, cutoff in ((10.0, 1.0), (8.0, 0.9), (5.0, 0.5), (0.0, 0.75)):
        got = capi.src_design(L, M, T, beta, cutoff)
        want = L * firwin(L * T, cutoff / max(L, M), window=("kaiser", beta))
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (beta, cutoff, np.abs(got - want).max())
    # every phase passes DC alike: the sums of the rows of c[p][k] = h[p + k L]
    sums = capi.src_design(L, M, T, 10.0, 1.0).reshape(T, L).sum(axis=0)
    print(f"{L}/{M} T={T}: per-phase sums within {np.abs(sums - 1.0).max():.2e} of 1")
    assert np.abs(sums - 1.0).max() <= 1e-3


def test_designer_refusals():
    from libear_amd import capi
    nan, inf = float("nan"), float("inf")
    for args in ((0, 1, 8), (1, 0, 8), (1025, 1, 8), (1, 1025, 8), (2, 4, 8), (6, 4, 8), (3, 2, 0), (3, 2, 257), (1024, 1, 33),
                 (3, 2, 8, -1.0), (3, 2, 8, nan), (3, 2, 8, inf), (3, 2, 8, 10.0, 0.0), (3, 2, 8, 10.0, 1.5), (3, 2, 8, 10.0, nan),
                 (-3, 2, 8), (3, 2, True), (2.5, 2, 8)):
        with pytest.raises(capi.InvalidArgument):
            capi.src_design(*args)
    assert capi.load().earhip_src_design(3, 2, 8, 10.0, 1.0, None) == capi.INVALID_ARGUMENT
    assert capi.src_design(1, 1, 1).tolist() == [1.0] and capi.src_design(1024, 1, 32).shape == (32768,)


def test_host_program_refuses_what_create_refuses():
    x = np.zeros((2, 8), np.float32)
    for (L, M, T), word in (((2, 4, 8), "common factor"), ((0, 1, 8), "up must"), ((1, 1025, 8), "down must"), ((3, 2, 257), "taps_per_phase"),
                            ((1024, 1, 33), "32768")):
        assert word in sm.host_run(x, np.zeros(max(L * T, 1)), L, M, T, expect=3), (L, M, T)
    for v in (float("nan"), float("inf"), 1e39):
        h = sm.taps_for(3, 2, 8)
        h[5] = v
        assert "finite" in sm.host_run(x, h, 3, 2, 8, expect=3)


NEW_SYMBOLS = ["earhip_src_create", "earhip_src_destroy", "earhip_src_reset", "earhip_src_info", "earhip_src_next_out",
               "earhip_src_process_device", "earhip_src_process", "earhip_src_design"]


def test_new_symbols_are_declared_exported_and_bound():
    from libear_amd import build as build_lib
    path = build_lib()
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\b(earhip_\w+)\b", out))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in exported, s
    assert "typedef struct earhip_src_config" in header and "typedef struct earhip_src_properties" in header
    from libear_amd import capi
    assert hasattr(capi, "SampleRateConverter") and hasattr(capi, "src_design")
    mirror = open(os.path.join(ROOT, "libear_amd", "host", "ear", "hip_src.hpp")).read()
    assert "class SampleRateConverter" in mirror


def test_bindings_refuse_bad_arguments_without_a_device():
    """the configuration is checked before the context is looked at: every refusal of earhip_src_create on any machine"""
    from libear_amd import capi
    nan, inf = float("nan"), float("inf")
    ok = sm.taps_for(3, 2, 8)
    good = dict(channels=2, up=3, down=2, taps_per_phase=8, taps=ok, max_samples=1000)

    def with_tap(v):
        h = ok.copy()
        h[7] = v
        return h

    bad = [dict(channels=0), dict(channels=65), dict(channels=-1), dict(channels=True), dict(channels=2.5),
           dict(up=0, taps=np.zeros(8)), dict(up=1025, taps=np.zeros(8)), dict(down=0), dict(down=1025), dict(up=4, taps=np.zeros(32)),
           dict(up=9, down=6, taps=np.zeros(72)), dict(taps_per_phase=0, taps=np.zeros(1)), dict(taps_per_phase=257, taps=np.zeros(771)),
           dict(up=1024, down=1, taps_per_phase=33, taps=np.zeros(1024 * 33)), dict(taps=ok[:-1]), dict(taps=np.concatenate([ok, [0.0]])),
           dict(taps=with_tap(nan)), dict(taps=with_tap(inf)), dict(taps=with_tap(-inf)), dict(taps=with_tap(1e39)),
           dict(max_samples=0), dict(max_samples=-1), dict(max_samples=True)]
    for kw in bad:
        with pytest.raises(capi.InvalidArgument):
            capi.SampleRateConverter(None, **dict(good, **kw))
    with pytest.raises(capi.InvalidArgument, match="ctx"):
        capi.SampleRateConverter(None, **good)  # (a good configuration gets as far as the missing context)
    lib = capi.load()
    assert lib.earhip_src_reset(None) == capi.INVALID_ARGUMENT and lib.earhip_src_destroy(None) == capi.OK
    assert lib.earhip_src_info(None, None) == capi.INVALID_ARGUMENT and lib.earhip_src_create(None, None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_src_next_out(None, 0, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_src_process(None, 0, None, None, 0, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_src_process_device(None, 0, None, 0, None, 0, 0, None) == capi.INVALID_ARGUMENT
