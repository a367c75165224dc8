"""CPU checks of the FIR filter matrix's filter sets (include/earhip.h, group M, FILTER SETS): the model of the output-side
crossfade (tests/firmix_sets_model.py) against an independent sample-by-sample float64 evaluation, the CPU path that sets the
device tests' bar on the fade blocks, the fade schedule and per-set lists of libear_amd/csrc/firmix.h under ASan + UBSan, the
six new symbols declared and exported, and the Python binding's argument checks.

e_cpu over the fade blocks measured here (worst output channel of each shape): 2.3e-7 .. 3.2e-7, against the bound of 1e-6."""
import os
import re
import subprocess

import numpy as np
import pytest

import firmix_model as fm
import firmix_sets_model as fsm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_against_a_sample_by_sample_evaluation():
    """one_block: every output sample as the formula's double sum, with the fade written out per sample"""
    C, K, J, B, T, _, s, F = fsm.SHAPES["one_block"]
    x, h0, h1, want, _ = fsm.case("one_block")
    xd, hd = x.astype(np.float64), (h0.astype(np.float64), h1.astype(np.float64))

    def y(which, k, n):
        acc = 0.0
        for c in range(C):
            j = np.arange(min(J, n + 1))
            acc += float(np.dot(hd[which][k, c, j], xd[c, n - j]))
        return acc

    worst = 0.0
    for k in range(K):
        for n in range(B * T):
            t = n // B
            if t < s:
                v = y(0, k, n)
            elif t < s + F:
                a = ((t - s) * B + n % B) / (F * B)
                v = (1.0 - a) * y(0, k, n) + a * y(1, k, n)
            else:
                v = y(1, k, n)
            worst = max(worst, abs(v - want[k, n]))
    scale = np.abs(want).max()
    print(f"one_block: model against the sample-by-sample sum, worst difference {worst:.3e} (largest sample {scale:.3e})")
    assert worst <= 1e-12 * max(scale, 1.0)
    assert np.array_equal(want[:, s * B], fm.truth(x, h0)[:, s * B]), "the ramp starts at 0: the set faded from alone"


@pytest.mark.parametrize("name", list(fsm.SHAPES))
def test_cpu_path_within_1e_6_of_truth_on_the_fade_blocks(name):
    C, K, J, B, T, calls, s, F = fsm.SHAPES[name]
    x, h0, h1, want, e_cpu = fsm.case(name)
    assert x.shape == (C, B * T) and h0.shape == h1.shape == (K, C, J) and sum(calls) == T and 0 < s and s + F < T
    assert sum(fsm.cut_calls(calls, s)) == T
    print(f"{name} {fsm.SHAPES[name]}: e_cpu on the fade blocks {e_cpu.min():.3e} .. {e_cpu.max():.3e}")
    assert np.all(e_cpu > 0) and np.all(e_cpu <= fm.E_CPU_MAX)


def test_cut_calls_and_the_lists_that_differ():
    assert fsm.cut_calls((5,), 2) == (2, 3)
    assert fsm.cut_calls((1, 2, 4), 1) == (1, 2, 4) and fsm.cut_calls((2, 2, 4), 5) == (2, 2, 1, 3)
    _, h0, h1, _, _ = fsm.case("lists_differ")
    nz0, nz1 = np.any(h0 != 0, axis=2), np.any(h1 != 0, axis=2)
    assert np.array_equal(nz0, np.eye(4, dtype=bool))
    assert nz1.sum() == 3 and not nz1[3].any() and all(nz1[k, 3 - k] for k in range(3))


def test_fade_schedule_and_set_lists_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/cpp/firmix_sets_host.cpp: per-set lists (dense, diagonal, device taps), the merged walk, which blocks of a feed are
    fade blocks and q of each, the ramp, every refusal of select"""
    exe = tmp_path / "firmix_sets_host"
    src = os.path.join(ROOT, "tests", "cpp", "firmix_sets_host.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-static-libasan", src, "-o", str(exe)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    m = re.search(r"^(\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert m and int(m.group(1)) > 500, res.stdout


NEW_SYMBOLS = ["earhip_firmix_create_sets", "earhip_firmix_load_set", "earhip_firmix_load_set_device", "earhip_firmix_select",
               "earhip_firmix_state", "earhip_firmix_set_info"]


def test_new_symbols_are_declared_and_exported():
    from libear_amd import build as build_lib
    path = build_lib()
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\b(earhip_\w+)\b", out))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in exported, s


class _Shape:
    """a FirMatrix's fields without a device object: the binding's own checks come before any call into the library"""
    K, C, J, B, h = 2, 3, 8, 64, None


def test_python_binding_argument_checks():
    from libear_amd import capi
    with pytest.raises(capi.InvalidArgument):
        capi.FirMatrix(None, np.ones((2, 3), np.float32), 64, n_sets=2)
    for bad in (2.5, "2", True):
        with pytest.raises(capi.InvalidArgument):
            capi.FirMatrix(None, np.ones((2, 3, 8), np.float32), 64, n_sets=bad)
    for taps in (np.ones((2, 3, 7), np.float32), np.ones((3, 2, 8), np.float32), np.ones((2, 3), np.float32)):
        with pytest.raises(capi.InvalidArgument):
            capi.FirMatrix.load_set(_Shape(), 1, taps)
    for ptr in (0, None):
        with pytest.raises(capi.InvalidArgument):
            capi.FirMatrix.load_set_device(_Shape(), 1, ptr)
