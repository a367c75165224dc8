"""CPU checks of the FIR filter matrix (include/earhip.h, group M): the float64 model (tests/firmix_model.py) against
scipy.signal.fftconvolve, the CPU path that sets the device tests' bar (one libear BlockConvolver per non-zero pair, summed in
float32) against the model on the device tests' shapes, the plan header the kernels share with the host
(libear_amd/csrc/firmix.h) under ASan + UBSan, and the new symbols declared and exported.

e_cpu measured here (worst output channel of each shape): 1.5e-7 .. 3.5e-7, against the bound of 1e-6."""
import os
import re
import subprocess

import numpy as np
import pytest

import firmix_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_against_scipy_fftconvolve():
    from scipy.signal import fftconvolve
    for C, K, J, n, seed in ((3, 2, 129, 448, 1), (5, 3, 700, 1280, 2), (1, 1, 1, 192, 3), (2, 2, 4097, 12288, 4)):
        x, h = fm.make_case(C, K, J, n, seed)
        if K * C > 1:
            h[K - 1, C - 1] = 0.0  # (a zero pair is skipped by the model and adds nothing here)
        want = np.zeros((K, n))
        for k in range(K):
            for c in range(C):
                want[k] += fftconvolve(x[c].astype(np.float64), h[k, c].astype(np.float64))[:n]
        got = fm.truth(x, h)
        worst = np.max(np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1))
        print(f"({C}, {K}, {J}, {n}): model against fftconvolve {worst:.3e}")
        assert worst <= 1e-12


@pytest.mark.parametrize("name", list(fm.SHAPES))
def test_cpu_path_within_1e_6_of_truth(name):
    x, h, want, e_cpu = fm.case(name)
    C, K, J, B, T, calls = fm.SHAPES[name]
    assert x.shape == (C, B * T) and h.shape == (K, C, J) and sum(calls) == T
    print(f"{name} {fm.SHAPES[name]}: e_cpu {e_cpu.min():.3e} .. {e_cpu.max():.3e}")
    assert np.all(e_cpu > 0) and np.all(e_cpu <= fm.E_CPU_MAX)


def test_rel_err_and_the_bar_catch_a_wrong_result():
    x, h, want, e_cpu = fm.case("last_partition_one_tap")
    assert np.all(fm.rel_err(want, want) == 0)
    assert np.all(fm.rel_err(np.zeros((2, 4)), np.zeros((2, 4))) == 0)
    bad = want.astype(np.float32)
    bad[1, 100] += 1e-3
    with pytest.raises(AssertionError):
        fm.check_against_bar(bad, want, e_cpu, "a wrong sample")


def test_plan_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/cpp/firmix_host.cpp: partition counts (n_taps = B, B + 1, 64 B), pair lists of dense, diagonal and all-zero matrices,
    ring slots over calls shorter than P - 1 blocks, every refused configuration"""
    exe = tmp_path / "firmix_host"
    src = os.path.join(ROOT, "tests", "cpp", "firmix_host.cpp")
    res = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-static-libasan", src, "-o", str(exe)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    m = re.search(r"^(\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert m and int(m.group(1)) > 1000, res.stdout


NEW_SYMBOLS = ["earhip_firmix_create", "earhip_firmix_destroy", "earhip_firmix_reset", "earhip_firmix_info",
               "earhip_firmix_process_device", "earhip_firmix_process", "earhip_render_attach_firmix",
               "earhip_render_firmix_position"]


def test_new_symbols_are_declared_and_exported():
    from libear_amd import build as build_lib
    path = build_lib()
    header = open(os.path.join(ROOT, "include", "earhip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r"\b(earhip_\w+)\b", out))
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in exported, s


def test_python_binding_refuses_taps_that_are_not_a_3d_array():
    from libear_amd import capi
    with pytest.raises(capi.InvalidArgument):
        capi.FirMatrix(None, np.ones((2, 3), np.float32), 64)
