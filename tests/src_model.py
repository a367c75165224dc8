"""A float64 model of the polyphase sample-rate converter (include/earhip.h, group P), written from the header's text and not
from the product code: scipy.signal.upfirdn over the float32-rounded taps, cut to the ceil(N L / M) outputs the header counts.

THE BOUND every form of the stage is held to against this model (derived, not measured).  Output j is a chain of T fused
multiply-adds in float32, acc = fmaf(c_k, x_k, acc): each step rounds once, relative error at most u = 2^-24 for a normal result
and absolute error at most 2^-150 for a subnormal one, so by the usual induction
    |y - ref| <= gamma_T * S + T * 2^-149,     gamma_T = T u / (1 - T u),     S = sum_k |c_k| |x_k| = upfirdn(|c|, |x|, L, M)
with ref the exact sum (float64 products of float32 numbers are exact, and the float64 sum's own error, T 2^-53 S, is 2^-29 of
the first term).  On uniform noise a bit-level model of the float32 chain sits at 0.10 .. 0.34 of the bound for the nine ratio
cases."""
import os
import struct
import subprocess
import tempfile

import numpy as np
from scipy.signal import upfirdn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (L, M, T): the ratio cases
CASES = [(1, 1, 1), (2, 1, 8), (1, 2, 8), (3, 2, 8), (2, 3, 8), (160, 147, 48), (147, 160, 48), (147, 320, 48), (320, 147, 24)]


def case_id(case):
    return "%d/%d T=%d" % case


def n_outputs(n, L, M):
    """ceil(n L / M): the outputs produced after n inputs in total"""
    return -((-n * L) // M)


def taps_for(L, M, T, seed=0):
    """a prototype for the tests: a windowed sinc by numpy (not by the designer under test); for 1/1 T=1 a plain gain"""
    if L * T == 1:
        return np.array([0.75])
    n = L * T
    m = np.arange(n) - (n - 1) / 2.0
    fc = 0.9 / max(L, M)
    h = fc * np.sinc(fc * m) * np.kaiser(n, 8.0)
    return L * h / h.sum()


def taps32(h):
    return np.asarray(h, np.float64).astype(np.float32).astype(np.float64)


def signals(n, seed=11):
    """4 channels: noise, a step, an impulse, silence"""
    x = np.zeros((4, n), np.float32)
    x[0] = np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)
    x[1, min(100, n // 2):] = 0.5
    x[2, min(37, n - 1)] = 1.0
    return x


def noise(C, n, seed=3):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (C, n)).astype(np.float32)


def model(x, h, L, M):
    """x [C][n] float32 -> (ref [C][n_out] float64, S [C][n_out] float64)"""
    x = np.atleast_2d(np.asarray(x, np.float32)).astype(np.float64)
    c = taps32(h)
    n_out = n_outputs(x.shape[1], L, M)
    ref = np.stack([upfirdn(c, row, L, M)[:n_out] for row in x])
    S = np.stack([upfirdn(np.abs(c), np.abs(row), L, M)[:n_out] for row in x])
    assert ref.shape == (x.shape[0], n_out)
    return ref, S


def bound(S, T):
    u = 2.0 ** -24
    return T * u / (1.0 - T * u) * S + T * 2.0 ** -149


def worst_ratio(y, ref, S, T):
    """the largest |y - ref| / bound (the bound is positive everywhere)"""
    y = np.atleast_2d(np.asarray(y, np.float64))
    assert y.shape == ref.shape, (y.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    return float((np.abs(y - ref) / bound(S, T)).max())


def cuttings(n, tile):
    """name -> call lengths that sum to n (tile: the kernel's tile length in inputs; 1 for the host form, which has none)"""
    assert n > 2 * tile + 9
    a = [1, 1, 1, 0, 5]
    b = [max(tile - 1, 0), 1, tile + 1]
    h = n // 2
    h += 1 - h % 2  # an odd sample
    return {"one call": [n], "short calls, an empty one": a + [n - sum(a)], "around the tile": b + [n - sum(b)],
            "two halves at an odd sample": [h, n - h]}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- libear_amd/csrc/src.h compiled for the host ------------------------------------------------------------------------------------
_exe = {}


def host_exe(sanitize=True):
    """tests/cpp/src_host.cpp built once per session: under ASan and UBSan (the CPU suite), or plainly"""
    if sanitize not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="src_host_"), "src_host")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"] if sanitize else ["-O2"]
        res = subprocess.run(["g++", "-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                             [os.path.join(ROOT, "tests", "cpp", "src_host.cpp"), "-o", exe],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode == 0, res.stdout
        _exe[sanitize] = exe
    return _exe[sanitize]


def host_run(x, h, L, M, T, calls=None, sanitize=True, expect=0):
    """x [C][n] through SrcRef in calls of the given lengths -> (y [C][total] float32, the outputs of every call); expect = 3:
    the refusal's text"""
    x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
    C, n = x.shape
    calls = np.asarray([n] if calls is None else calls, np.uint64)
    assert int(calls.sum()) == n
    exe = host_exe(sanitize)
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<6iQ", C, L, M, T, calls.size, 0, n))
        f.write(np.ascontiguousarray(h, np.float64).tobytes() + calls.tobytes() + x.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == expect, res.stdout
    if expect:
        return res.stdout
    raw = open(fout, "rb").read()
    total = struct.unpack_from("<Q", raw)[0]
    counts = np.frombuffer(raw, np.uint64, calls.size, 8)
    y = np.frombuffer(raw, np.float32, C * total, 8 + 8 * calls.size).reshape(C, total)
    assert len(raw) == 8 + 8 * calls.size + 4 * C * total
    return y, [int(v) for v in counts]
