"""A float64 model of the delay matrix (include/earhip.h, group S), written from the header's text and not from the product
code: per output row the sum over its routes of the float32 taps times the delayed float32 samples, products and sums in float64.

THE BOUND every form of the stage is held to against this model (derived, not measured; the bound of tests/src_model.py).
Output n of row k is ONE chain of K fused multiply-adds in float32 over all the routes into k, K = the sum of their T_r: each
step rounds once, relative error at most u = 2^-24 for a normal result and absolute error at most 2^-150 for a subnormal one,
so by the usual induction
    |y - ref| <= gamma_K * S + K * 2^-149,     gamma_K = K u / (1 - K u),     S = sum |h| |x| over the same products
with ref the exact sum (float64 products of float32 numbers are exact, and the float64 sum's own error, K 2^-53 S, is 2^-29 of
the first term)."""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def taps_for(T, seed):
    """T float32 taps for the tests (noise: nothing here depends on what they filter)"""
    return np.random.default_rng(1000 + seed).uniform(-1.0, 1.0, T).astype(np.float32)


def routes32(routes):
    """(in, out, delay, taps) with the taps as float32 arrays"""
    return [(int(i), int(o), int(d), np.asarray(h, np.float32).reshape(-1)) for i, o, d, h in routes]


# name -> (n_in, n_out, routes): the cases of the CPU and the GPU tests
CASES = {
    # every misalignment of an input window against the 16-byte output vectors
    "delays 0 1 2 3 5": (5, 5, [(c, c, d, [1.0 - 0.125 * c]) for c, d in enumerate((0, 1, 2, 3, 5))]),
    "T = 1, 2, 16, 32": (4, 4, [(c, c, d, taps_for(T, T)) for c, (T, d) in enumerate(((1, 4), (2, 0), (16, 13), (32, 85)))]),
    # two routes into output 0, none into output 1; input 1 is read by nothing
    "3 into 2, an idle output and an unread input": (3, 2, [(0, 0, 7, taps_for(16, 1)), (2, 0, 2, taps_for(2, 2))]),
    # crossed routes, an input read at two delays into one output, a long delay
    "a full matrix": (3, 3, [(0, 1, 0, [0.5]), (1, 0, 3, taps_for(4, 3)), (2, 2, 130, [-1.0]), (0, 2, 1, taps_for(6, 4)),
                             (0, 1, 41, taps_for(2, 5)), (1, 1, 9, [0.25])]),
}


def unread(n_in, routes):
    return sorted(set(range(n_in)) - {r[0] for r in routes})


def history(routes):
    return max(d + len(h) - 1 for _, _, d, h in routes32(routes))


def noise(C, n, seed=3):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (C, n)).astype(np.float32)


def model(x, n_out, routes):
    """x [n_in][n] float32 -> (ref [n_out][n] float64, S [n_out][n] float64, K [n_out] products per output)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    n = x.shape[1]
    ref, S, K = np.zeros((n_out, n)), np.zeros((n_out, n)), np.zeros(n_out, np.int64)
    for i, o, d, h in routes32(routes):
        row = x[i].astype(np.float64)
        for j, tap in enumerate(h.astype(np.float64)):
            s = d + j
            if s < n:
                ref[o, s:] += tap * row[:n - s]
                S[o, s:] += abs(tap) * np.abs(row[:n - s])
        K[o] += h.size
    return ref, S, K


def bound(S, K):
    u = 2.0 ** -24
    K = np.asarray(K, np.float64)[:, None]
    return K * u / (1.0 - K * u) * S + K * 2.0 ** -149


def worst_ratio(y, ref, S, K):
    """the largest |y - ref| / bound over the outputs that have a route (the others must be +0.0 exactly)"""
    y = np.atleast_2d(np.asarray(y, np.float64))
    assert y.shape == ref.shape, (y.shape, ref.shape)
    fed = np.asarray(K) > 0
    assert not np.ascontiguousarray(y[~fed], np.float32).view(np.uint32).any(), "an output without a route is not +0.0"
    if not fed.any() or ref.shape[1] == 0:
        return 0.0
    return float((np.abs(y - ref)[fed] / bound(S, K)[fed]).max())


def cuttings(n, H, tile=None):
    """name -> call lengths that sum to n: the cuttings every form is run under (H: the history; tile: the kernel's, for the device)"""
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107]
    out = {"one call": [n]}
    calls, k = [], 0
    while sum(calls) + primes[k % len(primes)] <= n:
        calls.append(primes[k % len(primes)])
        k += 1
    out["prime-length calls"] = calls + ([n - sum(calls)] if sum(calls) < n else [])
    out["an empty call in the middle"] = [n // 3, 0, n - n // 3]
    short = max(1, min(H - 1, 7)) if H > 1 else 1
    m = min(n // short, 40)
    out["calls shorter than H"] = [short] * m + [n - short * m]
    if tile is None:
        out["one-sample calls"] = [1] * n
    else:
        out["one-sample calls, then the rest"] = [1] * 9 + [n - 9]
        if n > 2 * tile + 2:
            b = [tile - 1, 1, tile + 1]
            out["around the tile"] = b + [n - sum(b)]
    for calls in out.values():
        assert sum(calls) == n
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- libear_amd/csrc/delaymix.h compiled for the host --------------------------------------------------------------------------------
_exe = {}


def host_exe(sanitize=True):
    """tests/cpp/delaymix_host.cpp built once per session: under ASan and UBSan (the CPU suite), or plainly"""
    if sanitize not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="delaymix_host_"), "delaymix_host")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"] if sanitize else ["-O2"]
        res = subprocess.run(["g++", "-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                             [os.path.join(ROOT, "tests", "cpp", "delaymix_host.cpp"), "-o", exe],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode == 0, res.stdout
        _exe[sanitize] = exe
    return _exe[sanitize]


def host_run(x, n_out, routes, calls=None, sanitize=True, expect=0, raw_routes=None):
    """x [n_in][n] through DelaymixRef in calls of the given lengths -> y [n_out][n] float32; expect = 3: the refusal's text.
    raw_routes: (in, out, delay, n_taps, taps) records written as they are (for the refusals)"""
    x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
    n_in, n = x.shape
    calls = np.asarray([n] if calls is None else calls, np.uint64)
    assert int(calls.sum()) == n
    exe = host_exe(sanitize)
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    if raw_routes is None:
        raw_routes = [(i, o, dl, h.size, h) for i, o, dl, h in routes32(routes)]
    with open(fin, "wb") as f:
        f.write(struct.pack("<4iQ", n_in, n_out, len(raw_routes), calls.size, n))
        for i, o, dl, T, h in raw_routes:
            taps = np.zeros(32, np.float32)
            taps[:min(len(h), 32)] = np.asarray(h, np.float32)[:32]
            f.write(struct.pack("<4i", i, o, dl, T) + taps.tobytes())
        f.write(calls.tobytes() + x.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == expect, res.stdout
    if expect:
        return res.stdout
    y = np.fromfile(fout, np.float32)
    assert y.size == n_out * n
    return y.reshape(n_out, n)
