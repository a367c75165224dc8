"""A float64 model of the look-ahead limiter (include/earhip.h, group N), written from the header's text and not from the product
code.  numpy only.  The interpolator is true_peak_model.interpolate on the float32 samples.

    e[n] = max over c of max(|x_c[n - D]|, max over p of |y_c[phases n + p]|)      (detect = 0: D = 0, e[n] = max |x_c[n]|)
    r[n] = min(1, c / e[n]), 1 where e = 0;  m[n] = min of r[n - M + 1 .. n], M = L + 2 + H, r = 1 before the stream
    s[n] = m[n] + .. + m[n - L];  g[n] = min(s[n] / K, r[n - L]), K = L + 1;  out_c[n] = x_c[n - D - L] g[n]

THE GUARANTEE (header): for finite input |out_c[n]| <= c (1 + 2^-22) in the float32 path.  Proof: the window of m[n - k],
k <= L, is r[n - k - M + 1 .. n - k]; M - 1 >= L + 1 > L - k, so r[n - L] lies in every one of them and the final min makes
g[n] <= r[n - L] hold exactly, whatever the K adds rounded to.  r[n - L] <= fl(c / e[n - L]) <= (c / e[n - L]) (1 + 2^-24), and
|x_c[n - D - L]| <= e[n - L] because the detector at n - L takes |x_c[(n - L) - D]| exactly (max is exact).  So the exact product
|x| g <= c (1 + 2^-24), and rounding it once gives at most c (1 + 2^-24)^2 < c (1 + 2^-22).  In this float64 model the same
chain holds with 2^-53 in the place of 2^-24.

THE BOUND the float32 path is held to against this model (bound() below), for finite samples:
    |g - g_model| <= ((taps + 1) A X / c + K + 4) 2^-24,        |out - out_model| <= |x_c[n - D - L]| times that
A and taps as in true_peak_model.bound (the first term is 0 with detect = 0), X the largest sample peak of any channel.
Derivation, in units of 2^-24:
  - the float32 interpolator is within (taps + 1) A X of the model's y (true_peak_model), |x| and max are exact, so e is too;
  - r differs only where one of the two is below 1, i.e. e >= c (up to the error itself): there |d(c / e) / de| = c / e^2 <= 1 / c,
    so the detector contributes (taps + 1) A X / c, and the correctly rounded division of a quotient <= 1 at most 1 (min with 1 is
    1-Lipschitz);
  - min is 1-Lipschitz: m inherits the error of r, and so does their mean s / K;
  - the K - 1 rounded adds (0 + m is exact) each err by at most 1 of their partial sum <= K: (K - 1) K in all, K - 1 after the
    division by K, which itself adds 1 of a quotient <= 1;
  - the outer min is 1-Lipschitz; the multiplication adds 1 of |x| g <= |x|.
That is (taps + 1) A X / c + 1 + (K - 1) + 1 + 1 = (taps + 1) A X / c + K + 2 for out and K + 1 for g; the form above leaves
two units for the second-order terms (errors of errors, e slightly below c) and the model's own float64 rounding."""
import os
import struct
import subprocess
import tempfile

import numpy as np

import true_peak_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shape(L, H, detect, table=None):
    """(D, M, K, taps, phases)"""
    if not detect:
        return 0, L + 2 + H, L + 1, 0, 0
    h = tm.default_table() if table is None else np.asarray(table, np.float64)
    return h.shape[1] // 2, L + 2 + H, L + 1, h.shape[1], h.shape[0]


def _delayed(x, d):
    """x [C][n] -> x[:, n - d], zero before the stream"""
    return np.concatenate([np.zeros((x.shape[0], d)), x], axis=1)[:, :x.shape[1]]


def detector(x, detect, table=None):
    """e [n] float64 on the float32 samples x [C][n]; NaN ignored"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    D = shape(8, 0, detect, table)[0]
    xd = _delayed(x.astype(np.float64), D)
    e = np.where(np.isnan(xd), 0.0, np.abs(xd)).max(axis=0)
    if detect:
        for c in range(x.shape[0]):
            y = np.abs(tm.interpolate(x[c], table))
            e = np.maximum(e, np.where(np.isnan(y), 0.0, y).max(axis=1))
    return e


def sliding_min(r, M):
    """min of r[n - M + 1 .. n], r = 1 before the stream: by the definition on a strided view where that is small, else in
    pieces"""
    a = np.concatenate([np.ones(M - 1), r])
    out = np.empty(r.size)
    step = max(1, (1 << 24) // M)
    for lo in range(0, r.size, step):
        hi = min(r.size, lo + step)
        out[lo:hi] = np.lib.stride_tricks.sliding_window_view(a[lo:hi + M - 1], M).min(axis=1)
    return out


def limit(x, c, L, H, detect=True, table=None):
    """x [C][n] -> dict: out [C][n] float64, g [n], r [n], e [n], latency, min_gain, limited"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    c = float(np.float32(c))
    D, M, K, _, _ = shape(L, H, detect, table)
    n = x.shape[1]
    e = detector(x, detect, table)
    with np.errstate(divide="ignore"):
        r = np.where(e > 0, np.minimum(1.0, c / np.where(e > 0, e, 1.0)), 1.0)
    m = np.concatenate([np.ones(L), sliding_min(r, M)])  # m[L + n] is m of sample n
    s = np.zeros(n)
    for k in range(K):
        s = s + m[L - k:L - k + n]
    g = np.minimum(s / K, np.concatenate([np.ones(L), r])[:n])
    with np.errstate(invalid="ignore"):
        out = _delayed(x.astype(np.float64), D + L) * g
    return {"out": out, "g": g, "r": r, "e": e, "latency": D + L, "min_gain": float(g.min()) if n else 1.0,
            "limited": int((g < 1.0).sum())}


def gain_bound(x, c, L, H, detect=True, table=None):
    """the bound on |g - g_model| (a number)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    c = float(np.float32(c))
    _, _, K, taps, _ = shape(L, H, detect, table)
    fin = np.abs(x[np.isfinite(x)]).astype(np.float64)
    X = float(fin.max()) if fin.size else 0.0
    A = tm.table_gain(tm.default_table() if table is None else table) if detect else 0.0
    return ((taps + 1) * A * X / c + K + 4) * 2.0 ** -24


def bound(x, c, L, H, detect=True, table=None):
    """the bound on |out - out_model| [C][n]"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    D = shape(L, H, detect, table)[0]
    return np.abs(_delayed(x.astype(np.float64), D + L)) * gain_bound(x, c, L, H, detect, table)


def worst_ratios(out, g, want, x, c, L, H, detect=True, table=None):
    """(the largest |out - model| / bound, the same for g); finite inputs"""
    b = bound(x, c, L, H, detect, table)
    err = np.abs(np.asarray(out, np.float64) - want["out"])
    assert np.all(err[b == 0] == 0)
    ro = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    rg = float(np.abs(np.asarray(g, np.float64) - want["g"]).max() / gain_bound(x, c, L, H, detect, table)) if want["g"].size else 0.0
    return ro, rg


def guarantee(c):
    """the most |out| may be"""
    return float(np.float32(c)) * (1.0 + 2.0 ** -22)


def true_peak_of(out, table=None):
    """the model's true peak of rows [C][n] (rounded to float32 first: what a file would hold)"""
    out = np.atleast_2d(np.asarray(out, np.float32))
    return max(float(np.abs(tm.interpolate(row, table)).max()) for row in out)


# ---- libear_amd/csrc/limiter.h compiled for the host ----------------------------------------------------------------------------
_exe = {}


def host_exe(sanitize=True):
    """tests/cpp/limiter_host.cpp built once per session: under ASan and UBSan (the CPU suite), or plainly (the GPU suite, which
    only wants the header's bits)"""
    if sanitize not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="limiter_host_"), "limiter_host")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"] if sanitize else ["-O2"]
        res = subprocess.run(["g++", "-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                             [os.path.join(ROOT, "tests", "cpp", "limiter_host.cpp"), "-o", exe],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode == 0, res.stdout
        _exe[sanitize] = exe
    return _exe[sanitize]


def host_run(x, c, L, H, detect=True, calls=None, table=None, sanitize=True):
    """x [C][n] through LimiterRef in calls of the given lengths -> dict: out [C][n], g [n] float32, min_gain float32, limited"""
    x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
    C, n = x.shape
    calls = np.asarray([n] if calls is None else calls, np.uint64)
    assert int(calls.sum()) == n
    t = np.zeros((0, 0)) if table is None else np.ascontiguousarray(table, np.float64)
    exe = host_exe(sanitize)
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<7ifQ", C, L, H, int(bool(detect)), t.shape[0], t.shape[1], calls.size, float(np.float32(c)), n))
        f.write(t.tobytes() + calls.tobytes() + x.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout
    raw = open(fout, "rb").read()
    assert len(raw) == 4 * C * n + 4 * n + 16
    out = np.frombuffer(raw, np.float32, C * n).reshape(C, n)
    g = np.frombuffer(raw, np.float32, n, 4 * C * n)
    mg = np.frombuffer(raw, np.float32, 1, 4 * (C + 1) * n)[0]
    lim = int(np.frombuffer(raw, np.uint64, 1, 4 * (C + 1) * n + 8)[0])
    return {"out": out, "g": g, "min_gain": mg, "limited": lim}
