"""A float64 model of the true-peak meter and of the loudness range (include/earhip.h, group L: ITU-R BS.1770-4 annex 2,
EBU Tech 3342), written from the header's text and not from the product code.  numpy only (scipy may be missing where the GPU
suite runs).

The interpolator: y[phases n + p] = sum over k of h[p][k] x[n - k] on the float32 samples, x zero before the stream; true peak
= the largest |y|, sample peak = the largest |x|, NaN ignored; y[phases n + p] belongs to the 100 ms step of sample n.
The bound the device is held to: |tp - tp_model| <= (taps + 1) 2^-24 A X_c, A the largest sum over k of |h[p][k]| of any phase,
X_c the channel's sample peak (float32 rounding of a chain of `taps` fused multiply-adds whose partial sums stay below A X_c)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
H1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]


def default_table():
    """[4][12] float64: BS.1770-4 annex 2"""
    return np.array([H0, H1, H1[::-1], H0[::-1]], np.float64) / 8192.0


def table_gain(table):
    """A of the bound"""
    return float(np.abs(np.asarray(table, np.float64)).sum(axis=1).max())


def interpolate(row, table=None):
    """one channel, float32 samples -> y [n][phases] float64 (zero history)"""
    h = default_table() if table is None else np.asarray(table, np.float64)
    h = h.astype(np.float32).astype(np.float64)  # (rounded once to float32, as the header says)
    taps = h.shape[1]
    x = np.concatenate([np.zeros(taps - 1), np.asarray(row, np.float32).astype(np.float64)])
    win = np.lib.stride_tricks.sliding_window_view(x, taps)[:, ::-1]  # win[n][k] = x[n - k]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.einsum("nk,pk->np", win, h)


def _nanmax0(a, axis):
    """the largest of 0 and the non-NaN entries"""
    a = np.where(np.isnan(a), 0.0, np.abs(a))
    return a.max(axis=axis) if a.shape[axis] else np.zeros(np.delete(a.shape, axis))


def peaks(x, table=None, rate=48000):
    """x [C][n] -> dict: step_tp, step_sp [steps][C] of the whole steps; open_tp, open_sp [C] of the rest; tp, sp [C] of all"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    step = rate // 10
    nsteps = x.shape[1] // step
    out = {k: [] for k in ("step_tp", "step_sp", "open_tp", "open_sp", "tp", "sp")}
    for c in range(x.shape[0]):
        ytp = _nanmax0(interpolate(x[c], table), 1)
        xsp = _nanmax0(x[c].astype(np.float64)[:, None], 1)
        for name, v in (("tp", ytp), ("sp", xsp)):
            out["step_" + name].append(_nanmax0(v[:nsteps * step].reshape(nsteps, step), 1))
            out["open_" + name].append(_nanmax0(v[nsteps * step:], 0))
            out[name].append(_nanmax0(v, 0))
    res = {k: np.array(v, np.float64) for k, v in out.items()}
    res["step_tp"], res["step_sp"] = res["step_tp"].T.reshape(nsteps, x.shape[0]), res["step_sp"].T.reshape(nsteps, x.shape[0])
    return res


def bound(table, sample_peak):
    h = default_table() if table is None else np.asarray(table, np.float64)
    return (h.shape[1] + 1) * 2.0 ** -24 * table_gain(h) * np.asarray(sample_peak, np.float64)


def worst_ratio(got, want, table, sample_peak):
    """the largest |got - want| / bound over everything ([..][C] against the channels' sample peaks [C]); infinities must match
    exactly and count as 0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    b = np.broadcast_to(bound(table, sample_peak), got.shape)
    inf = np.isinf(want) | np.isinf(got)
    assert np.array_equal(got[inf], want[inf])
    err = np.abs(np.where(inf, 0.0, got) - np.where(inf, 0.0, want))
    fin = np.isfinite(b) & ~inf
    ok = (b[fin] > 0) | (err[fin] == 0)
    assert ok.all()
    r = err[fin] / np.where(b[fin] > 0, b[fin], 1.0)
    return float(r.max()) if r.size else 0.0


def dbtp(v):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.asarray(v, np.float64))


# ---- loudness range (EBU Tech 3342) ---------------------------------------------------------------------------------------------
def _lk(p):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(p)


def range_details(z, weights):
    """(P_j, l_j of the 3 s windows, the relative gate or None)"""
    z = np.asarray(z, np.float64)
    n = z.shape[0] - 29
    if n <= 0:
        return np.empty(0), np.empty(0), None
    P = np.stack([z[j:j + 30].mean(axis=0) for j in range(n)]) @ np.asarray(weights, np.float64)
    l = _lk(P)
    ja = l > -70.0
    return P, l, (_lk(P[ja].mean()) - 20.0 if ja.any() else None)


def loudness_range(z, weights):
    """(LRA, low, high); (0, -inf, -inf) with no surviving window"""
    P, l, gamma = range_details(z, weights)
    if gamma is None:
        return 0.0, -np.inf, -np.inf
    s = np.sort(l[(l > -70.0) & (l > gamma)])
    if s.size == 0:
        return 0.0, -np.inf, -np.inf
    low = s[int(np.floor((s.size - 1) * 0.10 + 0.5))]
    high = s[int(np.floor((s.size - 1) * 0.95 + 0.5))]
    return float(high - low), float(low), float(high)


def range_margin(z, weights):
    """the smallest distance in LU of any window of the model from either gate (inf when there is none)"""
    _, l, gamma = range_details(z, weights)
    fin = l[np.isfinite(l)]
    d = [np.abs(fin + 70.0).min()] if fin.size else []
    if gamma is not None and fin.size:
        d.append(np.abs(fin - gamma).min())
    return min(d) if d else np.inf


# ---- libear_amd/csrc/true_peak.h compiled for the host ---------------------------------------------------------------------------
_host = None


def host_lib():
    global _host
    if _host is not None:
        return _host
    out = os.path.join(tempfile.mkdtemp(prefix="true_peak_host_"), "libtrue_peak_host.so")
    cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
           os.path.join(ROOT, "tests", "cpp", "true_peak_host.cpp"), "-o", out]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    lib = C.CDLL(out)
    lib.tp_run.restype = C.c_size_t
    lib.tp_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                           C.c_size_t, C.c_void_p]
    lib.tp_default_table.argtypes = [C.c_void_p]
    _host = lib
    return lib


def host_run(row, calls, table=None, rate=48000):
    """one channel through TruePeakChannelRef in calls of the given lengths -> (step_tp, step_sp, open [tp, sp]) float32"""
    lib = host_lib()
    row = np.ascontiguousarray(row, np.float32)
    calls = np.asarray(calls, np.uint64)
    assert int(calls.sum()) == row.size
    cap = row.size // (rate // 10) + 1
    tp, sp, op = np.zeros(cap, np.float32), np.zeros(cap, np.float32), np.zeros(2, np.float32)
    t = None if table is None else np.ascontiguousarray(table, np.float64)
    n = lib.tp_run(0 if t is None else t.shape[0], 0 if t is None else t.shape[1], None if t is None else t.ctypes.data, rate // 10,
                   row.ctypes.data, calls.ctypes.data, calls.size, tp.ctypes.data, sp.ctypes.data, cap, op.ctypes.data)
    assert n == row.size // (rate // 10)
    return tp[:n], sp[:n], op
