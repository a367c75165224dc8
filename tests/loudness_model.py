"""A float64 model of the programme loudness meter (include/earhip.h, group L: ITU-R BS.1770-4), written from the header's
definition and not from the product code: the K-weighting cascade with scipy.signal.lfilter, the 100 ms step energies, the
gating, and the channel-weight rule.

scipy may be missing where the GPU suite runs.  The cascade then comes from libear_amd/csrc/loudness.h compiled for the host
with g++ (tests/cpp/loudness_host.cpp), which tests/test_loudness_cpu.py pins to scipy.  The model never skips."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# [stage][b0 b1 b2 a1 a2], BS.1770-4 at 48 kHz
COEFFS = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                   [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])

try:
    from scipy.signal import lfilter as _lfilter
except Exception:  # pragma: no cover (a machine without scipy)
    _lfilter = None

_host = None


def host_lib():
    """loudness.h compiled for the host (g++ -O2 -ffp-contract=off, no device code), loaded with ctypes"""
    global _host
    if _host is not None:
        return _host
    out = os.path.join(tempfile.mkdtemp(prefix="loudness_host_"), "libloudness_host.so")
    cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
           os.path.join(ROOT, "tests", "cpp", "loudness_host.cpp"), "-o", out]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    lib = C.CDLL(out)
    lib.loud_run.restype = C.c_size_t
    lib.loud_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.loud_filter.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    _host = lib
    return lib


def host_filter(row):
    row = np.ascontiguousarray(row, np.float32)
    y = np.empty(row.size, np.float64)
    host_lib().loud_filter(row.ctypes.data, row.size, y.ctypes.data)
    return y


def k_weight(row, use_scipy=None):
    """y of one channel: float64 arithmetic on the float32 samples, zero initial state"""
    row = np.asarray(row, np.float32)
    if use_scipy is None:
        use_scipy = _lfilter is not None
    if not use_scipy:
        return host_filter(row)
    y = row.astype(np.float64)
    for b0, b1, b2, a1, a2 in COEFFS:
        y = _lfilter([b0, b1, b2], [1.0, a1, a2], y)
    return y


def step_energies(x, rate=48000):
    """x [C][n] -> z [steps][C]: the mean of y^2 over every whole 100 ms step"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    step = rate // 10
    nsteps = x.shape[1] // step
    z = np.empty((nsteps, x.shape[0]))
    for c in range(x.shape[0]):
        y = k_weight(x[c])[:nsteps * step]
        z[:, c] = np.mean(np.square(y).reshape(nsteps, step), axis=1)
    return z


def _lk(p):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(p)


def window_powers(z, weights, w):
    """P of every window of w consecutive steps, hop one step"""
    z = np.asarray(z, np.float64)
    n = z.shape[0] - w + 1
    if n <= 0:
        return np.empty(0)
    zw = np.stack([z[j:j + w].mean(axis=0) for j in range(n)])
    return zw @ np.asarray(weights, np.float64)


def gate_details(z, weights):
    """(P_j, l_j, Gamma_r) of the 400 ms blocks; Gamma_r None when no block passes the absolute gate"""
    P = window_powers(z, weights, 4)
    l = _lk(P)
    ja = l > -70.0
    gamma = _lk(P[ja].mean()) - 10.0 if ja.any() else None
    return P, l, gamma


def gate(z, weights):
    """(integrated, max momentary, max short-term); -inf where undefined"""
    P, l, gamma = gate_details(z, weights)
    integrated = -np.inf
    if gamma is not None:
        jg = (l > -70.0) & (l > gamma)
        if jg.any():
            integrated = _lk(P[jg].mean())
    mom = l.max() if l.size else -np.inf
    st = window_powers(z, weights, 30)
    return float(integrated), float(mom), float(_lk(st).max()) if st.size else -np.inf


def gate_margin(z, weights):
    """the smallest distance in LU of any block of the model from either gate (inf when there is none)"""
    _, l, gamma = gate_details(z, weights)
    fin = l[np.isfinite(l)]
    d = [np.abs(fin + 70.0).min()] if fin.size else []
    if gamma is not None and fin.size:
        d.append(np.abs(fin - gamma).min())
    return min(d) if d else np.inf


def channel_weight(azimuth, elevation, is_lfe):
    if is_lfe:
        return 0.0
    return 1.41 if abs(elevation) < 30.0 and 60.0 <= abs(azimuth) <= 120.0 else 1.0


def within_bound(z, z_model):
    """the accuracy bound of step energies, everywhere: |z - z_model| <= 1e-9 z_model + 1e-18 Z_c, Z_c the channel's largest
    model step energy.  Returns (ok, the worst |z - z_model| / (z_model + 1e-9 Z_c)): the second is what DESIGN.md quotes."""
    z, z_model = np.asarray(z, np.float64), np.asarray(z_model, np.float64)
    assert z.shape == z_model.shape, (z.shape, z_model.shape)
    zc = z_model.max(axis=0, keepdims=True)
    err = np.abs(z - z_model)
    ok = bool(np.all(err <= 1e-9 * z_model + 1e-18 * zc))
    worst = float(np.max(err / (z_model + 1e-9 * zc + 1e-300))) if z.size else 0.0
    return ok, worst
