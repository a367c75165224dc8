"""A float64 model of the biquad filter matrix (include/earhip.h, group O), written from the header's text and not from the
product code: scipy.signal.sosfilt per route on the float32 samples, then the float64 sum over the routes of an output in
ascending list index, rounded to float32 once by whoever compares.

THE BOUND every form of the stage is held to against this model, under any cutting of the stream:
    |y - ref| <= 2^-24 |ref| + 1e-9 * (the peak of |ref| over that output row)
The first term is the one rounding to float32.  The second covers the difference between float64 formulations of the same
recursion — sosfilt's, the header's fused multiply-adds, and above all the chunked form's propagated states: for the filters
of the tests (pole radius up to 0.9994) a plain float64 chunked form lies 7e-13 to 3e-11 of the peak from sosfilt at chunk
lengths 64, 256 and 1024, and sosfilt lies 4e-14 to 2e-12 from a long-double run of the recurrence (long_double_run below), so
the model alone sits at least 30x inside the bound."""
import os
import struct
import subprocess
import tempfile

import numpy as np
from scipy.signal import butter, sosfilt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_BUTTER = 2.0 ** -0.5


def sos_of(sections):
    """[S][5] b0 b1 b2 a1 a2 -> scipy's [S][6]"""
    s = np.asarray(sections, np.float64).reshape(-1, 5)
    return np.concatenate([s[:, :3], np.ones((s.shape[0], 1)), s[:, 3:]], axis=1)


def sections_of(sos):
    """scipy's [S][6] (a0 = 1) -> [S][5]"""
    sos = np.asarray(sos, np.float64)
    assert np.all(sos[:, 3] == 1.0)
    return np.ascontiguousarray(sos[:, [0, 1, 2, 4, 5]])


def butter_sections(order, f0, fs, kind="lowpass"):
    return sections_of(butter(order, f0, btype=kind, fs=fs, output="sos"))


def lr4(kind, f0, fs):
    """a Linkwitz-Riley 4th-order filter: two Butterworth 2nd-order sections of one kind"""
    return np.concatenate([butter_sections(2, f0, fs, kind)] * 2)


def model(x, n_out, routes):
    """x [n_in][n] float32, routes [(in, out, gain, sections or None)] -> ref [n_out][n] float64 (not yet rounded)"""
    x = np.atleast_2d(np.asarray(x, np.float32)).astype(np.float64)
    ref = np.zeros((n_out, x.shape[1]))
    for rin, rout, gain, sections in routes:
        z = x[rin] if sections is None or len(sections) == 0 else sosfilt(sos_of(sections), x[rin])
        ref[rout] = ref[rout] + float(gain) * z
    return ref


def long_double_run(x, sections):
    """the header's recurrence on one row in long double (no fused operations: the extended format's roundings are 2^-64)"""
    c = np.asarray(sections, np.longdouble).reshape(-1, 5)
    st = np.zeros((c.shape[0], 2), np.longdouble)
    out = np.empty(len(x), np.longdouble)
    for i, v in enumerate(np.asarray(x, np.float32).astype(np.longdouble)):
        for s in range(c.shape[0]):
            y = c[s, 0] * v + st[s, 0]
            st[s, 0] = c[s, 1] * v - c[s, 3] * y + st[s, 1]
            st[s, 1] = c[s, 2] * v - c[s, 4] * y
            v = y
        out[i] = v
    return out


def bound(ref):
    """[n_out][n]"""
    ref = np.atleast_2d(ref)
    return 2.0 ** -24 * np.abs(ref) + 1e-9 * np.abs(ref).max(axis=1, keepdims=True)


def worst_ratio(y, ref):
    """the largest |y - ref| / bound; where the bound is 0 (a silent row) the error must be 0"""
    y, ref = np.atleast_2d(np.asarray(y, np.float64)), np.atleast_2d(ref)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    b, err = bound(ref), np.abs(y - ref)
    assert np.all(err[b == 0] == 0)
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


def bass_management(names, fs, fc=80.0):
    """the route list of INTEGRATION.md for a BS.2051 layout given by its channel names: every main through a high-pass LR4, the
    mains' low-pass LR4 into every LFE channel (the sum of the mains scaled by 1 / the number of LFEs), LFE passed through"""
    lfe = [i for i, n in enumerate(names) if n.startswith("LFE")]
    mains = [i for i, n in enumerate(names) if not n.startswith("LFE")]
    routes = [(i, i, 1.0, lr4("highpass", fc, fs)) for i in mains]
    for k in lfe:
        routes.append((k, k, 1.0, None))
        routes += [(i, k, 1.0 / len(lfe), lr4("lowpass", fc, fs)) for i in mains]
    return routes


def cuttings(n, Lc, seed=0):
    """name -> call lengths that sum to n: the chunk length's neighbours, calls that start mid-chunk, short calls back to back"""
    rng = np.random.default_rng(seed)
    special = [0, 1, Lc - 1, Lc, Lc + 1, 0, 3, 5, 7, 2 * Lc + 9, Lc // 2, Lc // 2 + 1, 1, 1]
    assert sum(special) < n
    short = [int(v) for v in rng.integers(1, Lc, 12)]
    return {"one call": [n],
            "around the chunk length": special + [n - sum(special)],
            "short calls back to back": short + [n - sum(short)],
            "two halves off the grid": [n // 2 + 3, n - n // 2 - 3]}


# ---- libear_amd/csrc/iir.h compiled for the host ---------------------------------------------------------------------------------
_exe = {}


def host_exe(sanitize=True):
    """tests/cpp/iir_host.cpp built once per session: under ASan and UBSan (the CPU suite), or plainly"""
    if sanitize not in _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="iir_host_"), "iir_host")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"] if sanitize else ["-O2"]
        res = subprocess.run(["g++", "-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                             [os.path.join(ROOT, "tests", "cpp", "iir_host.cpp"), "-o", exe],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode == 0, res.stdout
        _exe[sanitize] = exe
    return _exe[sanitize]


def host_run(x, n_out, routes, calls=None, chunked=True, sanitize=True, expect=0):
    """x [n_in][n] through IirBankRef in calls of the given lengths -> out [n_out][n] float32 (expect = 3: the refusal's text)"""
    x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
    n_in, n = x.shape
    calls = np.asarray([n] if calls is None else calls, np.uint64)
    assert int(calls.sum()) == n
    exe = host_exe(sanitize)
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<6iQ", n_in, n_out, len(routes), int(bool(chunked)), calls.size, 0, n))
        for rin, rout, gain, sections in routes:
            sec = np.zeros((0, 5)) if sections is None else np.asarray(sections, np.float64).reshape(-1, 5)
            c = np.zeros((8, 5))
            c[:min(sec.shape[0], 8)] = sec[:8]
            f.write(struct.pack("<4id", rin, rout, sec.shape[0], 0, float(gain)) + c.tobytes())
        f.write(calls.tobytes() + x.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == expect, res.stdout
    if expect:
        return res.stdout
    raw = open(fout, "rb").read()
    assert len(raw) == 4 * n_out * n
    return np.frombuffer(raw, np.float32).reshape(n_out, n)
