"""Generates tests/golden/gain_interp_ref.npz from the REFERENCE's own GainInterpolator
(include/ear/dsp/gain_interpolator.hpp), compiled in place into oracle/_ref/libref_interp.so
(oracle/Makefile target `ref`, oracle/ref_interp_capi.cpp).  Run where the reference tree exists:
python tests/golden/make_interp_golden.py

Fixture = libear's outputs (data only), with per case its description and the SHA-256 of the inputs they were
computed from (generate()).  The inputs themselves are not stored: this module builds them — from numpy's
PCG64 with fixed seeds and the rules below — without the reference (inputs()), and load() checks them against
those digests before a test uses them, so a changed generator or random stream cannot go unnoticed.  The file
regenerates identically (tests/test_oracle_gain_interp.py checks that).  Long curves are evaluated in windows: the
points, and a short stretch of audio at the ramp's start, middle or end.

Three kinds of case, each a set of arrays under "<name>.":
  pol.*  one call of LinearInterp{Single,Vector,Matrix}::apply_interp / ::apply_constant:
         x [n_in][n], sp / ep [n_in][n_out], want [n_out][n] (zero outside [r0, r1)).
  gi.*   one GainInterpolator<LinearInterpMatrix> over a sequence of calls (block_start, nsamples) whose
         points may be replaced before a call: x [n_in][sum n], want [n_out][sum n], point sets p<j>.t / p<j>.v,
         calls [k][3] (block_start, nsamples, point set to install first or -1).
  rn.*   the objects gain stage (one GainInterpolator<LinearInterpVector> per object, summed into the bus in
         object order) over nblocks blocks of B samples from sample t0: x [M][nblocks B], want [N][nblocks B],
         curves as ct (all times), cg (all gains [P][N]) and co (object m's points: co[m] .. co[m + 1]).
meta["fast"]: the case is within what the fast (non-strict) kernels claim (finite gains of ordinary size, normal
numbers); the others are for the exact paths only.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _oracle  # noqa: E402

NAME = "gain_interp_ref.npz"
RAMPS = (1, 2, 3, (1 << 24) - 1, (1 << 24) + 1, (1 << 25) + 3, (1 << 31) - 1)
FMAX = np.float32(3.0e38)
DEN = np.float32(1e-40)  # a float32 denormal


def kind_of(n_in, n_out):
    return "single" if n_in == n_out == 1 else "vector" if n_in == 1 else "matrix"


def _meta(**kw):
    return np.array(json.dumps(kw, sort_keys=True))


# ---- interpolation policies ------------------------------------------------------------------------------------------
def policy_cases(rng):
    cases = []  # (name, meta, x, sp, ep)

    def add(name, n_in, n_out, n, r0, r1, block_start, start, end, interp, x=None, sp=None, ep=None, fast=True):
        x = rng.uniform(-1, 1, (n_in, n)).astype(np.float32) if x is None else x
        sp = rng.uniform(-1, 1, (n_in, n_out)).astype(np.float32) if sp is None else sp
        ep = rng.uniform(-1, 1, (n_in, n_out)).astype(np.float32) if ep is None else ep
        m = dict(kind=kind_of(n_in, n_out), interp=interp, n_in=n_in, n_out=n_out, r0=r0, r1=r1,
                 block_start=block_start, start=start, end=end, fast=fast)
        cases.append((name, m, x, sp, ep))

    # shapes: the range reaches before start (p < 0) and past end (p > 1)
    for n_in in (1, 2, 3, 33, 64, 257):
        for n_out in (1, 2, 7, 24, 64):
            bs = int(rng.integers(-1000, 1000))
            add(f"pol.shape_{n_in}x{n_out}_interp", n_in, n_out, 12, 1, 11, bs, bs + 4, bs + 8, True)
            add(f"pol.shape_{n_in}x{n_out}_const", n_in, n_out, 12, 1, 11, bs, 0, 1, False)
    # ramp lengths, windows at the start, in the middle and at the end (and past it)
    for L in RAMPS:
        for where, ofs in (("start", -5), ("mid", L // 2 - 8), ("end", L - 8)):
            for bs in (0, -(1 << 40) - 17, (1 << 40) + 3):
                start = bs + 11
                add(f"pol.ramp{L}_{where}_t{bs}", 1, 2, 16, 0, 16, start + ofs, start, start + L, True)
    # extrapolation far outside the curve (p << 0 and p >> 1)
    add("pol.extrap_before", 2, 3, 50, 0, 50, -5000, 100, 164, True)
    add("pol.extrap_after", 2, 3, 50, 0, 50, 7000, 100, 164, True)
    # zero-length ranges write nothing
    add("pol.empty_interp", 3, 7, 16, 9, 9, 0, 0, 10, True)
    add("pol.empty_const", 3, 7, 16, 0, 0, 0, 0, 1, False)
    # equal points through apply_interp still ramp: (1 - p) s + p s
    s = rng.uniform(-1, 1, (2, 5)).astype(np.float32)
    add("pol.equal_points_interp", 2, 5, 40, 0, 40, 0, 7, 20, True, sp=s, ep=s.copy())
    # gains and inputs at the edges of float32
    xe = rng.uniform(-1, 1, (2, 48)).astype(np.float32)
    xe[0, ::5] = DEN
    xe[0, 1::5] = -DEN
    xe[1, ::7] = 0.0
    xe[1, 1::7] = -0.0
    xe[1, 2::7] = 1.0
    xe[1, 3::7] = -1.0
    ge = np.float32([[0.0, DEN, -DEN, 0.5, -0.25], [FMAX, -FMAX, 1.0, -1.0, 2.5e-39]])
    gf = np.float32([[DEN, 0.0, 0.75, -DEN, FMAX], [-FMAX, FMAX, -0.0, 1.0, 0.0]])
    add("pol.edges_interp", 2, 5, 48, 0, 48, 0, 5, 40, True, x=xe, sp=ge, ep=gf, fast=False)
    add("pol.edges_const", 2, 5, 48, 0, 48, 0, 0, 1, False, x=xe, sp=ge, fast=False)
    add("pol.edges_const_b", 2, 5, 48, 2, 45, 0, 0, 1, False, x=xe, sp=gf, fast=False)
    return cases


def policy_inputs(rng, out):
    for name, m, x, sp, ep in policy_cases(rng):
        out[name + ".meta"] = _meta(**m)
        out[name + ".x"], out[name + ".sp"], out[name + ".ep"] = x, sp, ep


# ---- GainInterpolator<LinearInterpMatrix> across calls --------------------------------------------------------------
def ragged_points(rng, n_in, n_out, t_lo, t_hi, npts):
    """sorted times in [t_lo, t_hi) with steps (repeated times), equal neighbours and ramps"""
    t = np.sort(rng.integers(t_lo, t_hi, npts)).astype(np.int64)
    t[1::4] = t[0::4][:len(t[1::4])]  # steps
    t = np.sort(t)
    v = rng.uniform(-1, 1, (npts, n_in, n_out)).astype(np.float32)
    for k in range(2, npts, 5):
        v[k] = v[k - 1]  # equal neighbours: constant segments
    return t, v


def gi_cases(rng):
    cases = []  # (name, meta, point sets, calls [(block_start, n, point set or -1)])

    def contiguous(t0, sizes, sets_at=None):
        calls, t = [], t0
        for k, n in enumerate(sizes):
            calls.append((t, n, (sets_at or {0: 0}).get(k, -1)))
            t += n
        return calls

    # call partitions: one-sample and zero-length calls, the points replaced between calls, a jump back in time
    n_in, n_out = 3, 2
    p0 = ragged_points(rng, n_in, n_out, 0, 400, 24)
    p1 = ragged_points(rng, n_in, n_out, 150, 600, 17)
    p2 = (np.int64([200, 200, 200, 450]), rng.uniform(-1, 1, (4, n_in, n_out)).astype(np.float32))
    sizes = [1, 1, 0, 5, 1, 64, 0, 1, 100, 3, 2, 1, 90, 0, 45, 1, 1, 200]
    calls = contiguous(0, sizes, {0: 0, 9: 1, 14: 2})
    calls += [(120, 50, 0), (110, 7, -1), (700, 30, 1)]
    cases.append(("gi.partitions", dict(n_in=n_in, n_out=n_out, fast=True), [p0, p1, p2], calls))
    # shapes
    for n_in, n_out in ((1, 1), (1, 24), (2, 2), (33, 7), (64, 64), (257, 1), (257, 24)):
        p = ragged_points(rng, n_in, n_out, -10, 60, 12 if n_in * n_out < 1000 else 6)
        calls = contiguous(-20, [1, 2, 3, 45] if n_in * n_out < 1000 else [1, 2, 3, 13])
        cases.append((f"gi.shape_{n_in}x{n_out}", dict(n_in=n_in, n_out=n_out, fast=True), [p], calls))
    # steps exactly on a call boundary, on the first and on the last sample of a call; two and three points at
    # the same time; a curve ending inside a call; the whole curve before and after a call
    v = rng.uniform(-1, 1, (8, 2, 3)).astype(np.float32)
    t = np.int64([10, 10, 40, 40, 40, 64, 100, 100])
    calls = contiguous(0, [10, 30, 24, 40, 60])  # call boundaries at 10, 40, 64, 104
    cases.append(("gi.steps", dict(n_in=2, n_out=3, fast=True), [(t, v)], calls))
    cases.append(("gi.step_last_sample", dict(n_in=2, n_out=3, fast=True),
                  [(np.int64([0, 39, 39, 80]), v[:4])], contiguous(0, [40, 40, 40])))
    cases.append(("gi.outside_calls", dict(n_in=2, n_out=3, fast=True), [(np.int64([50, 70]), v[:2])],
                  [(0, 30, 0), (100, 30, -1), (60, 30, -1), (-200, 16, -1)]))
    cases.append(("gi.single_point", dict(n_in=2, n_out=3, fast=True), [(np.int64([25]), v[:1])],
                  contiguous(0, [20, 20])))
    # equal neighbours: bit-equal, +0 next to -0 (float-equal), NaN (never float-equal)
    a = rng.uniform(-1, 1, (1, 2, 3)).astype(np.float32)
    z = np.zeros((1, 2, 3), np.float32)
    nan = np.full((1, 2, 3), np.nan, np.float32)
    eq = np.concatenate([a, a, z, -z, z, nan, nan, a])
    cases.append(("gi.equal_neighbours", dict(n_in=2, n_out=3, fast=False),
                  [(np.int64([0, 20, 40, 60, 80, 100, 120, 140]), eq)], contiguous(0, [64, 64, 32])))
    # long ramps evaluated in windows, at sample times around 0, +-2^40
    for L in RAMPS[3:]:
        for base in (-(1 << 40), -1000, 0, 1 << 40):
            pts = (np.int64([base, base + L, base + L]), rng.uniform(-1, 1, (3, 1, 2)).astype(np.float32))
            calls = [(base - 3, 12, 0), (base + L // 2 - 4, 8, -1), (base + L - 8, 16, -1)]
            cases.append((f"gi.ramp{L}_t{base}", dict(n_in=1, n_out=2, fast=True), [pts], calls))
    return cases


def gi_inputs(rng, out):
    for name, m, sets, calls in gi_cases(rng):
        total = sum(n for _, n, _ in calls)
        x = rng.uniform(-1, 1, (m["n_in"], total)).astype(np.float32)
        out[name + ".meta"] = _meta(**m)
        out[name + ".x"] = x
        out[name + ".calls"] = np.int64(calls).reshape(-1, 3)
        for j, (t, v) in enumerate(sets):
            out[f"{name}.p{j}.t"], out[f"{name}.p{j}.v"] = np.int64(t), np.float32(v)


# ---- the objects gain stage ------------------------------------------------------------------------------------------
def ramp_curve(rng, n_out, start, length, hold=True):
    """one ramp of `length` samples from `start`; with hold, a repeated end point (libear's usual block metadata)"""
    t = [start, start + length] + ([start + length] if hold else [])
    g = rng.uniform(0, 1, (len(t), n_out)).astype(np.float32)
    if hold:
        g[2] = g[1]
    return np.int64(t), g


def render_cases(rng):
    cases = []  # (name, meta, curves [(times, gains)], x or None)

    def add(name, M, N, B, nblocks, t0, calls, curves, x=None, fast=True):
        assert sum(calls) == nblocks and len(curves) == M
        cases.append((name, dict(M=M, N=N, B=B, nblocks=nblocks, t0=t0, calls=calls, fast=fast), curves, x))

    # shapes: ragged curves (steps, equal neighbours, ramps across calls)
    for M, B, nblocks, calls in ((1, 4096, 1, [1]), (1, 512, 2, [1, 1]), (33, 45, 5, [2, 1, 2]), (33, 1000, 1, [1]),
                                 (33, 480, 2, [1, 1]), (257, 64, 2, [2]), (257, 16, 5, [1, 4]), (33, 512, 2, [1, 1])):
        N = 1 if B == 4096 else 2 if M == 1 or B >= 480 else 3
        total = B * nblocks
        curves = []
        for m in range(M):
            t, v = ragged_points(rng, 1, N, -total // 4, total + total // 4, int(rng.integers(1, 14)))
            curves.append((t, np.abs(v[:, 0, :])))
        add(f"rn.shape_M{M}_B{B}", M, N, B, nblocks, 0, calls, curves)
    # steps: two and three points at the same time, on a call boundary, on the first and last sample of a call
    B, M, N = 45, 33, 7
    edges = [0, 1, 44, 45, 46, 89, 90, 134, 135, 200, 269]
    curves = []
    for m in range(M):
        e = int(edges[m % len(edges)])
        k = 2 + m % 2  # points at time e
        t = np.int64([e - 30] + [e] * k + [e + 37])
        curves.append((t, rng.uniform(0, 1, (len(t), N)).astype(np.float32)))
    add("rn.steps", M, N, B, 6, 0, [1, 2, 3], curves)
    # equal neighbours (bit-equal and +0 / -0), single points, curves wholly before / after / ending inside the call
    curves = []
    for m in range(M):
        a = rng.uniform(0, 1, (1, N)).astype(np.float32)
        b = rng.uniform(0, 1, (1, N)).astype(np.float32)
        z = np.zeros((1, N), np.float32)
        kind = m % 6
        if kind == 0:
            curves.append((np.int64([10, 100, 200]), np.concatenate([b, a, a])))
        elif kind == 1:
            zz = z.copy()
            zz[0, ::2] = -0.0
            curves.append((np.int64([0, 64, 150, 250]), np.concatenate([a, z, zz, b])))
        elif kind == 2:
            curves.append((np.int64([int(rng.integers(-50, 300))]), a))
        elif kind == 3:
            curves.append((np.int64([-900, -400]), np.concatenate([a, b])))
        elif kind == 4:
            curves.append((np.int64([5000, 9000]), np.concatenate([b, a])))
        else:
            curves.append((np.int64([-100, 77]), np.concatenate([b, a])))
    add("rn.equal_neighbours", M, N, 64, 5, 0, [2, 3], curves)
    # NaN gains (never float-equal): libear ramps between them
    curves = [(np.int64([0, 50, 100, 150]), np.float32([[0.5] * 3, [np.nan] * 3, [np.nan] * 3, [0.25] * 3]))]
    curves.append((np.int64([0, 64]), rng.uniform(0, 1, (2, 3)).astype(np.float32)))
    add("rn.nan_gains", 2, 3, 64, 4, 0, [4], curves, fast=False)
    # ramps of every length, windows at the start / middle / end, sample times around 0, +-2^40
    for L in RAMPS:
        for base in (-(1 << 40), -1000, 0, 1 << 40):
            for where in ("start", "mid", "end") if L > 1000 else ("start",):
                # the objects' ramps start (and end) spread over the window
                M, N, B = 17, 2, 32
                ofs = {"start": -32, "mid": L // 2 - 32, "end": L - 32}[where]
                curves = [ramp_curve(rng, N, base + 4 * m - 32, L) for m in range(M)]
                add(f"rn.ramp{L}_{where}_t{base}", M, N, B, 2, base + ofs, [1, 1], curves)
    # the longest ramp's end under whole 512-sample tiles
    L, base = RAMPS[-1], 1 << 40
    curves = [ramp_curve(rng, 2, base + 29 * m - 400, L) for m in range(33)]
    add("rn.ramp_longest_end_B512", 33, 2, 512, 2, base + L - 512, [2], curves)
    # the same edges on 64 objects and whole 512-sample tiles, where the split-operand kernels (3-6) take the call
    M, N, B = 64, 2, 512
    curves = []
    for m in range(M):
        kind = m % 8
        a, b = rng.uniform(0, 1, (2, 1, N)).astype(np.float32)
        z = np.zeros((1, N), np.float32)
        if kind == 0:  # steps on a call boundary and on a tile boundary, three points at one time
            curves.append((np.int64([100, 512, 512, 768, 768, 768, 900]), rng.uniform(0, 1, (7, N)).astype(np.float32)))
        elif kind == 1:  # steps on the first and the last sample of a call
            curves.append((np.int64([0, 0, 1023, 1023]), rng.uniform(0, 1, (4, N)).astype(np.float32)))
        elif kind == 2:  # bit-equal neighbours inside a tile
            curves.append((np.int64([37, 300, 700]), np.concatenate([b, a, a])))
        elif kind == 3:  # +0 next to -0
            zz = z.copy()
            zz[0, 1::2] = -0.0
            curves.append((np.int64([50, 200, 620, 980]), np.concatenate([a, z, zz, b])))
        elif kind == 4:  # one point
            curves.append((np.int64([int(rng.integers(-100, 1100))]), a))
        elif kind == 5:  # ends inside the call
            curves.append((np.int64([-300, 333]), np.concatenate([b, a])))
        else:  # ramps across the call
            curves.append((np.int64([-200, 1300]), np.concatenate([b, a])))
    add("rn.split_edges_M64", M, N, B, 2, 0, [1, 1], curves)
    for L in RAMPS[4:]:  # long ramps ending inside the window, at +-2^40
        base = (1 << 40) if L % 2 else -(1 << 40)
        curves = [ramp_curve(rng, N, base + 11 * m - 300, L) for m in range(M)]
        add(f"rn.split_ramp{L}_end", M, N, B, 2, base + L - 512, [2], curves)
    # denormal gains and inputs, zeros of both signs, full scale
    M, N, B, nblocks = 33, 7, 64, 3
    total = B * nblocks
    x = rng.uniform(-1, 1, (M, total)).astype(np.float32)
    x[::3, ::5] = DEN
    x[1::3, ::4] = -DEN
    x[2::3, ::3] = -0.0
    x[::4, 1::7] = 1.0
    x[::5, 2::7] = -1.0
    curves = []
    for m in range(M):
        t = np.int64([0, 70, 70, 150])
        g = rng.uniform(0, 1, (4, N)).astype(np.float32)
        g[:, m % N] = DEN
        g[1, (m + 1) % N] = 0.0
        g[:, (m + 2) % N] *= -1
        curves.append((t, g))
    add("rn.denormals", M, N, B, nblocks, 0, [1, 2], curves, x=x, fast=False)
    # gains near FLT_MAX: products and sums overflow to +-inf
    curves = [(np.int64([0, 100]), np.float32([[FMAX, -FMAX, 1.0], [FMAX, FMAX, -FMAX]])),
              (np.int64([30, 30, 90]), np.float32([[FMAX, 0.5, FMAX], [-FMAX, 0.25, FMAX], [0.0, FMAX, FMAX]]))]
    add("rn.overflow", 2, 3, 64, 3, 0, [3], curves, fast=False)
    return cases


def render_inputs(rng, out):
    for name, m, curves, x in render_cases(rng):
        if x is None:
            x = rng.uniform(-1, 1, (m["M"], m["B"] * m["nblocks"])).astype(np.float32)
        out[name + ".meta"] = _meta(**m)
        out[name + ".x"] = x
        out[name + ".ct"] = np.concatenate([t for t, _ in curves]).astype(np.int64)
        out[name + ".cg"] = np.concatenate([g for _, g in curves]).astype(np.float32)
        out[name + ".co"] = np.int64(np.cumsum([0] + [len(t) for t, _ in curves]))


def inputs():
    """every case's inputs and description, built without the reference"""
    out = {}
    policy_inputs(np.random.default_rng(20261015), out)
    gi_inputs(np.random.default_rng(20261016), out)
    render_inputs(np.random.default_rng(20261017), out)
    return out


def digest(inp, name):
    """SHA-256 over a case's input arrays (name, dtype, shape and bytes of each, in name order)"""
    h = hashlib.sha256()
    for k in sorted(k for k in inp if k.startswith(name + ".") and k != name + ".meta"):
        a = np.ascontiguousarray(inp[k])
        h.update(f"{k[len(name):]}|{a.dtype.str}|{a.shape}|".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def outputs(ref, inp):
    """libear's outputs for every case of `inp` (ref: load_ref_interp(), or the oracle's lib() — the same entry points)"""
    out = {}
    for name in cases(inp, "pol"):
        m = meta(inp, name)
        want = np.zeros((m["n_out"], inp[name + ".x"].shape[1]), np.float32)
        _oracle.ref_policy(ref, m["kind"], inp[name + ".x"], want, m["r0"], m["r1"], m["block_start"], m["start"],
                           m["end"], inp[name + ".sp"], inp[name + ".ep"] if m["interp"] else None)
        out[name + ".want"] = want
    for name in cases(inp, "gi"):
        m = meta(inp, name)
        sets, x = gi_point_sets(inp, name), inp[name + ".x"]
        want = np.zeros((m["n_out"], x.shape[1]), np.float32)
        gi = _oracle.RefGainInterp(ref, m["n_in"], m["n_out"])
        ofs = 0
        for bs, n, ps in inp[name + ".calls"]:
            bs, n = int(bs), int(n)
            if ps >= 0:
                gi.set_points(*sets[ps])
            if n:
                want[:, ofs:ofs + n] = gi.process(bs, x[:, ofs:ofs + n])
            ofs += n
        out[name + ".want"] = want
    return out


def render_outputs(ref, inp):
    """the objects gain stage on libear's interpolator (the compiled reference only: the oracle's ObjectsRenderer is
    checked against these outputs by the tests)"""
    out = {}
    for name in cases(inp, "rn"):
        m = meta(inp, name)
        B, x = m["B"], inp[name + ".x"]
        objs = _oracle.RefObjects(ref, m["M"], m["N"])
        for i, (t, g) in enumerate(render_curves(inp, name)):
            objs.set_points(i, t, g)
        want = np.zeros((m["N"], x.shape[1]), np.float32)
        for b in range(m["nblocks"]):  # the block is libear's call
            want[:, b * B:(b + 1) * B] = objs.process(m["t0"] + b * B, x[:, b * B:(b + 1) * B])
        out[name + ".want"] = want
    return out


def generate(ref):
    """the fixture's contents: "index" (JSON: per case its description, the digest of its inputs and where its outputs
    lie in "want") and "want" (libear's outputs of every case, flattened and concatenated)"""
    inp = inputs()
    outs = outputs(ref, inp)
    outs.update(render_outputs(ref, inp))
    index, flat, ofs = [], [], 0
    for prefix in ("pol", "gi", "rn"):
        for name in cases(inp, prefix):
            w = outs[name + ".want"]
            index.append(dict(name=name, meta=json.loads(str(inp[name + ".meta"])), inputs=digest(inp, name),
                              offset=ofs, shape=list(w.shape)))
            flat.append(w.ravel())
            ofs += w.size
    return {"index": np.array(json.dumps(index)), "want": np.concatenate(flat).astype(np.float32)}


def load(path=None):
    """the cases as the tests read them: the inputs built here, checked against the fixture's digests, with the
    fixture's outputs under <name>.want"""
    gold = np.load(path or os.path.join(HERE, NAME))
    index, flat = json.loads(str(gold["index"])), gold["want"]
    inp = inputs()
    names = [n for p in ("pol", "gi", "rn") for n in cases(inp, p)]
    assert names == [c["name"] for c in index], "the fixture and the generator list other cases"
    for c in index:
        name = c["name"]
        assert c["inputs"] == digest(inp, name), f"{name}: inputs differ from those the fixture was made from"
        assert c["meta"] == meta(inp, name), name
        n = int(np.prod(c["shape"]))
        inp[name + ".want"] = flat[c["offset"]:c["offset"] + n].reshape(c["shape"])
    return inp


# ---- readers (the tests') --------------------------------------------------------------------------------------------
def cases(gold, prefix):
    """names of the cases of one kind ("pol", "gi", "rn"), in a stable order (gold: a case dict or the npz file)"""
    return sorted(k[:-5] for k in gold if k.startswith(prefix + ".") and k.endswith(".meta"))


def meta(gold, name):
    return json.loads(str(gold[name + ".meta"]))


def render_curves(gold, name):
    co, ct, cg = gold[name + ".co"], gold[name + ".ct"], gold[name + ".cg"]
    return [(ct[co[m]:co[m + 1]], cg[co[m]:co[m + 1]]) for m in range(len(co) - 1)]


def gi_point_sets(gold, name):
    sets, j = [], 0
    while f"{name}.p{j}.t" in gold:
        sets.append((gold[f"{name}.p{j}.t"], gold[f"{name}.p{j}.v"]))
        j += 1
    return sets


def main():
    ref = _oracle.load_ref_interp()
    assert ref is not None, "reference GainInterpolator not built (oracle/Makefile target `ref`)"
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **generate(ref))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
