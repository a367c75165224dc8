"""The HIP gain stage against libear's own GainInterpolator (include/ear/dsp/gain_interpolator.hpp), at the edges where
kernels drift: steps on and off call boundaries, equal neighbours (bit-equal, +0 / -0, NaN), single points, curves
outside the call, ramps of 1 .. 2^31 - 1 samples evaluated in windows, sample times around 0 and +-2^40, extrapolation,
denormal / zero / overflowing gains and inputs, shapes off the powers of two.

libear's outputs come from the committed fixture tests/golden/gain_interp_ref.npz (tests/golden/make_interp_golden.py),
and, where this tree holds oracle/_ref/libref_interp.so, from the compiled reference as well.

Bars:
  * the interpolation ABI (earhip_interp_apply_*), the whole-curve interpolator (earhip_gain_interp_*) and the renderer's
    gain stage in strict mode: bit for bit (np.array_equal, NaN equal to NaN);
  * the renderer's fast kernels (MFMA 1, 3, 4, 5, 6 forced, and the library's own choice) on the cases within their
    claim (finite, normal gains and inputs): per channel relative RMS <= 1e-6 against libear (their bar against the
    oracle in test_gpu_render.py), no further from a float64 evaluation than libear's own output (1.25x, or 1e-6), and on
    every sample within 1e-5 of the channel's largest magnitude — a step made a ramp, or an equal-neighbour segment made
    a ramp (or the reverse), is off by the size of the step and fails that."""
import numpy as np
import pytest

import _oracle
import scenes
from _hip import ctx, with_options
from refcases import interp_golden

pytestmark = pytest.mark.gpu

GEN, GOLD = interp_golden()
FAST_KERNELS = (None, 1, 3, 4, 5, 6)  # EARHIP_MFMA; None: the library's choice


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def strict(fn):
    ctx().set_strict(True)
    try:
        return fn()
    finally:
        ctx().set_strict(False)


def libear(name, live):
    """libear's output for a fixture case: the fixture's, checked against the compiled reference where it exists"""
    want = GOLD[name + ".want"]
    ref = _oracle.load_ref_interp()
    if ref is not None:
        assert same(live(ref), want), name
    return want


# ---- (A) interpolation policies --------------------------------------------------------------------------------------
def policy_refused(m):
    """earhip_interp_apply_interp takes samples less than 2^30 from the curve's start (api_core.hip); libear has no
    such limit, so those calls must be refused, never computed differently"""
    if not m["interp"]:
        return False
    first = m["block_start"] + m["r0"] - m["start"]
    return not (first > -(1 << 30) and first + (m["r1"] - m["r0"]) < (1 << 30))


def policy_hip(name):
    m = GEN.meta(GOLD, name)
    x = np.ascontiguousarray(GOLD[name + ".x"])
    out = np.zeros_like(GOLD[name + ".want"])
    if m["interp"]:
        ctx().apply_interp(x, out, m["r0"], m["r1"], m["block_start"], m["start"], m["end"], GOLD[name + ".sp"],
                           GOLD[name + ".ep"])
    else:
        ctx().apply_constant(x, out, m["r0"], m["r1"], GOLD[name + ".sp"])
    return out


def policy_live(name):
    m = GEN.meta(GOLD, name)

    def run(ref):
        out = np.zeros_like(GOLD[name + ".want"])
        return _oracle.ref_policy(ref, m["kind"], GOLD[name + ".x"], out, m["r0"], m["r1"], m["block_start"],
                                  m["start"], m["end"], GOLD[name + ".sp"], GOLD[name + ".ep"] if m["interp"] else None)
    return run


@pytest.mark.parametrize("name", GEN.cases(GOLD, "pol"))
def test_policy_bit_exact_against_libear(name):
    from libear_amd import capi
    m = GEN.meta(GOLD, name)
    want = libear(name, policy_live(name))
    if policy_refused(m):
        with pytest.raises(capi.InvalidArgument):
            strict(lambda: policy_hip(name))
        return
    assert same(strict(lambda: policy_hip(name)), want)
    if m["n_in"] == 1:  # 1 -> 1, 1 -> N: no accumulation, exact in either mode
        assert same(policy_hip(name), want)
    elif m["fast"]:  # M -> N in the default mode: fused multiply-adds and tree sums
        assert scenes.rel_rms_per_channel(policy_hip(name), want) <= 1e-6


# ---- (A') the whole-curve interpolator -------------------------------------------------------------------------------
def gi_live(name):
    m = GEN.meta(GOLD, name)

    def run(ref):
        sets = GEN.gi_point_sets(GOLD, name)
        gi = _oracle.RefGainInterp(ref, m["n_in"], m["n_out"])
        out = np.zeros_like(GOLD[name + ".want"])
        ofs = 0
        for bs, n, ps in GOLD[name + ".calls"]:
            if ps >= 0:
                gi.set_points(*sets[ps])
            if n:
                out[:, ofs:ofs + n] = gi.process(int(bs), GOLD[name + ".x"][:, ofs:ofs + n])
            ofs += int(n)
        return out
    return run


def gi_hip(name, device):
    import torch
    from libear_amd import capi
    m = GEN.meta(GOLD, name)
    sets = GEN.gi_point_sets(GOLD, name)
    x = GOLD[name + ".x"]
    out = np.full_like(GOLD[name + ".want"], np.float32(7.0))
    gi = capi.GainInterp(ctx(), m["n_in"], m["n_out"])
    try:
        ofs = 0
        for bs, n, ps in GOLD[name + ".calls"]:
            bs, n = int(bs), int(n)
            if ps >= 0:
                gi.set_points(*sets[ps])
            xs = np.ascontiguousarray(x[:, ofs:ofs + n])
            if not device:
                y = gi.process(bs, xs)
            else:
                stride = max(4, (n + 3) // 4 * 4)
                xd = torch.zeros((m["n_in"], stride), dtype=torch.float32, device="cuda")
                xd[:, :n] = torch.from_numpy(xs).cuda()
                yd = torch.full((m["n_out"], stride), 7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                gi.process_device(bs, n, xd.data_ptr(), stride, yd.data_ptr(), stride)
                ctx().synchronize()
                y = yd[:, :n].cpu().numpy()
            out[:, ofs:ofs + n] = y
            ofs += n
    finally:
        gi.close()
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", GEN.cases(GOLD, "gi"))
def test_gain_interp_bit_exact_against_libear(name, device):
    m = GEN.meta(GOLD, name)
    want = libear(name, gi_live(name))
    assert same(strict(lambda: gi_hip(name, device)), want)
    if m["n_in"] == 1:  # no accumulation: exact in the default mode as well
        assert same(gi_hip(name, device), want)
    elif m["fast"]:
        assert scenes.rel_rms_per_channel(gi_hip(name, device), want) <= 1e-6


# ---- (F) the renderer's gain stage -----------------------------------------------------------------------------------
def render_live(name):
    m = GEN.meta(GOLD, name)

    def run(ref):
        objs = _oracle.RefObjects(ref, m["M"], m["N"])
        for i, (t, g) in enumerate(GEN.render_curves(GOLD, name)):
            objs.set_points(i, t, g)
        B, x = m["B"], GOLD[name + ".x"]
        return np.concatenate([objs.process(m["t0"] + b * B, x[:, b * B:(b + 1) * B]) for b in range(m["nblocks"])],
                              axis=1)
    return run


def render_hip(name):
    """direct bus only, no decorrelation, delay 0: the output is the gain stage's bus; the call partition of the case,
    from the clock set with reset(t0).  -> (output, launch plan of the last call)"""
    from libear_amd import capi
    m = GEN.meta(GOLD, name)
    B, x = m["B"], GOLD[name + ".x"]
    r = capi.Renderer(ctx(), m["M"], m["N"], B, None, 0, max_blocks=max(m["calls"]))
    try:
        for i, (t, g) in enumerate(GEN.render_curves(GOLD, name)):
            r.set_object_points(i, t, g)
        r.reset(m["t0"])
        out, ofs, kernels = np.zeros_like(GOLD[name + ".want"]), 0, set()
        for nb in m["calls"]:
            out[:, ofs:ofs + nb * B] = r.process(np.ascontiguousarray(x[:, ofs:ofs + nb * B]))
            kernels.add(r.gain_kernel())
            ofs += nb * B
        plan = r.last_plan()
        plan["kernels"] = sorted(kernels)
    finally:
        r.close()
    return out, plan


def render_f64(name):
    """float64 evaluation of the case: libear's segmentation, exact arithmetic"""
    m = GEN.meta(GOLD, name)
    x = GOLD[name + ".x"].astype(np.float64)
    t = m["t0"] + np.arange(x.shape[1], dtype=np.int64)
    out = np.zeros((m["N"], x.shape[1]))
    for i, (times, g) in enumerate(GEN.render_curves(GOLD, name)):
        k = np.searchsorted(times, t, side="right")
        n = len(times)
        lo, hi = np.clip(k - 1, 0, n - 1), np.clip(k, 0, n - 1)
        inside = (k > 0) & (k < n)
        span = np.where(inside, times[hi] - times[lo], 1).astype(np.float64)
        p = np.where(inside, (t - times[lo]).astype(np.float64) / span, 0.0)
        g64 = g.astype(np.float64)
        gain = g64[lo] * (1 - p)[:, None] + g64[hi] * p[:, None]
        gain[k == 0] = g64[0]
        gain[k == n] = g64[n - 1]
        out += (gain * x[i][:, None]).T
    return out


@pytest.mark.parametrize("name", GEN.cases(GOLD, "rn"))
def test_render_strict_bit_exact_against_libear(name):
    want = libear(name, render_live(name))
    got, plan = strict(lambda: render_hip(name))
    print(f"{name}: strict, gain kernel {plan['kernels']}")
    assert plan["kernels"] == [0], plan
    assert same(got, want)


@pytest.mark.parametrize("mfma", FAST_KERNELS, ids=lambda v: "auto" if v is None else f"mfma{v}")
@pytest.mark.parametrize("name", [n for n in GEN.cases(GOLD, "rn") if GEN.meta(GOLD, n)["fast"]])
def test_render_fast_kernels_against_libear(name, mfma):
    want = libear(name, render_live(name))
    got, plan = with_options({"EARHIP_MFMA": mfma}, lambda: render_hip(name))
    print(f"{name}: MFMA={mfma}, gain kernel {plan['kernels']} (tile {plan['tile']}, {plan['ntiles']} tiles)")
    assert all(k >= 0 for k in plan["kernels"]), plan
    if mfma is None:
        assert 0 not in plan["kernels"], plan  # strict mode is off: the library picks a fast kernel
    elif mfma >= 3 and name.startswith("rn.split_"):  # 64 objects on whole tiles: the split-operand kernels take them
        assert set(plan["kernels"]) <= {3, 4, 5}, plan
    err = scenes.rel_rms_per_channel(got, want)
    assert err <= 1e-6, (err, plan)
    truth = render_f64(name)
    e_gpu, e_lib = scenes.rel_rms_per_channel(got, truth), scenes.rel_rms_per_channel(want, truth)
    assert e_gpu <= max(1.25 * e_lib, 1e-6), (e_gpu, e_lib, plan)
    scale = np.max(np.abs(want), axis=1, keepdims=True)
    bad = np.abs(got.astype(np.float64) - want) > 1e-5 * scale
    assert not bad.any(), (np.argwhere(bad)[:8], plan)


def test_render_refuses_block_sizes_below_16():
    """libear's gain stage takes any block; the renderer's configuration range is [16, 4096] (earhip.h): blocks of 1, 2
    and 3 samples are refused, not computed (the interpolators above take calls of any length, 0 and 1 included)"""
    from libear_amd import capi
    for B in (1, 2, 3, 15):
        with pytest.raises(capi.InvalidArgument):
            capi.Renderer(ctx(), 1, 2, B, None, 0, max_blocks=1)
