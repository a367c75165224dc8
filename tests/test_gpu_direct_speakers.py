"""GainCalculatorDirectSpeakers on the GPU: the channels that fall back to the point source panner go to the device
panner in one launch per call.

  * batches of 4096 channels (labels, frequencies, random positions with and without bounds, LFE and not) on every
    BS.2051 layout and on layouts with moved loudspeakers, against an independent numpy restatement of libear's
    calculate (tests/ds_model.py) whose panner is the pinned oracle panner: 1e-6;
  * a batch equals its channels computed one at a time, and no position escapes the panner's regions;
  * a 4+7+0 bed (labels as URNs) through the renderer together with ramping objects: the bed gains become constant
    curves on the direct bus, compared per channel with the CPU oracle renderer (relative RMS <= 1e-6); the bed
    alone, in strict mode, is bit-exact against the oracle's LinearInterpVector.
"""
import numpy as np
import pytest

import _oracle
import ds_model
import scenes
from _hip import ctx
from libear_amd import capi

pytestmark = pytest.mark.gpu

SUBST = {"foo": "M+030"}


def _moved(layout, seed):
    """the layout's channels a few degrees off their nominal positions (full layout, LFE included)"""
    ch = capi.layout_channels(layout)
    az = np.array([c[1] for c in ch], np.float64)
    el = np.array([c[2] for c in ch], np.float64)
    rng = np.random.default_rng(seed)
    raz = az + rng.uniform(-4, 4, len(az))
    rel = np.clip(el + rng.uniform(-3, 3, len(el)), -90, 90)
    raz[np.abs(el) == 90] = az[np.abs(el) == 90]
    return raz, rel


def _batch(layout, n, seed):
    """random_metadata plus channels anywhere on the sphere with nothing but a position (the panner's share)"""
    rng = np.random.default_rng(seed + 1)
    mds = ds_model.random_metadata(capi.layout_channels(layout), n - n // 4, seed, bounds=0.5)
    for _ in range(n // 4):
        md = {"azimuth": float(rng.uniform(-180, 180)), "elevation": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))}
        if rng.random() < 0.3:
            md["distance"] = float(rng.uniform(0.2, 2.0))
        mds.append(md)
    order = rng.permutation(len(mds))
    return [mds[i] for i in order]


CASES = [(layout, False) for layout in capi.layout_names()] + [("4+5+0", True), ("9+10+3", True), ("4+9+0", True)]


@pytest.mark.parametrize("layout,moved", CASES, ids=[f"{l}{'-moved' if m else ''}" for l, m in CASES])
def test_batched_fallback_vs_oracle_and_numpy_restatement(layout, moved):
    real = _moved(layout, sum(map(ord, layout))) if moved else None
    ds = capi.DirectSpeakers(ctx(), layout, SUBST, positions=real)
    model = ds_model.Model(capi.layout_channels(layout), SUBST, real)
    mds = _batch(layout, 4096, 17)
    got, gw = ds.calculate(mds)
    assert ds.missed() == 0
    want, ww = model.calculate(mds, ds_model.oracle_psp(layout, real))
    assert np.array_equal(gw, ww)
    assert np.max(np.abs(got - want)) <= 1e-6
    panned = [i for i, md in enumerate(mds) if model.one(md)[0] is None]
    assert len(panned) > 1000  # (the panner's share is real, and in one launch)
    lfe = np.array([c[3] for c in capi.layout_channels(layout)])
    assert not got[panned][:, lfe].any()
    # everything else is exact: one-hot rows, or silence
    rest = np.setdiff1d(np.arange(len(mds)), panned)
    assert np.array_equal(got[rest], want[rest])
    ds.close()


def test_batch_equals_one_at_a_time():
    layout = "9+10+3"
    real = _moved(layout, 3)
    ds = capi.DirectSpeakers(ctx(), layout, SUBST, positions=real)
    mds = _batch(layout, 400, 5)
    batch, bw = ds.calculate(mds)
    for i, md in enumerate(mds):
        g, w = ds.calculate([md])
        assert np.array_equal(g[0], batch[i]) and np.array_equal(w[0], bw[i]), i
    assert ds.missed() == 0
    ds.close()


def test_nominal_positions_given_explicitly_are_the_plain_constructor():
    layout = "4+7+0"
    ch = capi.layout_channels(layout)
    az, el = np.array([c[1] for c in ch]), np.array([c[2] for c in ch])
    a = capi.DirectSpeakers(ctx(), layout)
    b = capi.DirectSpeakers(ctx(), layout, positions=(az, el))
    mds = _batch(layout, 1024, 9)
    assert np.array_equal(a.calculate(mds)[0], b.calculate(mds)[0])
    a.close()
    b.close()


def _run_hip(curves, x, n_out, block, dec, delay, nblocks, strict=False):
    ctx().set_strict(strict)
    try:
        r = capi.Renderer(ctx(), x.shape[0], n_out, block, dec, delay, max_blocks=nblocks)
        for m, (t, d, f) in enumerate(curves):
            r.set_object_points(m, t, d, f if dec is not None else None)
        out = r.process(x)
        r.close()
    finally:
        ctx().set_strict(False)
    return out


def _run_oracle(curves, x, n_out, block, dec, delay):
    if dec is None:  # direct bus only: zero decorrelators, no delay => out == the direct bus exactly
        o = _oracle.ObjectsRenderer(x.shape[0], n_out, block, np.zeros((n_out, 1), np.float32), 0)
    else:
        o = _oracle.ObjectsRenderer(x.shape[0], n_out, block, dec, delay)
    for m, (t, d, f) in enumerate(curves):
        o.set_points(m, 0, t, d)
        o.set_points(m, 1, t, f if dec is not None else np.zeros_like(d))
    return o.process(x)


@pytest.mark.parametrize("out_layout", ["0+5+0", "9+10+3"])
def test_bed_through_the_renderer(out_layout):
    """a 4+7+0 DirectSpeakers bed (labels as URNs, the LFE also marked by its frequency) rendered to out_layout with
    64 ramping objects.  libear's docs: DirectSpeakers gains are applied straight to the channel, one
    LinearInterpVector each (docs/dsp.rst, "Rendering DirectSpeakers") — the renderer's constant curves."""
    bed = capi.layout_channels("4+7+0")
    mds = []
    for name, az, el, is_lfe in bed:
        md = {"speakerLabels": [ds_model.URN0 + name], "azimuth": az, "elevation": el}
        if is_lfe:
            md["lowPass"] = 120.0
        mds.append(md)
    ds = capi.DirectSpeakers(ctx(), out_layout)
    gains, warnings = ds.calculate(mds)
    assert not warnings.any() and ds.missed() == 0
    model = ds_model.Model(capi.layout_channels(out_layout))
    want_gains, _ = model.calculate(mds, ds_model.oracle_psp(out_layout))
    assert np.max(np.abs(gains - want_gains)) <= 1e-6
    ds.close()
    n = gains.shape[1]
    if out_layout == "0+5+0":  # M+090, M+135 and the height layer are panned; the rest go to their namesakes
        assert np.count_nonzero(gains.sum(axis=1) != 1.0) >= 6
    else:  # every bed channel has a namesake
        out_names = [c[0] for c in capi.layout_channels(out_layout)]
        assert [out_names[i] for i in np.argmax(gains, axis=1)] == [c[0] for c in bed]
        assert np.all(gains.max(axis=1) == 1.0) and np.all(np.count_nonzero(gains, axis=1) == 1)

    block, nblocks, n_obj = 512, 4, 64
    dec = capi.design_decorrelators_for_layout(out_layout)
    curves = [(np.zeros(1, np.int64), gains[c:c + 1].copy(), np.zeros((1, n), np.float32)) for c in range(len(bed))]
    curves += scenes.dense_curves(n_obj, n, block, nblocks, seed=33)
    x = scenes.audio(len(curves), block * nblocks, seed=71)
    got = _run_hip(curves, x, n, block, dec, 255, nblocks)
    want = _run_oracle(curves, x, n, block, dec, 255)
    assert scenes.rel_rms_per_channel(got, want) <= 1e-6
    # the bed leg alone, strict: bit for bit the oracle's LinearInterpVector
    k = len(bed)
    got_bed = _run_hip(curves[:k], x[:k], n, block, None, 0, nblocks, strict=True)
    assert np.array_equal(got_bed, _run_oracle(curves[:k], x[:k], n, block, None, 0))
