"""DirectSpeakers with Cartesian positions and screenEdgeLock (earhip group X) on the GPU: the channels that fall through, polar
ones at their (locked) position and Cartesian ones at the position the BS.2127 section 10 conversion gives, go to the device
panner in one launch per call.

  * batches of 2048 mixed polar, Cartesian and locked channels on three BS.2051 layouts and on 4+9+0 with moved loudspeakers,
    behind a default-sized reproduction screen off centre, against tests/ds_cart_model.py (a numpy restatement of the header
    comment) whose panner is the pinned oracle panner: 1e-6, the bar of tests/test_gpu_direct_speakers.py;
  * a batch equals its channels computed one at a time;
  * the 7.1.2 bed of an Atmos-style master as stepped tracks (Renderer.set_objects_blocks) beside 16 Cartesian objects from the
    allocentric panner, rendered to 4+7+0 and compared per channel with the CPU oracle renderer on the same rows (relative RMS
    <= 1e-6); the bed alone, in strict mode, is bit-exact.
"""
import numpy as np
import pytest

import _oracle
import ds_cart_model
import ds_model
import scenes
import timeline_model
from _hip import ctx
from libear_amd import capi
from ds_cart_model import SCREEN, atmos_bed, c_screen

pytestmark = pytest.mark.gpu

SUBST = {"foo": "M+030"}


def moved(layout, seed):
    return ds_cart_model.moved(capi.layout_channels(layout), seed)


CASES = [("0+5+0", False), ("4+7+0", False), ("9+10+3", False), ("4+9+0", True)]


@pytest.mark.parametrize("layout,move", CASES, ids=[f"{l}{'-moved' if m else ''}" for l, m in CASES])
def test_mixed_batch_vs_oracle_panner_and_numpy_restatement(layout, move):
    real = moved(layout, sum(map(ord, layout))) if move else None
    ds = capi.DirectSpeakers(ctx(), layout, SUBST, positions=real)
    model = ds_cart_model.Model(capi.layout_channels(layout), SUBST, real, SCREEN)
    mds = ds_cart_model.random_metadata(model, 2048, 17, cartesian=0.5, lock=0.3)
    got, gw = ds.calculate_screen(mds, c_screen(SCREEN))
    assert ds.missed() == 0
    want, ww, panned = model.calculate_screen(mds, ds_model.oracle_psp(layout, real))
    assert np.array_equal(gw, ww)
    err = float(np.max(np.abs(got - want)))
    print(f"{layout}: max |gain - model| = {err:.3g}, {len(panned)} of {len(mds)} panned")
    assert err <= 1e-6
    assert len(panned) > len(mds) // 4
    assert sum("X" in mds[i] for i in panned) > 100 and sum("screenEdgeLock" in mds[i] for i in panned) > 100
    lfe = np.array([c[3] for c in capi.layout_channels(layout)])
    assert not got[panned][:, lfe].any()
    assert np.allclose(np.sum(got[panned].astype(np.float64) ** 2, axis=1), 1.0, atol=1e-5)  # (the panner normalises)
    # everything else is exact: one-hot rows, or silence
    rest = np.setdiff1d(np.arange(len(mds)), panned)
    assert np.array_equal(got[rest], want[rest])
    ds.close()


def test_batch_equals_one_at_a_time():
    layout = "9+10+3"
    real = moved(layout, 3)
    ds = capi.DirectSpeakers(ctx(), layout, SUBST, positions=real)
    model = ds_cart_model.Model(capi.layout_channels(layout), SUBST, real, SCREEN)
    mds = ds_cart_model.random_metadata(model, 400, 5, cartesian=0.5, lock=0.3)
    screen = c_screen(SCREEN)
    batch, bw = ds.calculate_screen(mds, screen)
    for i, md in enumerate(mds):
        g, w = ds.calculate_screen([md], screen)
        assert np.array_equal(g[0], batch[i]) and np.array_equal(w[0], bw[i]), i
    assert ds.missed() == 0
    ds.close()


def _oracle_render(curves, x, n_out, block, dec, delay):
    if dec is None:  # direct bus only: zero decorrelators, no delay => out == the direct bus exactly
        o = _oracle.ObjectsRenderer(x.shape[0], n_out, block, np.zeros((n_out, 1), np.float32), 0)
    else:
        o = _oracle.ObjectsRenderer(x.shape[0], n_out, block, dec, delay)
    for m, (t, d, f) in enumerate(curves):
        o.set_points(m, 0, t, d)
        o.set_points(m, 1, t, f)
    return o.process(x)


def test_atmos_bed_and_cartesian_objects_through_the_renderer():
    out_layout = "4+7+0"
    ch = capi.layout_channels(out_layout)
    n = len(ch)
    block, nblocks, n_obj = 512, 4, 16
    bed = atmos_bed()
    ds = capi.DirectSpeakers(ctx(), out_layout)
    bed_rows, warnings = ds.calculate_screen(bed)
    assert ds.missed() == 0
    model = ds_cart_model.Model(ch)
    want_rows, ww, panned = model.calculate_screen(bed, ds_model.oracle_psp(out_layout))
    assert np.array_equal(warnings, ww) and np.max(np.abs(bed_rows - want_rows)) <= 1e-6
    ds.close()
    # the front three and the LFE have a loudspeaker of their own.  The section 10 conversion puts the side pair at azimuth
    # +-70 and the rear pair at +-110, where 4+7+0 (M+-090, M+-135) has none, so those and the top pair are panned
    names = [c[0] for c in ch]
    got_names = [names[int(np.argmax(g))] if np.count_nonzero(g) == 1 else None for g in bed_rows]
    assert got_names == ["M+030", "M-030", "M+000", "LFE1"] + [None] * 6
    assert panned == [4, 5, 6, 7, 8, 9]
    assert np.allclose(np.sum(bed_rows.astype(np.float64) ** 2, axis=1), 1.0, atol=1e-5)

    # tracks: the bed as stepped tracks of one open-ended block, 16 Cartesian objects of three ramping blocks each
    rng = np.random.default_rng(29)
    tracks = [(c, capi.TIMELINE_STEPPED, 0, [(0, -1, 0, -1)]) for c in range(len(bed))]
    for k in range(n_obj):
        tracks.append((len(bed) + k, capi.TIMELINE_INTERPOLATED, int(rng.integers(-100, 100)),
                       [(0, 700, 0, -1), (700, 600, 1, int(rng.integers(0, 400))), (1300, -1, 1, 300)]))
    offsets = np.cumsum([0] + [len(t[3]) for t in tracks])
    n_cart = int(offsets[-1] - len(bed))
    allo = capi.Allo(out_layout)
    xyz = rng.uniform(-1.0, 1.0, (3, n_cart))
    obj_direct, obj_diffuse = allo.calculate_objects(*xyz, width=rng.uniform(0.0, 0.5, n_cart), diffuse=rng.uniform(0.0, 1.0, n_cart))
    allo.close()
    direct = np.concatenate([bed_rows, obj_direct]).astype(np.float32)
    diffuse = np.concatenate([np.zeros_like(bed_rows), obj_diffuse]).astype(np.float32)

    def bind(r, sel):
        r.set_objects_blocks([tracks[k][0] for k in sel], [tracks[k][1] for k in sel], [tracks[k][2] for k in sel],
                             np.cumsum([0] + [len(tracks[k][3]) for k in sel]), [b for k in sel for b in tracks[k][3]],
                             np.concatenate([direct[offsets[k]:offsets[k + 1]] for k in sel]),
                             np.concatenate([diffuse[offsets[k]:offsets[k + 1]] for k in sel]) if r.K == 2 else None)

    def curves(sel):
        out = []
        for k in sel:
            pts = timeline_model.points(tracks[k][1], tracks[k][2], tracks[k][3], timeline_model.INT64_MIN, timeline_model.INT64_MAX)
            zero = np.zeros(n, np.float32)
            out.append((np.array([t for t, _ in pts], np.int64),
                        np.array([direct[offsets[k] + s] if s >= 0 else zero for _, s in pts], np.float32),
                        np.array([diffuse[offsets[k] + s] if s >= 0 else zero for _, s in pts], np.float32)))
        return out

    everything = list(range(len(tracks)))
    x = scenes.audio(len(tracks), block * nblocks, seed=71)
    dec = capi.design_decorrelators_for_layout(out_layout)
    r = capi.Renderer(ctx(), len(tracks), n, block, dec, 255, max_blocks=nblocks)
    bind(r, everything)
    r.commit()
    got = r.process(x)
    r.close()
    want = _oracle_render(curves(everything), x, n, block, dec, 255)
    err = float(scenes.rel_rms_per_channel(got, want))
    print(f"bed and objects: relative RMS per channel <= {err:.3g}")
    assert err <= 1e-6
    # the bed leg alone, strict: bit for bit the oracle's LinearInterpVector
    k = len(bed)
    ctx().set_strict(True)
    try:
        r = capi.Renderer(ctx(), k, n, block, None, 0, max_blocks=nblocks)
        bind(r, list(range(k)))
        r.commit()
        got_bed = r.process(x[:k])
        r.close()
    finally:
        ctx().set_strict(False)
    assert np.array_equal(got_bed, _oracle_render(curves(range(k)), x[:k], n, block, None, 0))
    assert np.abs(got_bed).max() > 0.1
