"""The device extent panner (k_pan_objects_extent) against libear's DOUBLE core (the oracle's PolarExtent.handle(which=1)) at the
edges of its chunk culling: the case table of tests/extent_cases.py, where the groups, the claims and the bar are written down.

The bar is measured against the reference, never against the device: per group and layout e_lib, the worst distance of
libear's float core from its double core over the group's positions, is computed in the same run (extent_cases.reference,
cached), and the device's worst distance from the double core is held to F x e_lib (F = 1.5).  Group 5 has no float core of its
own (its reference is tests/extent_model.py on a defined layout): there e_lib is that of 4+5+0 over the same positions.

Measured on an MI355X (e_gpu / e_lib, ratio): see NOTES.md, "The extent panner's edges"."""
import numpy as np
import pytest

import _oracle
import custom_layout_model as model
import extent_cases as ec
import extent_model
from _hip import ctx

pytestmark = pytest.mark.gpu


def device(layout, v, real, positions=None):
    """capi.Panner.calculate with gain 1 and diffuse 0 -> the direct rows' loudspeaker columns; the LFE columns and the diffuse
    rows are exactly 0"""
    from libear_amd import capi
    p = capi.Panner(ctx(), layout, positions)
    try:
        d, f = p.calculate(v["az"], v["el"], v["dist"], None, None, v["width"], v["height"], v["depth"])
    finally:
        p.close()
    lfe = [c for c in range(d.shape[1]) if c not in real]
    assert lfe or layout == "0+2+0"
    assert not d[:, lfe].any() and not f.any() and np.isfinite(d).all()
    return d[:, real]


def hold(label, got, ref, v):
    e = ec.rel(got, ref.want)
    at = int(e.argmax())
    print(f"{label}: e_gpu {e.max():.3e} e_lib {ref.e_lib:.3e} ratio {e.max() / ref.e_lib:.3f} over {len(e)} positions, worst at "
          f"az {v['az'][at]:g} el {v['el'][at]:.9g} dist {v['dist'][at]:g} width {v['width'][at]:.9g} height {v['height'][at]:.9g} "
          f"depth {v['depth'][at]:g}")
    assert ref.e_lib <= ec.E_LIB_MAX
    assert e.max() <= ec.F * ref.e_lib


@pytest.mark.parametrize("group,layout", [(g, name) for g in (1, 2, 3, 4) for name in ec.layouts_of(g)])
def test_group_against_the_double_core(group, layout):
    v = ec.columns(ec.cases(group))
    got = device(layout, v, ec.real_columns(layout))
    hold(f"group {group} {layout}", got, ec.reference(group, layout), v)


def test_wide_layout_against_the_model():
    """group 5: 32 channels, 22 loudspeakers, LFE channels inside the list"""
    from libear_amd import capi
    capi.define_layout("wide 22", ec.WIDE)
    c = ec.wide_positions()
    v = ec.columns((c,))
    real = [i for i, ch in enumerate(ec.WIDE) if not ch[3]]
    assert len(real) == 22 and real != list(range(22)) and real[-1] == 31
    got = device("wide 22", v, real)
    assert got.shape == (64, 22)
    panner = model.Panner(ec.WIDE)
    want = extent_model.PolarExtent(lambda p: panner.pan(p)[0]).handle(_oracle.cart(c.az, c.el, c.dist), c.width, c.height, c.depth)
    e_lib = ec.references("4+5+0", v).e_lib
    hold("group 5 wide 22", got, ec.Reference(want, e_lib, 0), v)
    # what the device takes no wider: 30 loudspeakers
    with pytest.raises(capi.EarHipError) as info:
        capi.define_layout("wide 30", ec.TOO_WIDE)
    assert info.value.code == capi.NOT_IMPLEMENTED


@pytest.mark.parametrize("layout", ec.EDGE_LAYOUTS)
def test_small_calls(layout):
    """group 6 (a): calls of 1, 3, 5, 127 and 129 positions, every other one with nothing to spread"""
    calls = [ec.small_call(n) for n in ec.CALL_SIZES]
    real = ec.real_columns(layout)
    got = np.concatenate([device(layout, ec.columns((c,)), real) for c in calls])
    v = ec.columns(calls)
    hold(f"group 6a {layout}", got, ec.references(layout, v), v)


def test_second_batch():
    """group 6 (b): 2^18 + 5 positions in one call are two batches of launch_objects; the rows around the boundary equal, bit for
    bit, a call of their own; 300 rows, those among them, meet the reference; no position was missed"""
    from libear_amd import capi
    layout = "0+5+0"
    c = ec.large_call()
    v = ec.columns((c,))
    n = len(c.az)
    assert n == ec.BATCH + 5
    lo = ec.BATCH - 64
    p = capi.Panner(ctx(), layout)
    try:
        d, f = p.calculate(v["az"], v["el"], v["dist"], None, None, v["width"], v["height"], v["depth"])
        assert p.missed() == 0
        d2, f2 = p.calculate(*(v[k][lo:] for k in ("az", "el", "dist")), None, None, *(v[k][lo:] for k in ("width", "height", "depth")))
        assert p.missed() == 0
    finally:
        p.close()
    assert d2.shape == (69, d.shape[1])
    assert np.array_equal(d[lo:], d2) and np.array_equal(f[lo:], f2) and not f.any()
    assert np.isfinite(d).all() and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 1e-5
    rng = np.random.default_rng(67)
    idx = np.r_[np.arange(lo, n), rng.choice(lo, 300 - (n - lo), replace=False)]
    real = ec.real_columns(layout)
    assert not np.delete(d, real, axis=1).any()
    vs = {k: a[idx] for k, a in v.items()}
    hold("group 6b 0+5+0", d[idx][:, real], ec.references(layout, vs), vs)
