"""The two references of the render — the CPU oracle's ObjectsRenderer (restated libear components, float32) and the float64
model scenes.render_f64 — against each other on every case of tests/k2_cases.py: compensation delays from 0 to several blocks,
FIRs of 1 tap to two partitions, blocks of 16 to 2048 samples.  No device: the table is well formed, both references take every
case, and the per-sample figure the GPU test (tests/test_gpu_render_delay.py) bounds the kernels by is measured HERE, on the
reference, and committed in the table (k2_cases.ORACLE_PER_SAMPLE)."""
import numpy as np
import pytest

import _oracle
import k2_cases
import scenes
from _hip import set_oracle_curves


def test_the_table_reaches_every_form_on_both_sides_of_the_block():
    """every kernel form and variant of the stage has cases with the delay below, at and above the block size, with no delay
    and with one longer than the first calls of its ragged cutting; every case has its three cuttings and a committed figure"""
    reached = {}
    for c in k2_cases.CASES:
        key = (c.plan["form"], 2 * c.plan["Bk"])
        reached.setdefault(key, set()).add(np.sign(c.D - c.B) if c.D else "none")
        if c.D > 3 * c.B:
            reached[key].add("long")
        assert len(c.cuttings) == 3 and c.cuttings[0] == [c.nblocks] and c.cuttings[1] == [1] * c.nblocks
        assert c.cuttings[2][:3] == [1, 1, 2]
        assert c.plan["NP"] == -(-c.n_taps // c.plan["Bk"])  # (the table's own consistency: written down, checked against its definition)
    want = {(k2_cases.WAVE, 1024), (k2_cases.WG, 1024), (k2_cases.WG, 2048), (k2_cases.WG, 128), (k2_cases.WG, 512),
            (k2_cases.WG, 4096), (k2_cases.RT, 32), (k2_cases.RT, 64), (k2_cases.RT, 960)}
    assert set(reached) == want
    for key, sides in reached.items():
        assert {"none", -1, 1, "long"} <= sides, (key, sides)
    # the delay equal to the block size: every form but the secondary rows
    for key in ((k2_cases.WAVE, 1024), (k2_cases.WG, 1024), (k2_cases.WG, 2048), (k2_cases.WG, 128), (k2_cases.WG, 512),
                (k2_cases.RT, 32), (k2_cases.RT, 960)):
        assert 0 in reached[key], key
    assert set(k2_cases.ORACLE_PER_SAMPLE) == set(k2_cases.BY_ID)


@pytest.mark.parametrize("case", k2_cases.CASES, ids=[c.id for c in k2_cases.CASES])
def test_oracle_against_float64(case):
    """per channel within the project's bound for the fused render, 1e-6 relative RMS; the worst per-sample
    difference over the channel's RMS is the committed one (printed: `K2REF id figure`; three digits are committed, and the oracle
    is compiled without contraction, so the figure repeats: 1 % covers the rounding of the committed number)"""
    curves, x, dec, n = k2_cases.scene(case)
    o = _oracle.ObjectsRenderer(x.shape[0], n, case.B, dec, case.D)
    set_oracle_curves(o, curves)
    want = o.process(x)
    truth = scenes.render_f64(curves, x, n, dec, case.D)
    rel = scenes.rel_rms_per_channel(want, truth)
    worst = k2_cases.per_sample_over_rms(want, truth)
    print(f"K2REF {case.id!r}: {worst:.3g},  # rel rms {rel:.3g}")
    assert np.isfinite(want).all()
    assert rel <= 1e-6
    committed = k2_cases.ORACLE_PER_SAMPLE[case.id]
    assert abs(worst - committed) <= 0.01 * committed, (worst, committed)
