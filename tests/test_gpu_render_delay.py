"""The decorrelator stage (K2) off its default operating point: every case of tests/k2_cases.py — compensation delays from 0 to
more than three blocks, FIRs of 1 tap to two partitions, blocks of 16 to 2048 samples, runs of 1 and 3 blocks — on the kernel
form the case was written for (earhip_render_last_decor_plan, asserted), under every cutting of the stream into calls.

  a. against the CPU oracle, per channel, and per sample against a float64 render;
  b. the delay line alone, bit for bit: with every diffuse gain zero a render with delay D is the render with delay 0 moved back
     by D samples; in strict mode the cutting does not change a bit either;
  c. state that outlives several calls (delay line, history and tails of two partitions): a reset after the second call gives
     a fresh renderer's bits;
  d. the device entry point with padded rows: the host entry point's bits, nothing written beside the rows.
"""
import numpy as np
import pytest

import k2_cases
import scenes
from _hip import ctx, set_renderer_curves, with_options
from test_gpu_render import run_hip, run_oracle

pytestmark = pytest.mark.gpu

CASE_IDS = [c.id for c in k2_cases.CASES]
# Per-sample error over the channel's RMS against float64: no value can be derived for it, so the kernels are held to the
# oracle's own figure (tests/test_render_delay_cpu.py, committed per case in the table): four times the largest of the table —
# block pairing and transform sizes differ between the oracle and each kernel form.
PER_SAMPLE_BOUND = 4.0 * max(k2_cases.ORACLE_PER_SAMPLE.values())

_refs = {}


def references(case):
    """(the oracle's render, the float64 render) of a case, made once"""
    if case.id not in _refs:
        curves, x, dec, n = k2_cases.scene(case)
        want = run_oracle(curves, x, n, case.B, dec, case.D)
        truth = scenes.render_f64(curves, x, n, dec, case.D)
        want.setflags(write=False)
        truth.setflags(write=False)
        _refs[case.id] = (want, truth)
    return _refs[case.id]


def render(case, cut, delay=None, zero_diffuse=False):
    """the case's stream through the host entry point under one cutting -> (outputs, the decorrelator plan of the last call)"""
    from libear_amd import capi
    curves, x, dec, n = k2_cases.scene(case, zero_diffuse)

    def go():
        r = capi.Renderer(ctx(), x.shape[0], n, case.B, dec, case.D if delay is None else delay, max_blocks=max(cut))
        try:
            set_renderer_curves(r, curves, True)
            out = np.zeros((n, x.shape[1]), np.float32)
            ofs = 0
            for nb in cut:
                k = nb * case.B
                out[:, ofs:ofs + k] = r.process(x[:, ofs:ofs + k])
                ofs += k
            return out, r.last_decor_plan()
        finally:
            r.close()

    return with_options(case.opts, go)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_every_case_and_cutting_against_the_oracle(cid):
    """a. relative RMS per channel within the project's 1e-6 of the oracle; per sample over the channel's RMS against float64
    within four times the oracle's own worst figure; on the kernel form, partition size and count and run length of the table"""
    case = k2_cases.BY_ID[cid]
    want, truth = references(case)
    for cut in case.cuttings:
        got, plan = render(case, cut)
        rel = scenes.rel_rms_per_channel(got, want)
        worst = k2_cases.per_sample_over_rms(got, truth)
        print(f"K2GPU {cid} form {plan['form']} L {2 * plan['Bk']} cut {len(cut)} rel {rel:.3g} per-sample {worst:.3g}")
        assert plan == case.plan, (plan, case.plan)
        assert np.isfinite(got).all()
        assert rel <= 1e-6, (cut, rel)
        assert worst <= PER_SAMPLE_BOUND, (cut, worst, PER_SAMPLE_BOUND)


_undelayed = {}


def undelayed(case, cut, strict):
    """the case's render with zero diffuse gains and NO delay under a cutting (made once per scene, options and cutting)"""
    key = (case.B, case.nblocks, case.n_taps, case.layout, tuple(sorted(case.opts.items())), tuple(cut), strict)
    if key not in _undelayed:
        curves, x, dec, n = k2_cases.scene(case, True)
        out = with_options(case.opts, lambda: run_hip(curves, x, n, case.B, dec, 0, cut, strict=strict))
        out.setflags(write=False)
        _undelayed[key] = out
    return _undelayed[key]


@pytest.mark.parametrize("cid", [c.id for c in k2_cases.CASES if c.D > 0])
def test_the_delay_line_alone_bit_for_bit(cid):
    """b. two buses, decorrelators present, every diffuse gain zero: the decorrelated signal is exactly zero and the output is
    the direct bus delayed.  Under one cutting the renders with delay D and with delay 0 have the same calls, so the same gain
    plans and the same direct-bus bits: the first D samples are zero, the rest is the undelayed render moved back by D.  In
    strict mode the direct bus does not depend on the cutting: all cuttings give the same bits.  No tolerance."""
    case = k2_cases.BY_ID[cid]
    curves, x, dec, n = k2_cases.scene(case, True)
    D, total = case.D, x.shape[1]
    strict_outs = []
    for cut in case.cuttings:
        got, plan = render(case, cut, zero_diffuse=True)
        assert plan == case.plan, (plan, case.plan)
        ref = undelayed(case, cut, False)
        assert np.any(ref)
        assert not np.any(got[:, :D]), cut
        assert np.array_equal(got[:, D:], ref[:, :total - D]), cut
        strict_outs.append(with_options(case.opts, lambda: run_hip(curves, x, n, case.B, dec, D, cut, strict=True)))
    ref = undelayed(case, case.cuttings[0], True)
    for cut, got in zip(case.cuttings, strict_outs):
        assert not np.any(got[:, :D]), cut
        assert np.array_equal(got[:, D:], ref[:, :total - D]), cut


STATE_IDS = [c.id for c in k2_cases.CASES if c.group == "taps" and c.n_taps == 2 * c.B]


@pytest.mark.parametrize("cid", STATE_IDS)
def test_reset_after_state_that_outlived_two_calls(cid):
    """c. FIRs of 2 B taps (two partitions: history and a tail per partition) and a delay of 2 B + 3 under the ragged cutting
    [1, 1, 2, ...]: the first calls are shorter than the delay and than the history, so each writes its state partly from the state
    it read, and the double buffers alternate.  A reset behind the second call makes the rest of the stream a fresh renderer's,
    bit for bit — and not what the stream gives when the state carries on."""
    from libear_amd import capi
    case = k2_cases.BY_ID[cid]
    assert case.D == 2 * case.B + 3 and case.plan["NP"] == 2
    curves, x, dec, n = k2_cases.scene(case)
    cut = case.cuttings[2]
    B = case.B

    def stream(r, calls, ofs):
        outs = []
        for nb in calls:
            outs.append(r.process(x[:, ofs:ofs + nb * B]))
            ofs += nb * B
        return np.concatenate(outs, axis=1)

    def go():
        r = capi.Renderer(ctx(), x.shape[0], n, B, dec, case.D, max_blocks=max(cut))
        fresh = capi.Renderer(ctx(), x.shape[0], n, B, dec, case.D, max_blocks=max(cut))
        try:
            set_renderer_curves(r, curves, True)
            set_renderer_curves(fresh, curves, True)
            head = stream(r, cut[:2], 0)
            r.reset(2 * B)
            tail = stream(r, cut[2:], 2 * B)
            plan = r.last_decor_plan()
            fresh.reset(2 * B)
            tail_fresh = stream(fresh, cut[2:], 2 * B)
        finally:
            r.close()
            fresh.close()
        return head, tail, tail_fresh, plan

    head, tail, tail_fresh, plan = with_options(case.opts, go)
    carried, _ = render(case, cut)
    assert plan == case.plan, (plan, case.plan)
    assert np.isfinite(tail).all() and np.any(tail)
    assert np.array_equal(head, carried[:, :2 * B])
    assert np.array_equal(tail, tail_fresh)
    assert not np.array_equal(tail, carried[:, 2 * B:])


DEVICE_IDS = ["wave-512-d513", "wave-1024-d1025", "wg1024-k2wg-d513", "wg2048-own-d1025", "wg128-d65", "wg512-d257", "rt16-d17",
              "rt480-d481", "taps-b512-t1024"]


@pytest.mark.parametrize("cid", DEVICE_IDS)
def test_device_entry_point_with_padded_rows(cid):
    """d. earhip_render_process_device from torch buffers whose rows are total + 4 floats apart, under the ragged cutting: the
    values are the host entry point's for the same cutting, bit for bit; the four columns behind every output row and the input
    buffer, its padding included, are as they were"""
    import torch
    from libear_amd import capi
    case = k2_cases.BY_ID[cid]
    curves, x, dec, n = k2_cases.scene(case)
    cut = case.cuttings[2]
    m, total = x.shape
    stride = total + 4
    host, plan_host = render(case, cut)

    def go():
        c = ctx()
        xin = torch.full((m, stride), -3.25, dtype=torch.float32)
        xin[:, :total] = torch.from_numpy(np.array(x))
        xdev = xin.cuda()
        out = torch.full((n, stride), 7.5, dtype=torch.float32, device="cuda")
        r = capi.Renderer(c, m, n, case.B, dec, case.D, max_blocks=max(cut))
        try:
            set_renderer_curves(r, curves, True)
            ofs = 0
            for nb in cut:
                r.process_device(nb, xdev.data_ptr() + 4 * ofs, stride, out.data_ptr() + 4 * ofs, stride)
                ofs += nb * case.B
            c.synchronize()
            plan = r.last_decor_plan()
        finally:
            r.close()
        return out.cpu().numpy(), xdev.cpu().numpy(), xin.numpy(), plan

    got, x_after, x_before, plan = with_options(case.opts, go)
    assert plan == case.plan and plan_host == case.plan, (plan, plan_host, case.plan)
    assert np.all(got[:, total:] == 7.5)
    assert np.array_equal(x_after, x_before)
    assert np.array_equal(got[:, :total], host)
