"""The rare paths of every gain kernel against the CPU oracle: tests/rare_path_cases.py has the cases, the scene of each, the
options it runs under and the plan and form it must run; tests/test_rare_paths_cpu.py holds the scenes to what they claim (bursts
and non-finite samples unprobed, what overflows and what does not, the oracle's own distance from float64).

Every render asserts what it ran — last_plan()'s kernel, tile and gsplit, last_list_layout(), wide_form() — so that no case passes
on another kernel or form than the one its id names.  The bar, unless a test says otherwise: every sample finite and
scenes.rel_rms_per_channel(got, oracle) <= 1e-6, the project's bar for these kernels up to 1024 objects.  The figures of every case
are printed; the last test prints the worst per group, kernel and form."""
import numpy as np
import pytest

import rare_path_cases as rc
import scenes
from _hip import set_renderer_curves, with_options

pytestmark = pytest.mark.gpu

BAR = 1e-6
WORST = {}  # (group, kernel, form) -> worst distance from the oracle
FORM = {"wide": True, "plain": False, "none": None}
PAD = 256   # floats of sentinel in front of and behind a device buffer's rows (a multiple of 4: the rows' alignment is the test's)
SENT_IN, SENT_OUT = np.float32(-3.25), np.float32(7.5)


def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def in_context(opts, fn, strict=False):
    """fn(context) on a fresh context made under `opts` (the kernel choice and GSPLIT are read when a context and a renderer are made)"""
    from libear_amd import capi

    def run():
        c = capi.Context(0)
        try:
            c.set_strict(strict)
            return fn(c)
        finally:
            c.close()
    return with_options(opts, run)


def check_ran(case, r, gsplit, form=None):
    """the plan and the form of the renderer's last call are the case's (form: of this render, where a case has several)"""
    plan, layout, wide = r.last_plan(), r.last_list_layout(), r.wide_form()
    ran = dict(plan, layout=layout, wide=wide)
    assert plan["kernel"] == case.kernel and r.gain_kernel() == case.kernel and plan["tile"] == case.tile, (case.id, ran)
    if gsplit is None:
        assert plan["gsplit"] > 1, (case.id, ran)
    else:
        assert plan["gsplit"] == gsplit, (case.id, ran)
    assert layout == case.paired, (case.id, ran)
    assert wide is FORM[form or case.form], (case.id, ran)
    if case.kernel == rc.HINGE:  # (the packed-f16 kink products' form, not handed to the lists standing by)
        assert not r.hinge_standby() and not r.hinge_robust(), (case.id, ran)
    return ran


def note(case, err, form=None):
    key = (case.group, rc.KNAME[case.kernel], form or case.form)
    WORST[key] = max(WORST.get(key, 0.0), err)


def held_to_the_oracle(case, got, want, ran, what="", form=None):
    err = scenes.rel_rms_per_channel(got, want)
    print(f"{case.id}{what}: {ran}: from the oracle {err:.3g}")
    note(case, err, form)
    assert np.isfinite(got).all(), (case.id, what)
    assert err <= BAR, (case.id, what, err, ran)
    return err


# ---- groups B and E: the long scenes, from device memory -----------------------------------------------------------------------------
_device_inputs = {}


def device_inputs(bursts):
    """the long scene's inputs on the device, uploaded once ([128][cus * 512] floats: 64 MB on an MI355X)"""
    import torch
    key = (compute_units(), bursts)
    if key not in _device_inputs:
        _device_inputs[key] = torch.from_numpy(np.array(rc.long_inputs(compute_units(), bursts))).cuda()
        torch.cuda.synchronize()
    return _device_inputs[key]


def render_long(c, r, xd, calls, n, block=512):
    """the renderer from time 0 over `calls` (blocks each) of the long scene's device rows -> the output [n][total]"""
    import torch
    total = sum(calls) * block
    yd = torch.full((n, total), float(SENT_OUT), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.reset(0)
    ofs = 0
    for nb in calls:
        r.process_device(nb, xd.data_ptr() + 4 * ofs, xd.shape[1], yd.data_ptr() + 4 * ofs, total)
        ofs += nb * block
    c.synchronize()
    return yd.cpu().numpy()


def long_renderer(c, scene, n, max_blocks, buses):
    from libear_amd import capi
    r = capi.Renderer(c, rc.M, n, scene.block, scene.dec, scene.delay, max_blocks=max_blocks)
    set_renderer_curves(r, scene.curves, buses == 2)
    return r


@pytest.mark.parametrize("case", rc.BY_GROUP["B"], ids=lambda c: c.id)
def test_redo_in_calls_that_pick_their_form_on_the_device(case):
    """Group B.  128 objects on 9+10+3 and on 0+5+0, two buses, as many blocks of 512 as make `compute units` tiles: with the objects split over
    two workgroups that is the shortest call whose form the device picks — the plain form, every object at one level.  Bursts 10^4
    above the level in eight tiles (rare_path_cases.long_bursts): the waves that hold one redo their share of the tile's list, and
    part 0 the objects of the tile's exact-path list (the three busiest objects are on it in every tile), between a pipeline
    carried in from the tile before and the requests for the tile behind.  Piece lists: P2_WGS 1, 3, 8 give the bits of a
    workgroup per tile (0) — on 0+5+0 (one column tile) at both tile sizes; on 9+10+3 (three column tiles) only the 512-sample
    tiles carry a pipeline, the 4-wave kernel keeps a workgroup per tile there and its four launches are the same one
    (rare_path_cases.carried; tests/test_rare_paths_cpu.py asserts that a carrying case exists per tile size, layout and form); GSPLIT = 1 runs the wide form (one round of workgroups).  The `cut` cases render the scene in blocks of
    128, once as one call (plain form) and once cut in two behind block 149 — sample 19072, a multiple of neither tile size; both
    calls are shorter than two rounds of workgroups: the wide form, and a ragged last tile — each held to the oracle's render in
    blocks of 128: the level and mode words alternate between calls, behind a call that overflowed."""
    cus = compute_units()
    kind, bursts = case.scene
    cut = case.extra["calls"] == "cut"
    block = rc.LONG["cut_block"] if cut else rc.LONG["block"]
    scene = rc.long_scene(kind, cus, bursts, case.buses, None, block, case.layout)
    n = scene.want.shape[0]
    total = rc.long_blocks(case.tile, cus) * 512
    nblocks = total // block
    cuttings = [("plain", [nblocks]), ("wide", [rc.LONG["cut"], nblocks - rc.LONG["cut"]])] if cut else [(case.form, [nblocks])]
    want = scene.want[:, :total]
    quiet = rc.burst_mask(total, rc.long_bursts(cus), 512, 1024)
    xd = device_inputs(True)

    def run(c):
        r = long_renderer(c, scene, n, nblocks, case.buses)
        outs = {}
        try:
            for form, calls in cuttings:
                for wgs in (rc.P2_WGS if case.kernel == rc.PIECES else (None,)):
                    c.set_option("P2_WGS", wgs)
                    got = render_long(c, r, xd, calls, n, block)
                    ran = check_ran(case, r, case.extra["gsplit"], form)
                    assert ran["ntiles"] == -(-calls[-1] * block // case.tile), (case.id, ran)
                    # the form is the device's choice exactly where the call is two rounds of workgroups or more (api_core.hip:117)
                    assert (ran["ntiles"] * ran["gsplit"] >= 2 * cus) == (form == "plain"), (case.id, ran, cus)
                    outs[(form, wgs)] = (got, ran)
        finally:
            r.close()
        return outs

    outs = in_context(case.opts, run)
    first = rc.P2_WGS[0] if case.kernel == rc.PIECES else None
    for form, calls in cuttings:
        got, ran = outs[(form, first)]
        held_to_the_oracle(case, got, want, ran, f" calls {calls} ({form})", form)
        e_quiet = scenes.rel_rms_per_channel(got[:, quiet], want[:, quiet])
        print(f"{case.id} calls {calls}: over the samples no burst reaches {e_quiet:.3g}")
        assert e_quiet <= BAR, (case.id, calls, e_quiet)
        for (f, wgs), (other, _) in outs.items():  # (every P2_WGS of a cutting: the bits of a workgroup per tile)
            if f == form:
                assert np.array_equal(other, got), (case.id, form, wgs, float(np.abs(other - got).max()))


@pytest.mark.parametrize("case", rc.BY_GROUP["E"], ids=lambda c: c.id)
def test_non_finite_input_stays_in_its_tile_in_the_list_kernels(case):
    """Group E.  The long scene without bursts on one bus (no decorrelator, no delay: an output sample depends on the inputs of its
    own instant alone), its first `compute units` 256-sample tiles (piece lists: P2_WGS 1 and 8 carry the pipeline through a
    workgroup's tiles, the launch's own count is a workgroup per tile at this length); one inf in an ordinary object, then one NaN in a busy one, at
    an unprobed sample of an interior tile.  Outside the workgroup tile that holds it every output is finite, within the bar of
    the oracle, and bit for bit the render of the same inputs with a zero in its place; at the sample itself every channel the
    oracle makes non-finite is."""
    cus = compute_units()
    kind, _ = case.scene
    nblocks = rc.long_blocks(256, cus)
    total = nblocks * 512
    scene = rc.long_scene(kind, cus, False, 1, nblocks)
    n = scene.want.shape[0]
    clean = device_inputs(False)

    def run(c):
        r = long_renderer(c, scene, n, nblocks, 1)
        outs = {}
        try:
            for what, obj in rc.NON_FINITE:
                s = rc.non_finite_sample(obj, cus)
                for value in (what, "zero"):
                    xd = clean.clone()
                    xd[obj, s] = {"inf": float("inf"), "nan": float("nan"), "zero": 0.0}[value]
                    outs[(what, value)] = render_long(c, r, xd, [nblocks], n)
                    ran = check_ran(case, r, case.extra["gsplit"])
                    assert (ran["ntiles"] * ran["gsplit"] >= 2 * cus) == (case.form == "plain"), (case.id, ran, cus)
        finally:
            r.close()
        return outs, ran

    outs, ran = in_context(case.opts, run)
    for what, obj in rc.NON_FINITE:
        s = rc.non_finite_sample(obj, cus)
        t0 = s // case.tile * case.tile
        outside = np.ones(total, bool)
        outside[t0:t0 + case.tile] = False
        got, zero = outs[(what, what)], outs[(what, "zero")]
        held_to_the_oracle(case, got[:, outside], scene.want[:, outside], ran, f" {what} in object {obj} at {s}, outside its tile")
        held_to_the_oracle(case, zero[:, outside], scene.want[:, outside], ran, f" zero in object {obj} at {s}")
        assert np.array_equal(got[:, outside], zero[:, outside]), (case.id, what, int((got[:, outside] != zero[:, outside]).sum()))
        # the oracle on the block of the sample
        b0 = s // 512 * 512
        x = np.array(scene.x[:, b0:b0 + 512])
        x[obj, s - b0] = np.inf if what == "inf" else np.nan
        _, _, at = rc._oracle_render(scenes.window_curves(scene.curves, b0, b0 + 512), x, n, 512, 1, case.layout)
        bad = ~np.isfinite(at[:, s - b0])
        assert bad.any() and not np.isfinite(got[bad, s]).any(), (case.id, what, at[:, s - b0], got[:, s])


# ---- group C: a fixed input scale ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.BY_GROUP["C"], ids=lambda c: c.id)
def test_fixed_input_scale(case):
    """Group C.  EARHIP_XSCALE = k: no probe, the launch's scale 2^k, the wide form.  Full-scale inputs (uniform in +-1): at 2^7
    nothing leaves the f16 range, at 2^16 some 64-sample wave spans do and others do not (both paths in one call), at 2^18 every
    span does — the whole call is the redo's output."""
    from libear_amd import capi
    scene = rc.small_scene(*case.scene)
    n = scene.want.shape[0]

    def run(c):
        r = capi.Renderer(c, rc.M, n, scene.block, scene.dec, scene.delay, max_blocks=scene.total // scene.block)
        try:
            set_renderer_curves(r, [(t + scene.start, d, f) for t, d, f in scene.curves], True)
            r.reset(scene.start)
            got = r.process(scene.x)
            assert c.get_option("XSCALE") == case.extra["k"]
            return got, check_ran(case, r, case.extra["gsplit"])
        finally:
            r.close()

    got, ran = in_context(case.opts, run)
    held_to_the_oracle(case, got, scene.want, ran)


# ---- group D: rows that are not vectors ----------------------------------------------------------------------------------------------
def _rows(buf, off, stride, nrows, total):
    return buf[PAD + off:PAD + off + nrows * stride].reshape(nrows, stride)[:, :total]


@pytest.mark.parametrize("case", rc.BY_GROUP["D"], ids=lambda c: c.id)
def test_rows_that_are_not_vectors(case):
    """Group D.  GainMixParams::vec_ok == 0 on every kernel kind, from device buffers filled with a sentinel, the call starting at
    sample 37: output rows total + 1 floats apart; output rows 4 bytes off a 16-byte boundary; input rows total + 1 floats apart on
    two buses (the kernel writes aligned bus slabs, its objects split over parts); input rows 4 bytes off.  Every float of the
    output buffer outside the rows' samples keeps the sentinel — in front of the first row, between rows, behind the last — and the
    input buffer is what was uploaded, bit for bit.  Strict mode: the oracle's bits."""
    import torch
    from libear_amd import capi
    scene = rc.small_scene(*case.scene)
    n, total, way = scene.want.shape[0], scene.total, case.extra["way"]
    istride, ioff = {"istride": (total + 1, 0), "ibase": (total + 4, 1)}.get(way, (total, 0))
    ostride, ooff = {"ostride": (total + 1, 0), "obase": (total + 4, 1)}.get(way, (total + 4, 0))
    hin = np.full(2 * PAD + ioff + rc.M * istride, SENT_IN, np.float32)
    _rows(hin, ioff, istride, rc.M, total)[:] = scene.x
    hout = np.full(2 * PAD + ooff + n * ostride, SENT_OUT, np.float32)

    def run(c):
        r = capi.Renderer(c, rc.M, n, scene.block, scene.dec, scene.delay, max_blocks=total // scene.block)
        try:
            set_renderer_curves(r, [(t + scene.start, d, f) for t, d, f in scene.curves], case.buses == 2)
            r.reset(scene.start)
            xd, yd = torch.from_numpy(hin).cuda(), torch.from_numpy(hout).cuda()
            torch.cuda.synchronize()
            ip, op = xd.data_ptr() + 4 * (PAD + ioff), yd.data_ptr() + 4 * (PAD + ooff)
            # (the rows are unaligned the way the case says, and only that way)
            assert (xd.data_ptr() % 16, yd.data_ptr() % 16) == (0, 0)
            assert (ip % 16 != 0) == (way == "ibase") and (op % 16 != 0) == (way == "obase")
            assert (istride % 4 != 0) == (way == "istride") and (ostride % 4 != 0) == (way == "ostride")
            r.process_device(total // scene.block, ip, istride, op, ostride)
            c.synchronize()
            return yd.cpu().numpy(), xd.cpu().numpy(), check_ran(case, r, case.extra["gsplit"])
        finally:
            r.close()

    out, xin, ran = in_context(case.opts, run, strict=case.extra["strict"])
    got = _rows(out, ooff, ostride, n, total)
    held_to_the_oracle(case, got, scene.want, ran)
    if case.extra["strict"]:
        assert got.dtype == np.float32 and np.array_equal(got, scene.want), (case.id, ran)
    untouched = np.ones(out.shape, bool)
    _rows(untouched, ooff, ostride, n, total)[:] = False
    assert np.all(out[untouched] == SENT_OUT), (case.id, np.flatnonzero(untouched & (out != SENT_OUT))[:8] - PAD - ooff)
    assert np.array_equal(xin.view(np.uint32), hin.view(np.uint32)), case.id


def test_measured_table():
    """prints what the tests above measured (nothing to assert: the bars are theirs)"""
    print("group kernel form | worst distance from the oracle")
    for (group, kernel, form), w in sorted(WORST.items()):
        print(f"{group} {kernel} {form} | {w:.3g}")
