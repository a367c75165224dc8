"""Every gain kernel above 1024 objects against libear (the CPU oracle) and a float64 evaluation, at the object counts where
plan_mix or a list builder changes what it does: tests/many_objects_cases.py has the cases and, written down from the
planner's rules, the plan each must run; tests/test_many_objects_cpu.py the references' own figures.

Bars, for every case but the roll call (want: the oracle's render; truth: float64; e_lib = rel_rms_per_channel(want, truth),
e_gpu = rel_rms_per_channel(got, truth)):
  1. the plan of the call — kernel, tile, tiles, object splits across workgroups, list layout — is the one written down, and a
     hinge call was not handed to the lists standing by;
  2. every sample finite;
  3. e_gpu <= max(1.25 e_lib, 1e-6): the device is no further from exact arithmetic than libear's own float path (the bar of
     test_render_fast_kernels_against_libear).  1e-6 against the oracle cannot be asked for up here: the oracle itself is
     1.7e-6 from float64 at 8193 objects and 4.7e-6 at 65537 (6.2e-7 at 1024);
  4. against the oracle: 1e-6 per channel up to 1024 objects; above, max(1e-6, bar 3 + e_lib) — bar 3 and the triangle
     inequality, a consistency bound;
  5. every sample within 1e-5 of its channel's largest magnitude of the oracle's (tests/test_gpu_gain_ref.py) — or, where the
     oracle's own worst sample is more than a quarter of that from float64, within 4 times the oracle's worst.  Measured on the
     CPU (test_many_objects_cpu.py): the oracle's worst sample is 1.3e-6 .. 2.3e-6 of the channel's peak at 1536 and 2048
     objects, 2.0e-6 .. 3.1e-6 at 4096 / 4097, 2.9e-6 .. 4.9e-6 at 8192 / 8193 and 8.8e-6 at 65536 / 65537 (1.1e-6 at 1024):
     the scaled bound is in force from about 4096 objects on.
The roll call (family `integer`): np.array_equal with the int64 answer, on every kernel and with every summation order.
Strict mode: kernel 0, bit for bit the oracle's.

The figures of every case are printed; the last test prints the worst per group, kernel and object count."""
import numpy as np
import pytest

import _oracle
import many_objects_cases as mc
import scenes
from _hip import ctx, with_options

pytestmark = pytest.mark.gpu

WORST = {}  # (group, kernel, M) -> [e_gpu, e_lib, distance from the oracle, worst sample / bound]


def render(case, opts=None):
    """one call of the whole scene, from device memory (a call from host memory of more than 16 MB of inputs — 4097 objects x
    1024 samples — runs as a pipeline of shorter calls, host_gather.h: not the plan under test) -> (output, what the call ran)"""
    import torch
    from libear_amd import capi
    s, N, total = mc.scene(case), mc.n_out(case), case.block * case.nblocks

    def run():
        r = capi.Renderer(ctx(), case.M, N, case.block, s.dec, s.delay, max_blocks=case.nblocks)
        try:
            for m, (t, d, f) in enumerate(s.curves):
                r.set_object_points(m, t, d, f if case.buses == 2 else None)
            xd = torch.from_numpy(s.x.copy()).cuda()
            yd = torch.full((N, total), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            r.process_device(case.nblocks, xd.data_ptr(), total, yd.data_ptr(), total)
            ctx().synchronize()
            got = yd.cpu().numpy()
            ran = dict(r.last_plan(), layout=r.last_list_layout())
            assert ran["kernel"] == r.gain_kernel()
            ran["standby"] = r.hinge_standby() if ran["kernel"] == mc.HINGE else False
        finally:
            r.close()
        return got, ran
    return with_options(case.opts if opts is None else opts, run)


def check_plan(case, ran):
    assert {k: ran[k] for k in case.plan} == case.plan, (case.id, ran)
    assert not ran["standby"], (case.id, ran)


def check_bars(case, got, ran):
    s = mc.scene(case)
    assert np.isfinite(got).all(), case.id
    if case.family == "integer":
        bad = np.argwhere(got != s.answer)
        assert np.array_equal(got, s.answer), (case.id, ran, len(bad), bad[:6], [(got[c, i], s.answer[c, i]) for c, i in bad[:6]])
        return
    e_lib, e_gpu = scenes.rel_rms_per_channel(s.want, s.truth), scenes.rel_rms_per_channel(got, s.truth)
    d_cpu = scenes.rel_rms_per_channel(got, s.want)
    bar3 = max(1.25 * e_lib, 1e-6)
    bar4 = 1e-6 if case.M <= 1024 else max(1e-6, bar3 + e_lib)
    per_sample = max(1e-5, 4.0 * mc.per_sample(s.want, s.truth))
    worst = mc.per_sample(got, s.want)
    print(f"{case.id}: kernel {ran['kernel']} tile {ran['tile']} x {ran['ntiles']} gsplit {ran['gsplit']}: e_gpu {e_gpu:.3g} e_lib {e_lib:.3g} "
          f"from the oracle {d_cpu:.3g} (bar {bar4:.3g}) worst sample {worst:.3g} (bar {per_sample:.3g})")
    w = WORST.setdefault((case.group, ran["kernel"], case.M), [0.0, 0.0, 0.0, 0.0])
    w[:] = [max(a, b) for a, b in zip(w, (e_gpu, e_lib, d_cpu, worst))]
    assert e_gpu <= bar3, (case.id, e_gpu, e_lib, ran)
    assert d_cpu <= bar4, (case.id, d_cpu, bar4, ran)
    assert worst <= per_sample, (case.id, worst, per_sample, ran)


@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.id)
def test_gain_kernels_above_1024_objects(case):
    got, ran = render(case)
    check_plan(case, ran)
    check_bars(case, got, ran)


@pytest.mark.parametrize("M", sorted(mc.BUILDER))
def test_hinge_list_builder_forms(M):
    """the hinge kernel's list builder with 1, 2, 4, 8 tiles per workgroup (up to 128 KB of dynamic LDS: 16 bytes per object
    and tile) and as two kernels: the lists are the same bit for bit, so the outputs are"""
    case = mc.builder_case(M)
    first = None
    for form in mc.BUILDER[M]:
        got, ran = render(case, dict(case.opts, **form))
        check_plan(case, ran)
        if first is None:
            first = got
            check_bars(case, got, ran)
        assert np.array_equal(got, first), (M, form, scenes.rel_rms_per_channel(got, first))


@pytest.mark.parametrize("family,M,layout,block,nb", mc.STRICT, ids=lambda v: str(v))
def test_strict_mode_bit_exact(family, M, layout, block, nb):
    """strict mode through the renderer and through earhip_gain_interp: libear's own arithmetic, bit for bit the oracle's"""
    from libear_amd import capi
    case = mc.strict_case(family, M, layout, block, nb)
    N, total = mc.n_out(case), block * nb
    ctx().set_strict(True)
    try:
        got, ran = render(case)
        check_plan(case, ran)
        assert got.dtype == np.float32 and np.array_equal(got, mc.scene(case).want), (case.id, scenes.rel_rms_per_channel(got, mc.scene(case).want))
        times, vals = mc.matrix_points(family, M, N, case.seed)
        x = mc.scene(case).x
        want = _oracle.gain_interp("matrix", times, vals, x, [total])
        gi = capi.GainInterp(ctx(), M, N)
        try:
            gi.set_points(times, vals)
            out = gi.process(0, x)
        finally:
            gi.close()
        assert out.dtype == np.float32 and np.array_equal(out, want), (case.id, scenes.rel_rms_per_channel(out, want))
        if family == "integer":
            assert np.array_equal(got, mc.scene(case).answer)
    finally:
        ctx().set_strict(False)


def test_measured_table():
    """prints what the tests above measured (nothing to assert: the bars are theirs)"""
    print("group kernel M | worst e_gpu, e_lib, distance from the oracle, sample")
    for (group, kernel, M), w in sorted(WORST.items()):
        print(f"{group} {kernel} {M} | {w[0]:.3g} {w[1]:.3g} {w[2]:.3g} {w[3]:.3g}")
