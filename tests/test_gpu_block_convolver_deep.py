"""HIP BlockConvolver beyond four partitions, and the destroy half of groups C and D (tests/conv_cases.py).

earhip_conv_process sums the spectral products in chunks of 16; every chunk after the first reads Y back and adds to it.  The
cases here reach sums of up to 66 products (every count of 15..17, 31..33, 47..49, exact multiples of 16 with and without a
remainder), queues of up to 40 partitions, the tail flush and the blocks where nothing is launched; tests/test_conv_cases_cpu.py
asserts that from the bookkeeping alone.  The reference is the CPU oracle (libear's block_convolver_impl.cpp restated), and
under it the float64 truth of conv_cases.truth.

Measured on an MI355X: against the oracle 2.0e-7 to 3.9e-7 over a case and 4.5e-7 in the worst single block (both one_at_512);
e_gpu 1.5e-7 to 2.4e-7 where e_cpu is 1.8e-7 to 3.4e-7, e_gpu / e_cpu between 0.71 and 0.96 (alternate_P8_B16).  A library
whose chunks after the first overwrite Y instead of adding to it fails 13 of the 17 cases (every one above 16 products, by 0.45
to 0.95 relative) and passes all of tests/test_gpu_block_convolver.py.

The lifetime tests never use a handle after its own close: they test the library's counting (a filter lives as long as a queue
slot points at it, a context refuses to go while anything points at it), not a use after free.
"""
import numpy as np
import pytest

import _oracle
import conv_cases as cc
from _hip import ctx

pytestmark = pytest.mark.gpu


def _capi():
    from libear_amd import capi
    return capi


@pytest.fixture(scope="module")
def oracle_outputs():
    out = {}

    def get(case):
        if case.name not in out:
            ref = cc.run(case, _oracle.ConvCtx(case.block), _oracle.ConvFilter, _oracle.BlockConvolver)
            ref.setflags(write=False)
            out[case.name] = ref
        return out[case.name]
    return get


@pytest.mark.parametrize("case", cc.cases(), ids=repr)
def test_deep_case(case, oracle_outputs):
    capi = _capi()
    got = cc.run(case, capi.ConvCtx(ctx(), case.block), capi.ConvFilter, capi.BlockConvolver)
    ref = oracle_outputs(case)
    want = cc.truth(case)
    e_ref, e_blk = cc.rel(got, ref), cc.worst_block_ratio(got, ref, case.block)
    counts = [k.terms for k in cc.term_counts(case)]
    line = f"{case.name}: B {case.block} P {case.P} terms up to {max(counts)}: against the oracle {e_ref:.3e}, worst block {e_blk:.3e}"
    if want is not None:
        e_gpu, e_cpu = cc.rel(got, want), cc.rel(ref, want)
        line += f", e_gpu {e_gpu:.3e} e_cpu {e_cpu:.3e} ratio {e_gpu / e_cpu:.3f}"
    print(line)
    assert e_ref <= 1e-6
    assert e_blk <= 1e-6
    if want is not None:
        assert e_cpu <= 1e-6
        assert e_gpu <= 1.5 * e_cpu, (e_gpu, e_cpu)  # (the device's passes sum in another order)
        assert e_ref <= e_gpu + e_cpu
    quiet = cc.silent_blocks(case)
    blocks = got.reshape(case.nblk, case.block)
    assert not blocks[quiet].any()
    assert all(blocks[b].any() for b in range(case.nblk) if b not in quiet)


def _blocks(conv, x, B, first, last):
    return np.concatenate([conv.process(x[b * B:(b + 1) * B]) for b in range(first, last)])


def test_zero_tap_filter():
    """a filter of no taps has no partitions: fading to it is fade_down, setting it is unset_filter, bit for bit, and the
    output is zeros once the tail has gone out.  The CPU oracle takes an empty filter too (test_conv_cases_cpu.py), so the
    outputs are also held to it."""
    capi = _capi()
    B, P, at = 32, 9, 4
    nblk = P + 8
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, nblk * B).astype(np.float32)
    ir = rng.uniform(-1, 1, P * B).astype(np.float32) / 8

    def run(how, c, Filter, Convolver):
        empty = Filter(c, np.empty(0, np.float32))
        assert empty.num_blocks() == 0
        conv = Convolver(c, Filter(c, ir), P)
        out = _blocks(conv, x, B, 0, at)
        {"crossfade empty": lambda: conv.crossfade_filter(empty), "fade_down": conv.fade_down,
         "set empty": lambda: conv.set_filter(empty), "unset": conv.unset_filter}[how]()
        return np.concatenate([out, _blocks(conv, x, B, at, nblk)]).reshape(nblk, B)

    c = capi.ConvCtx(ctx(), B)
    got = {how: run(how, c, capi.ConvFilter, capi.BlockConvolver) for how in ("crossfade empty", "fade_down", "set empty", "unset")}
    assert np.array_equal(got["crossfade empty"], got["fade_down"])
    assert np.array_equal(got["set empty"], got["unset"])
    # the fade's last products leave the queue P blocks on, the tail goes out in the call after, then nothing is launched
    assert got["fade_down"][at + P].any() and not got["fade_down"][at + P + 1:].any()
    assert got["unset"][at].any() and not got["unset"][at + 1:].any()
    for how in ("crossfade empty", "set empty"):
        ref = run(how, _oracle.ConvCtx(B), _oracle.ConvFilter, _oracle.BlockConvolver)
        assert cc.rel(got[how], ref) <= 1e-6 and cc.worst_block_ratio(got[how], ref, B) <= 1e-6
        assert np.array_equal(got[how].any(axis=1), ref.any(axis=1))
    with pytest.raises(capi.InvalidArgument):
        capi.BlockConvolver(c, capi.ConvFilter(c, np.empty(0, np.float32)), 0)


def test_two_convolvers_share_a_context_and_filters():
    """P = 9 and P = 17 on one ConvCtx with the same two ConvFilter objects, their process calls interleaved irregularly:
    each output is bit for bit that of the convolver run alone"""
    capi = _capi()
    B, nblk = 32, 40
    rng = np.random.default_rng(11)
    irs = [rng.uniform(-1, 1, n).astype(np.float32) / 8 for n in (9 * B, 8 * B + 1)]
    xs = [rng.uniform(-1, 1, nblk * B).astype(np.float32) for _ in range(2)]
    fades = [{3: 1, 4: 0, 5: 1, 17: 0, 30: 1}, {0: 1, 9: 0, 10: 1, 11: 0, 26: 1, 27: 0}]  # block -> filter, per convolver
    order = rng.permutation([0] * nblk + [1] * nblk)
    assert (np.diff(order) == 0).any() and (np.diff(order) != 0).any()

    def step(conv, which, b, filters, out):
        if b in fades[which]:
            conv.crossfade_filter(filters[fades[which][b]])
        out[b * B:(b + 1) * B] = conv.process(xs[which][b * B:(b + 1) * B])

    solo = []
    for which, P in enumerate((9, 17)):
        c = capi.ConvCtx(ctx(), B)
        filters = [capi.ConvFilter(c, ir) for ir in irs]
        conv = capi.BlockConvolver(c, filters[0], P)
        out = np.zeros(nblk * B, np.float32)
        for b in range(nblk):
            step(conv, which, b, filters, out)
        solo.append(out)
        conv.close()
        for f in filters:
            f.close()
        c.close()

    c = capi.ConvCtx(ctx(), B)
    filters = [capi.ConvFilter(c, ir) for ir in irs]
    convs = [capi.BlockConvolver(c, filters[0], P) for P in (9, 17)]
    outs = [np.zeros(nblk * B, np.float32) for _ in range(2)]
    done = [0, 0]
    for which in order:
        step(convs[which], which, done[which], filters, outs[which])
        done[which] += 1
    for which in range(2):
        assert np.abs(solo[which]).max() > 0.1
        assert np.array_equal(outs[which], solo[which]), which
    for h in convs + filters + [c]:
        h.close()


@pytest.mark.parametrize("drop", ["f after set_filter, g after crossfade_filter", "f after crossfade_filter"])
def test_filter_closed_while_a_queue_holds_it(drop):
    """the creator lets go of a filter that a P = 17 queue still points at: right after set_filter(f), or right after the
    crossfade_filter(g) that starts f fading out.  The blocks after are bit for bit those of a run that kept the handles."""
    capi = _capi()
    B, P, at = 32, 17, 3
    nblk = at + 2 * P
    rng = np.random.default_rng(13)
    x = rng.uniform(-1, 1, nblk * B).astype(np.float32)
    irs = [rng.uniform(-1, 1, n).astype(np.float32) / 8 for n in (P * B, (P - 1) * B + 1)]

    def run(drop):
        c = capi.ConvCtx(ctx(), B)
        f, g = (capi.ConvFilter(c, ir) for ir in irs)
        conv = capi.BlockConvolver(c, None, P)
        conv.set_filter(f)
        if drop.startswith("f after set_filter"):
            f.close()
        out = _blocks(conv, x, B, 0, at)
        conv.crossfade_filter(g)
        if drop.startswith("f after set_filter"):
            g.close()
        elif drop:
            f.close()
        out = np.concatenate([out, _blocks(conv, x, B, at, nblk)])
        # whatever the queue still holds goes with the convolver; then nothing points at the context
        conv.close()
        f.close()
        g.close()
        c.close()
        return out

    kept = run("")
    assert np.abs(kept[-B:]).max() > 0.1
    assert np.array_equal(run(drop), kept)


def test_context_refuses_to_close_while_anything_lives():
    capi = _capi()
    B, P = 32, 17
    rng = np.random.default_rng(17)
    x = rng.uniform(-1, 1, 3 * B).astype(np.float32)
    ir = rng.uniform(-1, 1, P * B).astype(np.float32) / 8
    message = "convolver context still has live filters or convolvers"

    # the twin that nobody tries to take apart
    c0 = capi.ConvCtx(ctx(), B)
    conv0 = capi.BlockConvolver(c0, capi.ConvFilter(c0, ir), P)
    want = [conv0.process(x[:B]), conv0.process(x[B:2 * B])]
    conv0.crossfade_filter(capi.ConvFilter(c0, ir[:5 * B]))
    want.append(conv0.process(x[2 * B:3 * B]))

    c = capi.ConvCtx(ctx(), B)
    f = capi.ConvFilter(c, ir)
    with pytest.raises(capi.InvalidArgument, match=message):  # a filter lives
        c.close()
    assert c.h
    conv = capi.BlockConvolver(c, f, P)
    got = [conv.process(x[:B])]
    f.close()  # (the queue's P + 1 slots keep the filter)
    f.close()
    with pytest.raises(capi.InvalidArgument, match=message):  # a convolver lives, and through it the filter
        c.close()
    got.append(conv.process(x[B:2 * B]))
    g = capi.ConvFilter(c, ir[:5 * B])
    conv.crossfade_filter(g)
    got.append(conv.process(x[2 * B:3 * B]))
    conv.close()
    conv.close()
    with pytest.raises(capi.InvalidArgument, match=message):  # the convolver took the first filter along; g still lives
        c.close()
    # everything is still usable: a new convolver on the same context
    conv = capi.BlockConvolver(c, g, 5)
    assert conv.process(x[:B]).any()
    conv.close()
    g.close()
    c.close()
    c.close()
    assert not c.h and not f.h and not g.h and not conv.h
    assert all(w.any() and np.array_equal(g_, w) for g_, w in zip(got, want))


def test_delay_buffer_close():
    capi = _capi()
    x = np.random.default_rng(19).uniform(-1, 1, (3, 500)).astype(np.float32)
    db = capi.DelayBuffer(ctx(), 3, 100)
    out = db.process(x)
    assert np.array_equal(out[:, 100:], x[:, :400]) and not out[:, :100].any()
    db.close()
    assert not db.h
    db.close()


@pytest.mark.parametrize("nch", [1, 3, 70])
@pytest.mark.parametrize("delay", [0, 1, 1000, 4097])
def test_delay_buffer_edges(delay, nch):
    """delay 0 (the input back, bit for bit), 1, above one workgroup and above 4096; calls of 0 samples, 1, fewer than the
    delay, the delay, one more, and one of 3 delay + 300: the exact shift"""
    capi = _capi()
    sizes = [0, 1] + ([delay - 1] if delay > 1 else []) + [delay, 0, delay + 1, 3 * delay + 300]
    total = sum(sizes)
    x = np.random.default_rng(100 * nch + delay % 97).uniform(-1, 1, (nch, total)).astype(np.float32)
    db = capi.DelayBuffer(ctx(), nch, delay)
    assert db.get_delay() == delay
    out = np.full_like(x, np.nan)
    ofs = 0
    for n in sizes:
        got = db.process(x[:, ofs:ofs + n])
        assert got.shape == (nch, n)
        out[:, ofs:ofs + n] = got
        ofs += n
    db.close()
    want = np.zeros_like(x)
    want[:, delay:] = x[:, :total - delay]
    assert np.array_equal(out, want)
    if delay == 0:
        assert np.array_equal(out, x)
