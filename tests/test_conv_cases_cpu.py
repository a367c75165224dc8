"""The deep BlockConvolver cases without a device (tests/conv_cases.py):
  * the bookkeeping model says the cases reach what they were written for: multiply-accumulate sums of 15, 16, 17, 31, 32, 33,
    47, 48, 49 and of at least 64 products (the device sums them in chunks of 16), a non-empty exact multiple of 16 with input
    present, and in `drain_and_resume` each of the three output branches, the inverse transform once more after the tail was
    marked zero;
  * the CPU oracle is within 1e-6 (relative L2) of the float64 truth wherever a case has one, before it is the device's reference;
  * where the model says nothing is computed, the oracle's block is zeros — the model and the oracle keep the same books.

Measured (x86-64): the oracle against the truth is between 1.8e-7 (alternate_P8_B16) and 3.4e-7 (one_at_512), 2.7e-7 at most
below block 512; the largest count is 66 (alternate_P33_B45 and one_at_512); the oracle takes an empty filter (no partitions)
and treats it as no filter."""
import numpy as np
import pytest

import _oracle
import conv_cases as cc


@pytest.fixture(scope="module")
def oracle_outputs():
    out = {c.name: cc.run(c, _oracle.ConvCtx(c.block), _oracle.ConvFilter, _oracle.BlockConvolver) for c in cc.cases()}
    for v in out.values():
        v.setflags(write=False)
    return out


def test_case_set_reaches_the_chunk_boundaries():
    by_name = {c.name: c for c in cc.cases()}
    assert len(by_name) == len(cc.cases())
    reached = set()
    for c in cc.cases():
        calls = cc.term_counts(c)
        assert len(calls) == c.nblk and c.P + 8 <= c.nblk <= 3 * c.P + 10, c  # (the cases stay short)
        counts = {k.terms for k in calls}
        print(f"{c.name}: B {c.block} P {c.P} blocks {c.nblk} filters {c.filter_blocks()} counts {min(counts)}..{max(counts)} "
              f"branches {sorted({k.branch for k in calls})} truth {c.has_truth()}")
        reached |= counts
    assert {15, 16, 17, 31, 32, 33, 47, 48, 49} <= reached and max(reached) >= 64
    assert any(k.terms > 0 and k.terms % 16 == 0 and k.has_input for c in cc.cases() for k in cc.term_counts(c))
    # steady: every count from 1 to P, as the queue fills
    for P in (8, 9, 16, 17, 32, 33, 40):
        assert [k.terms for k in cc.term_counts(by_name[f"steady_P{P}"])][:P] == list(range(1, P + 1))
    # alternate: about 2 P
    for c in cc.cases():
        if c.name.startswith("alternate") or c.name == "one_at_512":
            assert max(k.terms for k in cc.term_counts(c)) == 2 * c.P
    # sliding_silence: down across 32 and 16 and back up
    t = [k.terms for k in cc.term_counts(by_name["sliding_silence"])]
    full = t.index(40)
    low = full + int(np.argmin(t[full:]))
    print("sliding_silence:", t)
    assert t[low] < 16 and t[-1] == 40 and {16, 32} <= set(t[full:low]) and {16, 32} <= set(t[low:])
    kinds = {inp for _, inp in by_name["sliding_silence"].schedule}
    assert kinds == {cc.X, cc.NONE, cc.ZEROS}
    # mixed_lengths: the short filters cut terms that a full queue would have
    t = [k.terms for k in cc.term_counts(by_name["mixed_lengths"])]
    print("mixed_lengths:", t)
    assert min(t[20:]) < 20 and len(set(t[20:])) > 5
    # only hard_switches is without a truth
    assert [c.name for c in cc.cases() if not c.has_truth()] == ["hard_switches"]
    assert {cc.IFFT, cc.TAIL, cc.NOTHING} == {k.branch for k in cc.term_counts(by_name["hard_switches"])}


def test_drain_and_resume_takes_every_branch():
    case = next(c for c in cc.cases() if c.name == "drain_and_resume")
    calls = cc.term_counts(case)
    P = case.P
    branches = [k.branch for k in calls]
    # input, the queue drains over P silent blocks, one tail flush, four blocks of nothing, input again
    assert branches == [cc.IFFT] * (2 * P + 2) + [cc.TAIL] + [cc.NOTHING] * 4 + [cc.IFFT] * (P + 3)
    assert [k.terms for k in calls[P + 3:2 * P + 3]] == list(range(P - 1, -1, -1))
    resume = calls[2 * P + 7]
    assert resume.branch == cc.IFFT and resume.tail_zero and resume.has_input and resume.terms == 1
    assert sum(k.branch == cc.IFFT and k.tail_zero for k in calls) == 2  # (the very first block is the other)
    assert cc.silent_blocks(case) == list(range(2 * P + 3, 2 * P + 7))


@pytest.mark.parametrize("case", cc.cases(), ids=repr)
def test_oracle_is_close_to_the_truth(case, oracle_outputs):
    want = cc.truth(case)
    if want is None:
        assert not case.has_truth()
        return
    e_cpu = cc.rel(oracle_outputs[case.name], want)
    print(f"{case.name}: oracle against the float64 truth {e_cpu:.3e}")
    assert 0.0 < e_cpu <= 1e-6


@pytest.mark.parametrize("case", cc.cases(), ids=repr)
def test_model_predicts_silence_exactly(case, oracle_outputs):
    got = oracle_outputs[case.name].reshape(case.nblk, case.block)
    quiet = cc.silent_blocks(case)
    assert not got[quiet].any()
    # and nowhere else: a block that was computed is not all zeros
    assert all(got[b].any() for b in range(case.nblk) if b not in quiet)


def test_oracle_takes_an_empty_filter():
    """a filter of zero taps has no partitions (block_convolver_impl.cpp:21-36 loops zero times); fading to it is
    fade_down, setting it is unset_filter, bit for bit"""
    B, P = 32, 9
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, (P + 8) * B).astype(np.float32)
    ir = rng.uniform(-1, 1, P * B).astype(np.float32) / 8
    outs = {}
    for how in ("crossfade empty", "fade_down", "set empty", "unset"):
        c = _oracle.ConvCtx(B)
        empty = _oracle.ConvFilter(c, np.empty(0, np.float32))
        assert empty.num_blocks() == 0
        conv = _oracle.BlockConvolver(c, _oracle.ConvFilter(c, ir), P)
        out = np.zeros_like(x)
        for b in range(P + 8):
            if b == 4:
                {"crossfade empty": lambda: conv.crossfade_filter(empty), "fade_down": conv.fade_down,
                 "set empty": lambda: conv.set_filter(empty), "unset": conv.unset_filter}[how]()
            out[b * B:(b + 1) * B] = conv.process(x[b * B:(b + 1) * B])
        outs[how] = out.reshape(-1, B)
    assert np.array_equal(outs["crossfade empty"], outs["fade_down"]) and np.array_equal(outs["set empty"], outs["unset"])
    assert outs["fade_down"][4 + P].any() and not outs["fade_down"][4 + P + 1:].any()
    assert outs["unset"][4].any() and not outs["unset"][5:].any()
