"""BlockConvolver cases beyond four partitions, for the device (tests/test_gpu_block_convolver_deep.py) and, without one, for
the CPU oracle (tests/test_conv_cases_cpu.py).

A case is a block size B, a partition count P, filters (taps from a seeded default_rng, uniform(-1, 1) / 8), dense input
(uniform(-1, 1)) and a schedule: per block the operations issued before `process` and what `process` is given.

  operations   ("crossfade", i)  ("set", i)  ("fade_down",)  ("unset",)
  input        X: the block of the case's input,  NONE: a null pointer,  ZEROS: an array of zeros

  run(case, ctx, Filter, Convolver)  drives an implementation through the schedule
  truth(case)        float64: per filter the input faded linearly over the block in which the filter enters or leaves,
                     np.convolve, summed (the construction of libear's own test, tests/block_convolver_tests.cpp:83-116).
                     A hard set / unset switches every slot of the filter queue at once, the blocks already in it
                     included, and cannot be written as a fade of the input: a case that uses one after its first block
                     has no truth (truth() is None) and is compared with the oracle only.
  term_counts(case)  the bookkeeping of BlockConvolver::process (src/dsp/block_convolver_impl.cpp:143-237) and nothing else:
                     the filter queue of P + 1 slots, the "is all zero" flags of the two spectra queues and of the tail, the
                     rotation.  Per call: how many products the multiply-accumulate sums, and which way the output goes.
"""
import functools
from collections import namedtuple

import numpy as np

X, NONE, ZEROS = "x", "none", "zeros"
IFFT, TAIL, NOTHING = "inverse transform", "tail flush", "nothing"

# terms: products summed; branch: IFFT / TAIL / NOTHING; tail_zero: the tail's flag when the call began; has_input: the call
# was given a block that is not silent
Call = namedtuple("Call", "terms branch tail_zero has_input")


class Case:
    def __init__(self, name, block, P, taps, schedule, seed):
        """taps: the length of each filter; schedule: [(operations, input)] per block"""
        self.name, self.block, self.P = name, block, P
        self.schedule = [(tuple(ops), inp) for ops, inp in schedule]
        self.nblk = len(self.schedule)
        rng = np.random.default_rng(seed)
        self.irs = [rng.uniform(-1, 1, n).astype(np.float32) / 8 for n in taps]
        self.x = rng.uniform(-1, 1, self.nblk * block).astype(np.float32)
        for b, (_, inp) in enumerate(self.schedule):
            if inp != X:
                self.x[b * block:(b + 1) * block] = 0.0
            else:
                assert self.x[b * block:(b + 1) * block].any()
        assert all(-(-n // block) <= P for n in taps)

    def filter_blocks(self):
        return [-(-len(ir) // self.block) for ir in self.irs]

    def has_truth(self):
        """no hard switch after the first block (see the module's docstring)"""
        return not any(op[0] in ("set", "unset") for ops, _ in self.schedule[1:] for op in ops)

    def __repr__(self):
        return self.name


def run(case, ctx, Filter, Convolver):
    """Filter(ctx, taps); Convolver(ctx, None, P) with set_filter, crossfade_filter, fade_down, unset_filter, process"""
    B = case.block
    filters = [Filter(ctx, ir) for ir in case.irs]
    conv = Convolver(ctx, None, case.P)
    zeros = np.zeros(B, np.float32)
    out = np.zeros_like(case.x)
    for b, (ops, inp) in enumerate(case.schedule):
        for op in ops:
            if op[0] == "crossfade":
                conv.crossfade_filter(filters[op[1]])
            elif op[0] == "set":
                conv.set_filter(filters[op[1]])
            elif op[0] == "fade_down":
                conv.fade_down()
            else:
                assert op[0] == "unset"
                conv.unset_filter()
        sl = slice(b * B, (b + 1) * B)
        out[sl] = conv.process(case.x[sl] if inp == X else None if inp == NONE else zeros)
    return out


@functools.lru_cache(maxsize=None)
def truth(case):
    if not case.has_truth():
        return None
    B, n = case.block, case.nblk * case.block
    # (last, cur): the filter the block's input fades out of and the one it fades into
    pairs, last, cur = [], None, None
    for b, (ops, _) in enumerate(case.schedule):
        for op in ops:
            if op[0] == "crossfade":
                cur = op[1]
            elif op[0] == "fade_down":
                cur = None
            elif op[0] == "set":
                last = cur = op[1]
            else:
                last = cur = None
        pairs.append((last, cur))
        last = cur
    up = np.arange(B, dtype=np.float64) / B
    total = np.zeros(n)
    for i, ir in enumerate(case.irs):
        xf = np.zeros(n)
        for b, (last, cur) in enumerate(pairs):
            sl = slice(b * B, (b + 1) * B)
            if last == i and cur == i:
                xf[sl] = case.x[sl]
            elif cur == i:
                xf[sl] = case.x[sl] * up
            elif last == i:
                xf[sl] = case.x[sl] * (1.0 - up)
        total += np.convolve(xf, ir.astype(np.float64))[:n]
    total.setflags(write=False)
    return total


@functools.lru_cache(maxsize=None)
def term_counts(case):
    P, nb = case.P, case.filter_blocks()
    fq = [None] * (P + 1)
    f_ofs = s_ofs = 0
    old_zero, new_zero, tail_zero = [True] * P, [True] * P, True
    calls = []

    def slot(i):
        return (f_ofs + i) % (P + 1)

    for ops, inp in case.schedule:
        for op in ops:
            if op[0] in ("crossfade", "fade_down"):
                fq[slot(0)] = op[1] if op[0] == "crossfade" else None
            else:
                fq = [op[1] if op[0] == "set" else None] * (P + 1)
        i0 = s_ofs % P
        if inp != X:  # :156-159
            old_zero[i0] = new_zero[i0] = True
        else:  # :162-187
            new_zero[i0] = False
            old_zero[i0] = fq[slot(1)] == fq[slot(0)]
        terms = 0
        for i in range(P):  # :195-209
            fo, fn, s = fq[slot(i + 1)], fq[slot(i)], (s_ofs + i) % P
            terms += fo is not None and i < nb[fo] and not old_zero[s]
            terms += fn is not None and i < nb[fn] and not new_zero[s]
        if terms:  # :217-234
            calls.append(Call(terms, IFFT, tail_zero, inp == X))
            tail_zero = False
        elif not tail_zero:
            calls.append(Call(0, TAIL, False, inp == X))
            tail_zero = True
        else:
            calls.append(Call(0, NOTHING, True, inp == X))
        s_ofs = (s_ofs + P - 1) % P  # :114-122
        f_ofs = (f_ofs + P) % (P + 1)
        fq[slot(0)] = fq[slot(1)]
    return tuple(calls)


def silent_blocks(case):
    """the blocks that the bookkeeping says are not computed at all: the output is zeros"""
    return [b for b, c in enumerate(term_counts(case)) if c.branch == NOTHING]


def _alternate(nblk, fade_first):
    """two filters crossfaded every block; the first block hears filter 0 alone, or is already a fade into filter 1"""
    sched = [([("set", 0)] + ([("crossfade", 1)] if fade_first else []), X)]
    cur = 1 if fade_first else 0
    for _ in range(1, nblk):
        cur ^= 1
        sched.append(([("crossfade", cur)], X))
    return sched


def _steady(P):
    return Case(f"steady_P{P}", 32, P, [P * 32], [([("set", 0)], X)] + [((), X)] * (P + 7), 1000 + P)


def _alternate_case(P, B, fade_first, name=None, nblk=None):
    return Case(name or f"alternate_P{P}_B{B}", B, P, [P * B, (P - 1) * B + 1], _alternate(nblk or 2 * P + 8, fade_first),
                2000 + P)


def _sliding_silence():
    """`alternate` at P = 20; once the queue is full, runs of 4 silent blocks (a null pointer and an array of zeros in turn)
    one input block apart take the count from 40 down to 8, across 32 and 16, and P + 4 blocks of input take it back up"""
    P, B = 20, 32
    kinds = [X] * (P + 2)
    for _ in range(4):
        kinds += [NONE, ZEROS, NONE, ZEROS, X]
    kinds += [X] * (P + 4)
    sched = [(ops, k) for (ops, _), k in zip(_alternate(len(kinds), True), kinds)]
    return Case("sliding_silence", B, P, [P * B, (P - 1) * B + 1], sched, 3000)


def _drain_and_resume():
    P, B = 17, 32
    sched = [([("set", 0)], X)] + [((), X)] * (P + 2)
    sched += [((), NONE if k % 2 == 0 else ZEROS) for k in range(P + 4)]
    sched += [((), X)] * (P + 3)
    return Case("drain_and_resume", B, P, [P * B], sched, 4000)


def _mixed_lengths():
    """filters of 3, 20 and 11 blocks in a queue of 20, crossfaded in turn every 7 blocks: `i < nblocks` cuts the terms"""
    P, B, nblk = 20, 32, 3 * 20 + 8
    sched = [([("set", 0)], X)]
    for b in range(1, nblk):
        sched.append(([("crossfade", (b // 7) % 3)] if b % 7 == 0 else [], X))
    return Case("mixed_lengths", B, P, [3 * B, 20 * B, 10 * B + 5], sched, 5000)


def _hard_switches():
    """set / unset / fade_down in the middle of a deep queue.  No truth: a hard switch also changes the filter that the
    blocks already in the queue are multiplied with, which no fade of the input expresses — oracle only."""
    P, B = 17, 32
    at = {0: [("set", 0)], 6: [("crossfade", 1)], 20: [("set", 2)], 27: [("fade_down",)], 31: [("crossfade", 0)],
          40: [("unset",)], 43: [("set", 1), ("crossfade", 2)], 50: [("unset",)], 51: [("set", 0)]}
    quiet = {12: NONE, 13: ZEROS, 45: NONE}
    sched = [(at.get(b, []), quiet.get(b, X)) for b in range(3 * P + 8)]
    return Case("hard_switches", B, P, [P * B, 9 * B - 3, 16 * B + 1], sched, 6000)


@functools.lru_cache(maxsize=None)
def cases():
    out = [_steady(P) for P in (8, 9, 16, 17, 32, 33, 40)]
    # block sizes spread over the depths: L = 32 and 90 take the run-time transforms (90 mixed radix), 64 and 128 their own
    out += [_alternate_case(8, 16, True), _alternate_case(9, 45, False), _alternate_case(16, 64, False),
            _alternate_case(17, 32, True), _alternate_case(33, 45, False)]
    out += [_sliding_silence(), _drain_and_resume(), _mixed_lengths(), _hard_switches()]
    # the only case at a workload's size; its first block is a fade already, so its counts are the even numbers up to 2 P
    out.append(_alternate_case(33, 512, True, name="one_at_512", nblk=2 * 33 + 6))
    return tuple(out)


def rel(a, b):
    """||a - b|| / ||b||"""
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def worst_block_ratio(got, ref, block):
    """max over blocks of ||got_b - ref_b|| / max(||ref_b||, 1e-3 max_b ||ref_b||): one wrong block is not averaged away"""
    g = np.asarray(got, np.float64).reshape(-1, block)
    r = np.asarray(ref, np.float64).reshape(-1, block)
    norms = np.linalg.norm(r, axis=1)
    return float((np.linalg.norm(g - r, axis=1) / np.maximum(norms, 1e-3 * norms.max())).max())
