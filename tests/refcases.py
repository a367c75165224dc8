"""Shared test scenarios restated from the reference's own test-suite so that the CPU oracle and
the HIP path are driven through exactly the same cases.

* convolution scenarios: reference tests/block_convolver_tests.cpp:197-356 (15 cases) with the
  brute-force oracle of :83-116 and tests/block_convolver_test_utils.cpp:31-60.
* The inputs are sparse random impulses like the reference's generate_random
  (block_convolver_test_utils.cpp:12-23); that helper draws from libstdc++'s
  implementation-defined std::uniform_*_distribution, so the values are regenerated here from
  numpy's PCG64 (the expected outputs come from the brute-force convolution, not from stored
  reference outputs, so the exact impulse values do not matter).
"""
import numpy as np


def generate_random(length, num_nonzero, seed):
    rng = np.random.default_rng(1000 + seed)
    data = np.zeros(length, np.float32)
    for _ in range(num_nonzero):
        data[rng.integers(0, length)] = np.float32(rng.uniform())
    return data


def fade_up(x):
    n = len(x)
    a = (np.arange(n, dtype=np.float32) * np.float32(1.0 / n)).astype(np.float32)
    return (a * x).astype(np.float32)


def fade_down(x):
    n = len(x)
    a = (np.arange(n, dtype=np.float32) * np.float32(1.0 / n)).astype(np.float32)
    return ((np.float32(1) - a) * x).astype(np.float32)


class ConvScenario:
    """One reference ConvolutionTest (block_convolver_tests.cpp:29-195)."""

    def __init__(self, name, num_blocks, irs, initial_ir, ir_for_block, input_nonzero, block_size=512,
                 max_num_blocks=0, null_for_zeros=False, constructor="no_filter", zero_range=None):
        self.name = name
        self.block_size = block_size
        self.num_blocks = num_blocks
        self.len = block_size * num_blocks
        self.irs = [generate_random(n, nz, seed) for (n, nz, seed) in irs]
        self.initial_ir = initial_ir
        self.ir_for_block = ir_for_block
        self.max_num_blocks = max_num_blocks
        self.null_for_zeros = null_for_zeros
        self.constructor = constructor
        self.input = generate_random(self.len, input_nonzero, 0)
        if zero_range is not None:
            self.input[zero_range[0]:zero_range[0] + zero_range[1]] = 0.0

    def expected(self):
        """Brute-force: per IR, fade the input per block, convolve, mix (:83-116)."""
        B = self.block_size
        total = np.zeros(self.len, np.float64)
        for i, ir in enumerate(self.irs):
            x = np.zeros(self.len, np.float32)
            for b in range(self.num_blocks):
                sl = slice(b * B, (b + 1) * B)
                last = i == (self.initial_ir if b == 0 else self.ir_for_block[b - 1])
                this = i == self.ir_for_block[b]
                if last and this:
                    x[sl] = self.input[sl]
                elif this:
                    x[sl] = fade_up(self.input[sl])
                elif last:
                    x[sl] = fade_down(self.input[sl])
            total += np.convolve(x.astype(np.float64), ir.astype(np.float64))[:self.len]
        return total

    def run(self, ctx, Filter, Convolver):
        """Drive an implementation (:119-177).  Filter(ctx, taps); Convolver(ctx, filt, num_blocks)."""
        B = self.block_size
        filters = [Filter(ctx, ir) for ir in self.irs]
        max_blocks = max([self.max_num_blocks] + [f.num_blocks() for f in filters])
        if self.constructor == "no_filter":
            conv = Convolver(ctx, None, max_blocks)
        elif self.constructor == "with_filter_num_blocks":
            conv = Convolver(ctx, filters[self.initial_ir], max_blocks)
        else:
            conv = Convolver(ctx, filters[self.initial_ir], 0)
        if self.initial_ir >= 0:
            conv.set_filter(filters[self.initial_ir])
        out = np.zeros(self.len, np.float32)
        for b in range(self.num_blocks):
            sl = slice(b * B, (b + 1) * B)
            this = self.ir_for_block[b]
            last = self.initial_ir if b == 0 else self.ir_for_block[b - 1]
            if last != this:
                if this >= 0:
                    conv.crossfade_filter(filters[this])
                else:
                    conv.fade_down()
            if self.null_for_zeros and not np.any(self.input[sl]):
                out[sl] = conv.process(None)
            else:
                out[sl] = conv.process(self.input[sl])
        return out


def conv_scenarios():
    S = ConvScenario
    return [
        S("single_block", 1, [(100, 10, 1)], 0, [0], 200),
        S("two_blocks", 2, [(512 * 3, 20, 1)], 0, [0, 0], 300),
        S("fade_once", 3, [(100, 10, 1), (512, 10, 2)], 0, [0, 1, 1], 300),
        S("fade_at_start_from_silence", 2, [(512, 10, 1)], -1, [0, 0], 300),
        S("fade_to_silence", 3, [(512, 10, 1)], 0, [0, -1, -1], 300),
        S("fade_from_silence", 3, [(512, 10, 1)], -1, [-1, 0, 0], 300),
        S("fade_at_start_from_filter", 2, [(512, 10, 1), (512, 10, 2)], 0, [1, 1], 300),
        S("smaller_filter_than_convolver", 4, [(512 * 2, 20, 1)], 0, [0, 0, 0, 0], 300, max_num_blocks=3),
        S("different_num_blocks", 4, [(512 * 2, 20, 1), (512 * 3, 20, 2)], 0, [0, 1, 1, 1], 300),
        S("zero_input_blocks", 5, [(512 * 2, 20, 1)], 0, [0] * 5, 300, zero_range=(512, 512 * 3)),
        S("null_input_blocks", 5, [(512 * 2, 20, 1)], 0, [0] * 5, 300, zero_range=(512, 512 * 3),
          null_for_zeros=True),
        S("lots_of_filters", 9, [(512 * 2, 20, 1), (512 * 3, 20, 2), (512, 20, 3), (512 * 4, 20, 4)], 0,
          [0, 1, 2, 3, 3, 2, 2, 1, 0], 500),
        S("construct_with_filter", 3, [(512 * 2, 20, 1)], 0, [0, 0, 0], 300,
          constructor="with_filter_num_blocks"),
        S("construct_with_filter_no_blocks", 3, [(512 * 2, 20, 1)], 0, [0, 0, 0], 300,
          constructor="with_filter_no_num_blocks"),
    ]


# ---- GainInterpolator cases (reference tests/gain_interpolator_tests.cpp:58-257) ----------------

def single_interp_expected(x, t0, start, end, sp, ep):
    """Closed form used by the reference test :58-70 (float64 evaluation)."""
    t = t0 + np.arange(len(x))
    p = (t - start) / float(end - start)
    return (ep * p + (1.0 - p) * sp) * x.astype(np.float64)


def gain_interp_cases():
    """(name, points [(time, value)], length, expected segments [(a, b, kind, args)])."""
    return [
        ("basic", [(100, 0.2), (200, 0.8), (300, 0.8), (400, 0.3)], 500,
         [(0, 100, "const", 0.2), (100, 200, "ramp", (100, 200, 0.2, 0.8)), (200, 300, "const", 0.8),
          (300, 400, "ramp", (300, 400, 0.8, 0.3)), (400, 500, "const", 0.3)], [50, 75, 100, 500]),
        ("step", [(100, 0.2), (200, 0.2), (200, 0.8), (300, 0.8)], 400,
         [(0, 200, "const", 0.2), (200, 400, "const", 0.8)], [50, 75, 100, 400]),
        ("only_step", [(100, 0.2), (100, 0.8)], 200,
         [(0, 100, "const", 0.2), (100, 200, "const", 0.8)], [50, 75, 100, 200]),
        ("one_point", [(100, 0.2)], 200, [(0, 200, "const", 0.2)], [50, 75, 100, 200]),
    ]


def expected_single(x, segments):
    out = np.zeros(len(x), np.float64)
    for a, b, kind, args in segments:
        if kind == "const":
            out[a:b] = np.float64(np.float32(args)) * x[a:b]
        else:
            start, end, sp, ep = args
            out[a:b] = single_interp_expected(x[a:b], a, start, end, np.float64(np.float32(sp)),
                                              np.float64(np.float32(ep)))
    return out


def chunks(total, size):
    out = []
    while total > 0:
        n = min(size, total)
        out.append(n)
        total -= n
    return out


def is_approx(a, b, prec=1e-5):
    """Eigen::isApprox for float: ||a-b|| <= prec * min(||a||, ||b||) (reference tests/eigen_utils.hpp)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) <= prec * min(np.linalg.norm(a), np.linalg.norm(b))


def interp_golden():
    """(the generator module tests/golden/make_interp_golden.py — case definitions and readers —, its cases: the inputs
    it builds, checked against the digests in tests/golden/gain_interp_ref.npz, with libear's outputs from that file)"""
    import importlib.util
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_interp_golden", os.path.join(here, "make_interp_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.load()
