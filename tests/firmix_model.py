"""The FIR filter matrix of include/earhip.h (group M) on the CPU: `truth`, the formula in float64 on the float32 inputs and
taps, and `cpu_path`, what a libear user would write — one BlockConvolver (tests/_oracle.py: the restatement pinned to the
reference's kissfft) per non-zero pair, outputs summed in float32 in ascending c.  The bar of the device tests is set by the
CPU path's own error: e = ||. - truth|| / ||truth|| per output channel, e_device <= 1.5 e_cpu and e_cpu <= 1e-6."""
import functools

import numpy as np

# (C, K, taps, B, blocks, call lengths in blocks): the smallest shapes at which each mechanism can go wrong
SHAPES = {
    "one_tap": (1, 1, 1, 64, 3, (3,)),
    "last_partition_one_tap": (3, 2, 129, 64, 7, (1, 2, 4)),
    "taps_not_a_multiple": (5, 3, 700, 256, 5, (5,)),
    "monitoring": (24, 2, 2048, 512, 9, (4, 5)),
    "64_partitions": (2, 2, 4096, 64, 70, (70,)),
    "ring_longer_than_calls": (2, 1, 512, 64, 12, (1,) * 12),
    "widths_at_limits": (64, 16, 64, 64, 2, (2,)),
    "largest_block": (2, 2, 4097, 4096, 3, (3,)),
}

RATIO = 1.5    # e_device <= RATIO * e_cpu: tests/test_gpu_block_convolver.py's margin for a transform that sums in another order
E_CPU_MAX = 1e-6


def make_case(C, K, J, n, seed):
    """inputs uniform in [-1, 1], taps uniform x exp(-4 j / J)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (C, n)).astype(np.float32)
    h = (rng.uniform(-1.0, 1.0, (K, C, J)) * np.exp(-4.0 * np.arange(J) / J)).astype(np.float32)
    return x, h


def truth(x, h):
    """y[k][n] = sum over c, j of h[k][c][j] x[c][n - j] in float64, n < x.shape[1]"""
    x = np.asarray(x, np.float32).astype(np.float64)
    h = np.asarray(h, np.float32).astype(np.float64)
    K, C, _ = h.shape
    n = x.shape[1]
    y = np.zeros((K, n))
    for k in range(K):
        for c in range(C):
            if np.any(h[k, c] != 0.0):
                y[k] += np.convolve(x[c], h[k, c])[:n]
    return y


def cpu_path(x, h, B):
    """one BlockConvolver per non-zero pair, block by block, the pairs' outputs summed in float32 in ascending c"""
    import _oracle
    x = np.asarray(x, np.float32)
    h = np.asarray(h, np.float32)
    K, C, _ = h.shape
    n = x.shape[1]
    assert n % B == 0
    ctx = _oracle.ConvCtx(B)
    y = np.zeros((K, n), np.float32)
    for k in range(K):
        for c in range(C):
            if not np.any(h[k, c] != 0.0):
                continue
            conv = _oracle.BlockConvolver(ctx, _oracle.ConvFilter(ctx, h[k, c]))
            for t in range(n // B):
                y[k, t * B:(t + 1) * B] += conv.process(x[c, t * B:(t + 1) * B])
    return y


def rel_err(got, want):
    """per output channel ||got - want|| / ||want|| (0 where both are zero)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    num = np.linalg.norm(got - want, axis=1)
    den = np.linalg.norm(want, axis=1)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, h, truth, e_cpu per output) of a named shape: computed once, shared, left unchanged"""
    C, K, J, B, T, _ = SHAPES[name]
    x, h = make_case(C, K, J, B * T, seed=1 + sorted(SHAPES).index(name))
    want = truth(x, h)
    e_cpu = rel_err(cpu_path(x, h, B), want)
    for a in (x, h, want, e_cpu):
        a.setflags(write=False)
    return x, h, want, e_cpu


def check_against_bar(got, want, e_cpu, label):
    """prints the worst figures, then asserts the bar"""
    e_dev = rel_err(got, want)
    ratio = np.where(e_cpu > 0, e_dev / np.where(e_cpu > 0, e_cpu, 1.0), np.where(e_dev > 0, np.inf, 0.0))
    print(f"{label}: worst e_device {e_dev.max():.3e}, worst e_cpu {e_cpu.max():.3e}, worst ratio {ratio.max():.3f}")
    assert np.all(e_cpu <= E_CPU_MAX), (label, e_cpu.max())
    assert np.all(e_dev <= RATIO * e_cpu), (label, e_dev.max(), e_cpu.max(), ratio.max())
    return e_dev.max(), e_cpu.max(), ratio.max()
