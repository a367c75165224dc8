"""Filter sets of the FIR filter matrix (include/earhip.h, group M, FILTER SETS) on the CPU, built from tests/firmix_model.py:
with y_s = h_s * x over the whole history, a select(to, F) before block s gives

    blocks before s:             y = y_from
    fade block q in [0, F):      a = (q B + n) / (F B),  y = (1 - a) y_from + a y_to
    blocks from s + F on:        y = y_to

`truth` is that blend in float64 of firmix_model.truth of each set; `cpu_path` is firmix_model.cpu_path of each set (one libear
BlockConvolver per non-zero pair), blended in float32 with the float32 a.  The bar is firmix_model.check_against_bar, taken over
the FADE BLOCKS' samples only (the steady blocks, which are bit-identical to a plain matrix, would dilute it).

A select acts on the next block FED, so it falls between two calls: where a shape's select block lies inside one of its calls
(lists_differ: one call of 5 blocks, select before block 2) `cut_calls` cuts that call there, (5,) -> (2, 3), and every matrix
compared is fed the cut calls."""
import functools

import numpy as np

import firmix_model as fm

# (C, K, taps, B, blocks, calls, select before block, F)
SHAPES = {
    "one_block": (3, 2, 129, 64, 7, (1, 2, 4), 1, 1),
    "across_calls": (2, 3, 200, 64, 8, (2, 2, 4), 2, 3),
    "monitoring": (24, 2, 2048, 512, 6, (3, 3), 3, 1),
    "lists_differ": (4, 4, 100, 64, 5, (5,), 2, 2),
}
SEEDS = {"one_block": 201, "across_calls": 202, "monitoring": 203, "lists_differ": 204}  # set 0; set 1: + 100


def cut_calls(calls, s):
    """the calls, with the one that block s lies inside cut at s"""
    out, at = [], 0
    for nb in calls:
        if at < s < at + nb:
            out += [s - at, at + nb - s]
        else:
            out.append(nb)
        at += nb
    return tuple(out)


def gain(F, B, dtype):
    """a of every sample of the F fade blocks"""
    if dtype == np.float32:
        return np.arange(F * B).astype(np.float32) / np.float32(F * B)
    return np.arange(F * B, dtype=np.float64) / float(F * B)


def blend(y_from, y_to, B, s, F, dtype):
    y_from, y_to = np.asarray(y_from, dtype), np.asarray(y_to, dtype)
    y = y_to.copy()
    y[:, :s * B] = y_from[:, :s * B]
    if F:
        a = gain(F, B, dtype)
        lo, hi = s * B, (s + F) * B
        y[:, lo:hi] = (dtype(1) - a) * y_from[:, lo:hi] + a * y_to[:, lo:hi]
    return y


def truth(x, h_from, h_to, B, s, F):
    return blend(fm.truth(x, h_from), fm.truth(x, h_to), B, s, F, np.float64)


def cpu_path(x, h_from, h_to, B, s, F):
    return blend(fm.cpu_path(x, h_from, B), fm.cpu_path(x, h_to, B), B, s, F, np.float32)


def make_sets(name):
    C, K, J, B, T, _, _, _ = SHAPES[name]
    x, h0 = fm.make_case(C, K, J, B * T, SEEDS[name])
    h1 = fm.make_case(C, K, J, B * T, SEEDS[name] + 100)[1]
    if name == "lists_differ":  # set 0 diagonal, set 1 anti-diagonal without the last output's pair
        eye = np.eye(K, C, dtype=np.float32)
        anti = eye[:, ::-1].copy()
        anti[K - 1] = 0.0
        h0 = h0 * eye[:, :, None]
        h1 = h1 * anti[:, :, None]
    return x, h0, h1


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, h0, h1, truth, e_cpu over the fade blocks per output) of a named shape: computed once, shared, left unchanged"""
    C, K, J, B, T, _, s, F = SHAPES[name]
    x, h0, h1 = make_sets(name)
    want = truth(x, h0, h1, B, s, F)
    fade = slice(s * B, (s + F) * B)
    e_cpu = fm.rel_err(cpu_path(x, h0, h1, B, s, F)[:, fade], want[:, fade])
    for a in (x, h0, h1, want, e_cpu):
        a.setflags(write=False)
    return x, h0, h1, want, e_cpu
