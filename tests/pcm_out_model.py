"""numpy model of the float -> PCM conversion include/earhip.h defines for earhip_render_process_frames_pcm (group F): scale,
optional TPDF dither from a counter-based hash of (seed, sample clock, channel), round half to even, saturate, pack; with the
clip mask and the levels earhip_render_output_levels reports.  Independent of the device kernel: plain numpy float32 operations,
each of which rounds once, which is the definition."""
import numpy as np

import pcm_model

BITS = {"s16": 16, "s24": 24, "s32": 32}
DTYPE = {"s16": np.int16, "s24": np.uint8, "s32": np.int32, "f32": np.float32}


def _mix(a):
    a = a.astype(np.uint32)
    a = a ^ (a >> np.uint32(16))
    a = a * np.uint32(0x7FEB352D)
    a = a ^ (a >> np.uint32(15))
    a = a * np.uint32(0x846CA68B)
    return a ^ (a >> np.uint32(16))


def dither_hash(seed, t, n):
    """h(seed, t, n) of the header, uint32: t the sample clock (any int64, broadcast against n, the output channel)"""
    t = np.asarray(t, np.int64).astype(np.uint64)
    n = np.asarray(n, np.int64).astype(np.uint32)
    with np.errstate(over="ignore"):
        t_lo, t_hi = (t & np.uint64(0xFFFFFFFF)).astype(np.uint32), (t >> np.uint64(32)).astype(np.uint32)
        h = _mix(t_lo + np.uint32(0x9E3779B9))
        h = _mix(h ^ t_hi)
        h = _mix(h + n * np.uint32(0x85EBCA6B))
        return _mix(h ^ np.uint32(seed & 0xFFFFFFFF))


def dither(seed, t, n):
    """d of the header: TPDF over (-1, 1) LSB, float32 (exact multiples of 2^-16)"""
    h = dither_hash(seed, t, n)
    s = (h & np.uint32(0xFFFF)).astype(np.int64) + (h >> np.uint32(16)).astype(np.int64) - 65535
    return s.astype(np.float32) * np.float32(2.0 ** -16)


def from_float(x, fmt, dither_on=False, seed=0, t0=0):
    """x float32 [frames][N] (row f at sample clock t0 + f) -> (samples, clipped): samples int16 / int32 [frames][N], uint8
    [frames][3N] for s24, the float32 bits for f32; clipped bool [frames][N]"""
    x = np.asarray(x, np.float32)
    assert x.ndim == 2
    if fmt == "f32":
        assert not dither_on
        return x.copy(), np.zeros(x.shape, bool)
    bits = BITS[fmt]
    assert not dither_on or fmt == "s16"
    with np.errstate(over="ignore", invalid="ignore"):
        v = x * np.float32(2.0 ** (bits - 1))  # (one float32 multiply: exact short of overflow)
        if dither_on:
            t = np.int64(t0) + np.arange(x.shape[0], dtype=np.int64)[:, None]
            v = v + dither(seed, t, np.arange(x.shape[1])[None, :])  # (one float32 add)
        assert v.dtype == np.float32
        r = np.rint(v).astype(np.float64)  # (ties to even; every float32 is a float64)
    lo, hi = -(2.0 ** (bits - 1)), 2.0 ** (bits - 1) - 1
    nan = np.isnan(r)
    clipped = nan | (r > hi) | (r < lo)
    q = np.where(nan, 0.0, np.clip(r, lo, hi)).astype(np.int64)
    if fmt == "s16":
        return q.astype(np.int16), clipped
    if fmt == "s32":
        return q.astype(np.int32), clipped
    return pcm_model.s24_pack(q), clipped


def peak(x):
    """per channel max |x| of float32 [frames][N], NaN ignored (0 when there is nothing else)"""
    a = np.abs(np.asarray(x, np.float32))
    return np.max(np.where(np.isnan(a), np.float32(0), a), axis=0, initial=np.float32(0)).astype(np.float32)


def as_bytes(a):
    """any of the sample arrays as uint8 [frames][bytes per frame]"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)
