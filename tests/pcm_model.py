"""numpy model of the PCM conversion include/earhip.h defines for earhip_render_process_frames, and helpers that build frame
buffers: the reference every frames test converts with (independent of the device kernel)."""
import numpy as np

SAMPLE_BYTES = {"s16": 2, "s24": 3, "s32": 4, "f32": 4}


def to_float(x, fmt):
    """interleaved frames x -> float32 [frames][C] by the header's rules: s16 int16 [F][C] -> x * 2^-15; s24 uint8 [F][3C] ->
    3 little-endian bytes sign-extended from bit 23, * 2^-23; s32 int32 [F][C] -> float32(x) (nearest even) * 2^-31; f32: the bits"""
    if fmt == "s16":
        assert x.dtype == np.int16
        return x.astype(np.float32) * np.float32(2.0 ** -15)
    if fmt == "s24":
        assert x.dtype == np.uint8 and x.shape[1] % 3 == 0
        b = x.reshape(x.shape[0], -1, 3).astype(np.int32)
        v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return v.astype(np.float32) * np.float32(2.0 ** -23)
    if fmt == "s32":
        assert x.dtype == np.int32
        return x.astype(np.float32) * np.float32(2.0 ** -31)  # (int32 -> float32: round to nearest even)
    if fmt == "f32":
        assert x.dtype == np.float32
        return x.copy()
    raise ValueError(fmt)


def rows(x, fmt, first, M):
    """the renderer's planar inputs [M][frames] float32: channels [first, first + M) of the converted frames"""
    return np.ascontiguousarray(to_float(x, fmt)[:, first:first + M].T)


def s24_pack(v):
    """int32 values in [-2^23, 2^23) [F][C] -> uint8 [F][3C], little-endian"""
    u = np.asarray(v, np.int64) & 0xFFFFFF
    out = np.empty(u.shape + (3,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF
    return out.reshape(u.shape[0], -1)


def random_frames(rng, fmt, frames, channels, extremes=False):
    """interleaved frames of full-scale noise (extremes: the format's limits mixed in)"""
    if fmt == "s16":
        x = rng.integers(-32768, 32768, size=(frames, channels), dtype=np.int16)
        if extremes:
            x.flat[::7] = -32768
            x.flat[3::11] = 32767
        return x
    if fmt == "s24":
        v = rng.integers(-(1 << 23), 1 << 23, size=(frames, channels), dtype=np.int64)
        if extremes:
            v.flat[::7] = -(1 << 23)
            v.flat[3::11] = (1 << 23) - 1
        return s24_pack(v)
    if fmt == "s32":
        x = rng.integers(-(1 << 31), 1 << 31, size=(frames, channels), dtype=np.int64).astype(np.int32)
        if extremes:
            x.flat[::7] = np.iinfo(np.int32).min
            x.flat[3::11] = np.iinfo(np.int32).max
            x.flat[5::13] = (1 << 24) + 1  # (rounds to even: 2^24)
            x.flat[6::13] = (1 << 24) + 3  # (rounds up: 2^24 + 4)
        return x
    if fmt == "f32":
        return rng.uniform(-1.0, 1.0, size=(frames, channels)).astype(np.float32)
    raise ValueError(fmt)
