"""Interleaved PCM frames OUT of the Objects renderer (include/earhip.h: earhip_render_process_frames_pcm / _pcm_device,
earhip_render_output_levels), on the GPU.

The reference of every comparison is the project's existing call, never the new code: the numpy model of the header's conversion
(tests/pcm_out_model.py) applied to what earhip_render_process_frames(..., out_interleaved = 1) returns for the same frames, in
the same kind of memory, from the same reset, cut into the same calls.  Every comparison is BYTE-FOR-BYTE equality."""
import ctypes as C

import numpy as np
import pytest

import pcm_model
import pcm_out_model as om
import scenes
from layouts import LAYOUTS

pytestmark = pytest.mark.gpu

OUT_FORMATS = ("s16", "s24", "s32", "f32")


@pytest.fixture(scope="module")
def ctx():
    from libear_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def make_renderer(ctx, M, layout, B, T, curves, two_bus=True):
    from libear_amd import capi
    names = LAYOUTS[layout]
    dec = capi.design_decorrelators(names) if two_bus else None
    r = capi.Renderer(ctx, M, len(names), B, dec, 255 if two_bus else 0, max_blocks=T)
    for i, (t, d, f) in enumerate(curves):
        r.set_object_points(i, t, d, f if two_bus else None)
    r.commit()
    return r


def host_copy(ctx, a, pinned, keep):
    if not pinned:
        return np.array(a, copy=True)
    p = ctx.pinned_array(a.shape, a.dtype)
    p[...] = a
    keep.append(p)
    return p


def release_all(ctx, keep):
    for a in keep:
        ctx.release(a)
    keep.clear()


def float_reference(ctx, r, x, fmt, first, nblocks_list, t0, pinned, keep):
    """the existing call: interleaved float frames [frames][N] of consecutive calls from reset(t0), and their chunk counts"""
    B, N = r.B, r.N
    r.reset(t0)
    at, parts, chunks = 0, [], []
    for nb in nblocks_list:
        xf = host_copy(ctx, x[at:at + nb * B], pinned, keep)
        out = host_copy(ctx, np.zeros((nb * B, N), np.float32), pinned, keep)
        parts.append(np.array(r.process_frames_into(xf, out, fmt, first, interleaved_out=True)))
        chunks.append(r.last_host_chunks())
        at += nb * B
    return np.concatenate(parts, axis=0), chunks


def pcm_calls(ctx, r, x, fmt, first, nblocks_list, t0, out_fmt, pinned, keep, dither=False, seed=0, chunks=None):
    """the new call, cut the same way: uint8 [frames][bytes per frame]"""
    from libear_amd import capi
    B, N = r.B, r.N
    _, dtype, cols = capi.pcm_format(out_fmt)
    r.reset(t0)
    at, parts = 0, []
    for k, nb in enumerate(nblocks_list):
        xf = host_copy(ctx, x[at:at + nb * B], pinned, keep)
        out = host_copy(ctx, np.zeros((nb * B, N * cols), dtype), pinned, keep)
        r.process_frames_pcm_into(xf, out, fmt, first, out_fmt, dither, seed)
        if chunks is not None:
            assert r.last_host_chunks() == chunks[k], (r.last_host_chunks(), chunks[k])
        parts.append(om.as_bytes(np.array(out)))
        at += nb * B
    return np.concatenate(parts, axis=0)


def assert_both_branches(ref, fmt):
    """the reference itself has clipped and unclipped samples on every channel: neither branch of the conversion is vacuous"""
    _, clip = om.from_float(ref, fmt)
    assert clip.any(axis=0).all() and (~clip).any(axis=0).all(), (fmt, clip.mean(axis=0))


@pytest.mark.parametrize("two_bus", [True, False])
@pytest.mark.parametrize("in_fmt", ["s16", "s24", "f32"])
def test_every_out_format_equals_the_model_of_the_float_call(ctx, in_fmt, two_bus):
    """s16 / s24 / s32 / f32 out x s16 / s24 / f32 in, one- and two-bus renderers, M = 13 (not a multiple of 4), N = 11 (odd: s16
    and s24 frames are no dword multiples), frames wider than the renderer with its channels at an odd offset, three consecutive
    calls of different block counts (state carried over), pageable and device-reachable memory; and the levels: peak = max
    |reference| bitwise, clipped = the model's count, accumulated over the calls"""
    M, layout, B, T = 13, "4+5+1", 512, 3
    N = len(LAYOUTS[layout])
    assert N % 2 == 1
    cuts = [2, 1, 3]
    total = sum(cuts) * B
    r = make_renderer(ctx, M, layout, B, T, scenes.ragged_curves(M, N, total, seed=61), two_bus)
    rng = np.random.default_rng(23)
    x = pcm_model.random_frames(rng, in_fmt, total, M + 4)
    keep = []
    try:
        for pinned in (False, True):
            ref, chunks = float_reference(ctx, r, x, in_fmt, 3, cuts, 0, pinned, keep)
            assert chunks == [0, 0, 0]
            for out_fmt in OUT_FORMATS:
                if out_fmt != "f32":
                    assert_both_branches(ref, out_fmt)
                want, clip = om.from_float(ref, out_fmt)
                got = pcm_calls(ctx, r, x, in_fmt, 3, cuts, 0, out_fmt, pinned, keep, chunks=chunks)
                assert np.array_equal(got, om.as_bytes(want)), (in_fmt, out_fmt, two_bus, pinned)
                peak, clipped = r.output_levels()
                assert np.array_equal(peak.view(np.uint32), om.peak(ref).view(np.uint32)), (out_fmt, peak, om.peak(ref))
                assert np.array_equal(clipped, clip.sum(axis=0).astype(np.uint64)), (out_fmt, clipped, clip.sum(axis=0))
            release_all(ctx, keep)
        assert r.scratch_regrows() == 0
    finally:
        release_all(ctx, keep)
        r.close()


def test_levels_accumulate_reset_and_ignore_float_calls(ctx):
    M, layout, B, T = 13, "0+5+0", 256, 4
    N = len(LAYOUTS[layout])
    r = make_renderer(ctx, M, layout, B, T, scenes.ragged_curves(M, N, 3 * T * B, seed=63))
    x = pcm_model.random_frames(np.random.default_rng(29), "s16", 3 * T * B, M)
    keep = []
    try:
        peak, clipped = r.output_levels()  # (before any PCM-out call)
        assert not peak.any() and not clipped.any() and peak.dtype == np.float32 and clipped.dtype == np.uint64
        ref, _ = float_reference(ctx, r, x, "s16", 0, [T, T, T], 7, False, keep)
        _, clip = om.from_float(ref, "s16")
        assert_both_branches(ref, "s16")
        n = T * B
        r.reset(7)
        r.process_frames_pcm(x[:n], "s16", 0, "s16")
        peak, clipped = r.output_levels()
        assert np.array_equal(peak.view(np.uint32), om.peak(ref[:n]).view(np.uint32))
        assert np.array_equal(clipped, clip[:n].sum(axis=0).astype(np.uint64))
        # a float-out call in between leaves them alone (and renders the second part of the stream)
        r.process_frames(x[n:2 * n], "s16", 0, interleaved_out=True)
        p2, c2 = r.output_levels()
        assert np.array_equal(p2, peak) and np.array_equal(c2, clipped)
        # the third part in s24: both numbers go on from where they were
        r.process_frames_pcm(x[2 * n:], "s16", 0, "s24")
        _, clip24 = om.from_float(ref[2 * n:], "s24")
        p3, c3 = r.output_levels(reset=True)
        assert np.array_equal(p3.view(np.uint32), np.maximum(om.peak(ref[:n]), om.peak(ref[2 * n:])).view(np.uint32))
        assert np.array_equal(c3, (clip[:n].sum(axis=0) + clip24.sum(axis=0)).astype(np.uint64))
        p4, c4 = r.output_levels()  # (the reset argument zeroed them)
        assert not p4.any() and not c4.any()
        r.process_frames_pcm(x[:n], "s16", 0, "s16")
        assert r.output_levels()[1].any()
        r.reset(0)  # (earhip_render_reset zeroes them too)
        p5, c5 = r.output_levels()
        assert not p5.any() and not c5.any()
    finally:
        r.close()


def test_non_finite_samples_nan_to_zero_inf_saturated_both_counted(ctx):
    """f32 frames with NaN payloads, +-inf and denormals on a direct-bus-only renderer (the scene of test_gpu_render_frames.py's
    NaN test): NaN -> 0 and counted, inf saturated and counted, by the model of the float call's own output"""
    from libear_amd import capi
    M, N, B, T = 5, 2, 256, 2
    n = T * B
    r = capi.Renderer(ctx, M, N, B, None, 0, max_blocks=T)
    for i in range(M):
        g = np.zeros((2, N), np.float32)
        g[0, i % N], g[1, (i + 1) % N] = 1.0, 0.5
        r.set_object_points(i, np.array([0, n], np.int64), g)
    raw = np.random.default_rng(13).integers(0, 1 << 32, size=(n, M + 2), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00400000, 0x80000000], np.uint32)
    raw[:, 1:3] = np.resize(special, raw[:, 1:3].shape)
    fin = np.random.default_rng(14).uniform(-1, 1, size=(n, M + 2)).astype(np.float32)
    fin[::3, 1] = np.array([1e-40, -3e-42, 1.4e-45], np.float32)[np.arange(fin[::3, 1].size) % 3]
    fin[5::7, 2] = np.float32(np.inf)
    fin[6::7, 2] = np.float32(-np.inf)
    fin[3::11, 3] = np.float32(np.nan)
    keep = []
    try:
        # (the default gain kernels split their inputs into f16 pieces, which turns an infinite input into NaN: infinities reach
        # the converter in strict mode, libear's own arithmetic; the random-bits scene has both infinities in every other frame)
        for x, strict in ((raw.view(np.float32), False), (fin, False), (fin, True)):
            ctx.set_strict(strict)
            ref, _ = float_reference(ctx, r, x, "f32", 1, [T], 0, False, keep)
            assert np.isnan(ref).any() and np.isfinite(ref).any()
            if strict:
                assert (ref == np.inf).any() and (ref == -np.inf).any()
            for out_fmt in OUT_FORMATS:
                want, clip = om.from_float(ref, out_fmt)
                if out_fmt != "f32":
                    assert clip[np.isnan(ref)].all() and clip[np.isinf(ref)].all()
                got = pcm_calls(ctx, r, x, "f32", 1, [T], 0, out_fmt, False, keep)
                assert np.array_equal(got, om.as_bytes(want)), out_fmt
                peak, clipped = r.output_levels()
                assert np.array_equal(peak.view(np.uint32), om.peak(ref).view(np.uint32))
                assert np.array_equal(clipped, clip.sum(axis=0).astype(np.uint64))
    finally:
        ctx.set_strict(False)
        r.close()


@pytest.mark.parametrize("t0", [12345, 2 ** 40 + 3])
def test_dither_follows_the_sample_clock_not_the_calls(ctx, t0):
    """bytes equal the model's with t0 from reset; the same stream as one call of T blocks and cut as (1, T - 1) and (T / 2, T / 2)
    each equals the model applied to ITS OWN float reference with the stream's clock (the float results may differ in the last
    bit between cuts, the dither may not); two seeds differ"""
    M, layout, B, T = 13, "4+5+1", 512, 8
    N = len(LAYOUTS[layout])
    r = make_renderer(ctx, M, layout, B, T, scenes.ragged_curves(M, N, T * B, seed=65))
    x = pcm_model.random_frames(np.random.default_rng(31), "s16", T * B, M)
    x = (x.astype(np.int32) // 64).astype(np.int16)  # (quiet: the dither decides many samples; some still clip)
    keep = []
    try:
        outs = {}
        for cuts in ([T], [1, T - 1], [T // 2, T // 2]):
            ref, _ = float_reference(ctx, r, x, "s16", 0, cuts, t0, False, keep)
            want, _ = om.from_float(ref, "s16", dither_on=True, seed=77, t0=t0)
            plain, _ = om.from_float(ref, "s16")
            assert np.mean(want != plain) > 0.2  # (the dither is really there)
            got = pcm_calls(ctx, r, x, "s16", 0, cuts, t0, "s16", False, keep, dither=True, seed=77)
            assert np.array_equal(got, om.as_bytes(want)), cuts
            outs[tuple(cuts)] = got
        other = pcm_calls(ctx, r, x, "s16", 0, [T], t0, "s16", False, keep, dither=True, seed=78)
        assert np.mean(other != outs[(T,)]) > 0.1
        ref, _ = float_reference(ctx, r, x, "s16", 0, [T], t0, False, keep)
        want, _ = om.from_float(ref, "s16", dither_on=True, seed=78, t0=t0)
        assert np.array_equal(other, om.as_bytes(want))
    finally:
        r.close()


@pytest.mark.parametrize("out_fmt", ["s16", "s24"])
def test_long_pipelined_calls(ctx, out_fmt):
    """>= 16 MB of float-equivalent input per call with HOST_CHUNK_MB = 4: >= 3 chunks; input and output pageable and
    earhip_host_alloc-ed; equal to the reference, and no scratch regrowth after the first call"""
    M, layout, B, T = 61, "0+5+0", 512, 140
    N = len(LAYOUTS[layout])
    assert 4 * M * T * B >= 16 << 20
    r = make_renderer(ctx, M, layout, B, T, scenes.ragged_curves(M, N, 2 * T * B, seed=67))
    ctx.set_option("HOST_CHUNK_MB", 4)
    x = pcm_model.random_frames(np.random.default_rng(37), "s16", 2 * T * B, 2 * M + 1)
    x = (x.astype(np.int32) // 4).astype(np.int16)
    keep = []
    try:
        for pinned in (False, True):
            ref, chunks = float_reference(ctx, r, x, "s16", M + 1, [T, T], 0, pinned, keep)
            assert min(chunks) >= 3, chunks
            assert_both_branches(ref, out_fmt)
            want, clip = om.from_float(ref, out_fmt)
            got = pcm_calls(ctx, r, x, "s16", M + 1, [T, T], 0, out_fmt, pinned, keep, chunks=chunks)
            assert r.last_host_chunks() >= 3
            assert np.array_equal(got, om.as_bytes(want)), (out_fmt, pinned)
            peak, clipped = r.output_levels()
            assert np.array_equal(peak.view(np.uint32), om.peak(ref).view(np.uint32))
            assert np.array_equal(clipped, clip.sum(axis=0).astype(np.uint64))
            assert r.scratch_regrows() == 0
            release_all(ctx, keep)
    finally:
        release_all(ctx, keep)
        ctx.set_option("HOST_CHUNK_MB", None)
        r.close()


def device_float_reference(ctx, r, xdev_ptr, fmt, C_, first, T, n, N, t0):
    import torch
    r.reset(t0)
    o = torch.empty((n, N), dtype=torch.float32, device="cuda")
    r.process_frames_device(T, xdev_ptr, fmt, C_, first, o.data_ptr(), N, True)
    ctx.synchronize()
    return o.cpu().numpy()


@pytest.mark.parametrize("out_fmt", OUT_FORMATS)
def test_device_form_writes_its_runs_and_nothing_else(ctx, out_fmt):
    """out_frame_bytes wider than the run, a non-zero out_first_byte (odd for s24, and the buffer itself at an odd byte), the
    buffer pre-filled with a byte pattern: the runs equal the model of earhip_render_process_frames_device's interleaved floats,
    every other byte still holds the pattern; with and without dither"""
    import torch
    from libear_amd import capi
    M, layout, B, T = 29, "4+5+1", 512, 4
    N = len(LAYOUTS[layout])
    n = T * B
    r = make_renderer(ctx, M, layout, B, T, scenes.ragged_curves(M, N, n, seed=69))
    x = pcm_model.random_frames(np.random.default_rng(41), "s16", n, M + 3)
    xdev = torch.from_numpy(x).cuda()
    So = capi.pcm_format(out_fmt)[2] * np.dtype(capi.pcm_format(out_fmt)[1]).itemsize
    run = N * So
    first_byte = 5 if out_fmt == "s24" else 2 * So
    fbytes = run + first_byte + (7 if out_fmt == "s24" else 3 * So)
    shift = 1 if out_fmt == "s24" else 0
    try:
        ref = device_float_reference(ctx, r, xdev.data_ptr(), "s16", M + 3, 1, T, n, N, 99)
        if out_fmt != "f32":
            assert_both_branches(ref, out_fmt)
        for dither in ((False, True) if out_fmt == "s16" else (False,)):
            want, _ = om.from_float(ref, out_fmt, dither_on=dither, seed=5, t0=99)
            pattern = (np.arange(n * fbytes + 16, dtype=np.int64) * 37 + 11).astype(np.uint8)
            buf = torch.from_numpy(pattern.copy()).cuda()
            r.reset(99)
            r.process_frames_pcm_device(T, xdev.data_ptr(), "s16", M + 3, 1, buf.data_ptr() + shift, fbytes, first_byte, out_fmt,
                                        dither, 5)
            ctx.synchronize()
            got = buf.cpu().numpy()
            body = got[shift:shift + n * fbytes].reshape(n, fbytes)
            assert np.array_equal(body[:, first_byte:first_byte + run], om.as_bytes(want)), (out_fmt, dither)
            mask = np.ones(got.size, bool)
            m2 = mask[shift:shift + n * fbytes].reshape(n, fbytes)
            m2[:, first_byte:first_byte + run] = False
            assert np.array_equal(got[mask], pattern[mask]), (out_fmt, dither)
    finally:
        r.close()


@pytest.mark.parametrize("out_fmt", ["s16", "s24"])
def test_two_renderers_fill_disjoint_channels_of_the_same_frames(ctx, out_fmt):
    """two renderers (6 and 11 channels) write bytes [0, 6 S) and [6 S, 17 S) of the same frames of 17 S + 1 bytes (s24) / 18 S
    (s16), enqueued back to back: both runs intact — their shared edge dwords were written as bytes —, the padding untouched"""
    import torch
    M, B, T = 13, 512, 4
    n = T * B
    la, lb = "0+5+0", "4+5+1"
    Na, Nb = len(LAYOUTS[la]), len(LAYOUTS[lb])
    ra = make_renderer(ctx, M, la, B, T, scenes.ragged_curves(M, Na, n, seed=71))
    rb = make_renderer(ctx, M, lb, B, T, scenes.ragged_curves(M, Nb, n, seed=73))
    x = pcm_model.random_frames(np.random.default_rng(43), "s16", n, 2 * M)
    xdev = torch.from_numpy(x).cuda()
    So = 2 if out_fmt == "s16" else 3
    fbytes = (Na + Nb) * So + (1 if out_fmt == "s24" else So)
    try:
        refa = device_float_reference(ctx, ra, xdev.data_ptr(), "s16", 2 * M, 0, T, n, Na, 0)
        refb = device_float_reference(ctx, rb, xdev.data_ptr(), "s16", 2 * M, M, T, n, Nb, 0)
        pattern = (np.arange(n * fbytes, dtype=np.int64) * 29 + 3).astype(np.uint8)
        buf = torch.from_numpy(pattern.copy()).cuda()
        ra.reset(0)
        rb.reset(0)
        ra.process_frames_pcm_device(T, xdev.data_ptr(), "s16", 2 * M, 0, buf.data_ptr(), fbytes, 0, out_fmt)
        rb.process_frames_pcm_device(T, xdev.data_ptr(), "s16", 2 * M, M, buf.data_ptr(), fbytes, Na * So, out_fmt)
        ctx.synchronize()
        got = buf.cpu().numpy().reshape(n, fbytes)
        assert np.array_equal(got[:, :Na * So], om.as_bytes(om.from_float(refa, out_fmt)[0]))
        assert np.array_equal(got[:, Na * So:(Na + Nb) * So], om.as_bytes(om.from_float(refb, out_fmt)[0]))
        assert np.array_equal(got[:, (Na + Nb) * So:], pattern.reshape(n, fbytes)[:, (Na + Nb) * So:])
    finally:
        ra.close()
        rb.close()


def test_every_error_case_leaves_the_output_untouched(ctx):
    import torch
    from libear_amd import capi
    lib = capi.load()
    M, layout, B, T = 13, "0+5+0", 256, 2
    N = len(LAYOUTS[layout])
    n = T * B
    r = make_renderer(ctx, M, layout, B, T, scenes.ragged_curves(M, N, n, seed=53))
    raw = np.zeros(n * (M + 3) * 4 + 64, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % 16)
    outbuf = np.full(n * N * 4 + 64, 0x5A, np.uint8)
    obase = outbuf.ctypes.data + (-outbuf.ctypes.data % 16)

    def spec(fmt=1, dither=0, seed=0):
        return capi.PcmOut(fmt, dither, seed)

    def call(nblocks=T, frames=base, fmt=1, C_=M + 3, first=0, o=obase, sp=spec()):
        return lib.earhip_render_process_frames_pcm(r.h, C.c_size_t(nblocks), C.c_void_p(frames), C.c_int(fmt), C.c_int(C_), C.c_int(first),
                                                    C.c_void_p(o), C.byref(sp) if sp is not None else None)
    cases = {
        "unknown format 0": dict(fmt=0), "unknown format 5": dict(fmt=5), "first < 0": dict(first=-1), "first + M > C": dict(first=4),
        "C < M": dict(C_=M - 1), "NULL frames": dict(frames=None), "nblocks > max_blocks": dict(nblocks=T + 1),
        "s16 in misaligned": dict(frames=base + 1), "NULL out_frames": dict(o=None), "NULL out": dict(sp=None),
        "unknown out format 0": dict(sp=spec(0)), "unknown out format 9": dict(sp=spec(9)), "dither with s24": dict(sp=spec(2, 1)),
        "dither with s32": dict(sp=spec(3, 1)), "dither with f32": dict(sp=spec(4, 1)), "dither = 2": dict(sp=spec(1, 2)),
        "s16 out misaligned": dict(o=obase + 1), "s32 out misaligned": dict(o=obase + 2, sp=spec(3)),
        "f32 out misaligned": dict(o=obase + 1, sp=spec(4)),
    }
    try:
        assert call() == capi.OK
        outbuf[...] = 0x5A
        for name, kw in cases.items():
            assert call(**kw) == capi.INVALID_ARGUMENT, name
            assert (outbuf == 0x5A).all(), name
        assert call(o=obase + 1, sp=spec(2)) == capi.OK  # s24 out may start at any byte
        assert call(sp=spec(1, 1, 9)) == capi.OK
        dev = torch.full((n * (N + 2) * 4 + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        fr = torch.zeros(n * (M + 3) * 2 + 16, dtype=torch.uint8, device="cuda")

        def dcall(nblocks=T, frames=fr.data_ptr(), fmt=1, C_=M + 3, first=0, o=dev.data_ptr(), fbytes=(N + 2) * 2, fbyte=2, sp=spec()):
            return lib.earhip_render_process_frames_pcm_device(r.h, C.c_size_t(nblocks), C.c_void_p(frames), C.c_int(fmt), C.c_int(C_),
                                                                C.c_int(first), C.c_void_p(o), C.c_size_t(fbytes), C.c_size_t(fbyte),
                                                                C.byref(sp) if sp is not None else None)
        dcases = {
            "unknown format": dict(fmt=7), "first < 0": dict(first=-1), "NULL frames": dict(frames=None), "NULL out_dev": dict(o=None),
            "NULL out": dict(sp=None), "nblocks > max_blocks": dict(nblocks=T + 1), "unknown out format": dict(sp=spec(6)),
            "dither with s24": dict(sp=spec(2, 1), fbytes=(N + 2) * 3, fbyte=3), "frame too small": dict(fbytes=N * 2 - 2, fbyte=0),
            "first byte beyond": dict(fbyte=6), "s16 odd first byte": dict(fbyte=1), "s16 odd frame bytes": dict(fbytes=(N + 2) * 2 + 1),
            "s32 frame bytes not x4": dict(sp=spec(3), fbytes=(N + 2) * 4 + 2, fbyte=4), "f32 first byte not x4": dict(sp=spec(4), fbytes=(N + 2) * 4, fbyte=2),
            "s16 out_dev misaligned": dict(o=dev.data_ptr() + 1),
        }
        for name, kw in dcases.items():
            assert dcall(**kw) == capi.INVALID_ARGUMENT, name
        ctx.synchronize()
        assert (dev == 0x5A).all()
        assert dcall() == capi.OK
        assert dcall(sp=spec(2), fbytes=N * 3 + 2, fbyte=1, o=dev.data_ptr() + 1) == capi.OK  # s24: any byte
        ctx.synchronize()
    finally:
        r.close()
