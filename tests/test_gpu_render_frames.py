"""Interleaved PCM frames into the Objects renderer (include/earhip.h: earhip_render_process_frames / _device), on the GPU.

The reference of every case is earhip_render_process (or _process_device) on the planar float rows the numpy model of the
header's conversion (tests/pcm_model.py) makes from the same frames, held in the same kind of memory: the outputs must be
BIT-IDENTICAL, in default and in strict mode — both forms take the same chunk plan, and the conversion is exact.  Curves
ramp, step and hold (scenes.ragged_curves); M is not a multiple of 4; frames are wider than the renderer's channels, with the
renderer's range at the start, at an odd offset and at the end."""
import ctypes as C

import numpy as np
import pytest

import pcm_model
import scenes
from layouts import LAYOUTS

pytestmark = pytest.mark.gpu

FORMATS = ("s16", "s24", "s32", "f32")


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
    return r


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def host_copy(ctx, a, pinned, keep):
    """a in pageable memory (a copy), or in earhip_host_alloc memory"""
    if not pinned:
        return np.array(a, copy=True)
    p = ctx.pinned_array(a.shape, a.dtype)
    p[...] = a
    keep.append(p)
    return p


def render_pair(ctx, r, x, fmt, first, pinned, interleaved, nblocks_list, keep):
    """(reference, frames form) outputs [N][total] of consecutive calls of nblocks_list blocks, each form from reset(0)"""
    M, N, B = r.M, r.N, r.B
    want, got, chunks = [], [], []
    rows_all = pcm_model.rows(x, fmt, first, M)
    r.reset(0)
    at = 0
    for nb in nblocks_list:
        rows = host_copy(ctx, rows_all[:, at:at + nb * B], pinned, keep)
        want.append(r.process_into(rows, np.empty((N, nb * B), np.float32)))
        chunks.append(r.last_host_chunks())
        at += nb * B
    r.reset(0)
    at = 0
    for k, nb in enumerate(nblocks_list):
        xf = host_copy(ctx, x[at:at + nb * B], pinned, keep)
        o = r.process_frames(xf, fmt, first, interleaved_out=interleaved)
        got.append(o.T if interleaved else o)
        assert r.last_host_chunks() == chunks[k], (r.last_host_chunks(), chunks[k])
        at += nb * B
    return np.concatenate(want, axis=1), np.concatenate(got, axis=1), chunks


def release_all(ctx, keep):
    for a in keep:
        ctx.release(a)
    keep.clear()


@pytest.mark.parametrize("strict", [False, True])
def test_short_calls_bit_identical(ctx, strict):
    """every format x frame widths {M, M+3, 2M+1} x first channel at 0 / odd / the end x pageable / host_alloc x planar /
    interleaved outputs; two consecutive calls (state carried over)"""
    M, layout, B, T = 13, "0+5+0", 512, 3
    N = len(LAYOUTS[layout])
    curves = scenes.ragged_curves(M, N, 2 * T * B, seed=41)
    ctx.set_strict(strict)
    r = make_renderer(ctx, M, layout, B, T, curves)
    rng = np.random.default_rng(5)
    keep = []
    n_cases = 0
    try:
        for fmt in FORMATS:
            for C_, first in ((M, 0), (M + 3, 1), (M + 3, 3), (2 * M + 1, M + 1), (2 * M + 1, 0)):
                x = pcm_model.random_frames(rng, fmt, 2 * T * B, C_)
                for pinned in (False, True):
                    for interleaved in (False, True):
                        want, got, chunks = render_pair(ctx, r, x, fmt, first, pinned, interleaved, [T, T], keep)
                        assert chunks == [0, 0]
                        assert np.isfinite(want).all() and np.abs(want).max() > 0
                        assert bits_equal(got, want), (fmt, C_, first, pinned, interleaved, np.abs(got - want).max())
                        n_cases += 1
                release_all(ctx, keep)
    finally:
        release_all(ctx, keep)
        r.close()
        ctx.set_strict(False)
    print(f"short calls ({'strict' if strict else 'default'}): {n_cases} cases bit-identical")


@pytest.mark.parametrize("fmt", FORMATS)
def test_long_pipelined_calls_bit_identical(ctx, fmt):
    """>= 16 MB of float-equivalent input per call: the pipeline, >= 3 chunks (HOST_CHUNK_MB = 4), pageable and host_alloc frames,
    planar and interleaved outputs, two consecutive calls; 2M + 1 channels a frame with the renderer's at the odd offset M + 1"""
    M, layout, B, T = 61, "0+5+0", 512, 140
    N = len(LAYOUTS[layout])
    assert 4 * M * T * B >= 16 << 20
    curves = scenes.ragged_curves(M, N, 2 * T * B, seed=43)
    r = make_renderer(ctx, M, layout, B, T, curves)
    ctx.set_option("HOST_CHUNK_MB", 4)
    rng = np.random.default_rng(7)
    x = pcm_model.random_frames(rng, fmt, 2 * T * B, 2 * M + 1)
    keep = []
    try:
        for pinned in (False, True):
            for interleaved in (False, True):
                want, got, chunks = render_pair(ctx, r, x, fmt, M + 1, pinned, interleaved, [T, T], keep)
                assert min(chunks) >= 3, chunks
                assert bits_equal(got, want), (fmt, pinned, interleaved, np.abs(got - want).max())
                release_all(ctx, keep)
    finally:
        release_all(ctx, keep)
        ctx.set_option("HOST_CHUNK_MB", None)
        r.close()
    print(f"long calls {fmt}: chunks {chunks}, bit-identical")


@pytest.mark.parametrize("strict", [False, True])
def test_long_calls_odd_block_size_and_frame_counts(ctx, strict):
    """block 243 (the chunks start on 4-block boundaries: odd frame counts per chunk), an odd number of blocks (the last chunk's
    frames odd), s24 frames of 3 (2M + 1) bytes (chunks start at odd byte offsets), the renderer's channels at the end"""
    M, layout, B, T = 67, "0+5+0", 243, 297
    N = len(LAYOUTS[layout])
    curves = scenes.ragged_curves(M, N, T * B, seed=45)
    ctx.set_strict(strict)
    r = make_renderer(ctx, M, layout, B, T, curves)
    ctx.set_option("HOST_CHUNK_MB", 4)
    rng = np.random.default_rng(9)
    keep = []
    try:
        for fmt in ("s24", "s16"):
            x = pcm_model.random_frames(rng, fmt, T * B, 2 * M + 1, extremes=True)
            for pinned in (False, True):
                want, got, chunks = render_pair(ctx, r, x, fmt, M + 1, pinned, True, [T], keep)
                assert chunks[0] >= 3
                assert bits_equal(got, want), (fmt, pinned, np.abs(got - want).max())
                release_all(ctx, keep)
    finally:
        release_all(ctx, keep)
        ctx.set_option("HOST_CHUNK_MB", None)
        ctx.set_strict(False)
        r.close()


def test_extremes_bit_identical(ctx):
    """-32768 / 32767, the s24 limits, INT32_MIN / MAX and values that round (s32), each through a renderer with both buses"""
    M, layout, B, T = 13, "0+5+0", 256, 2
    N = len(LAYOUTS[layout])
    r = make_renderer(ctx, M, layout, B, T, scenes.ragged_curves(M, N, T * B, seed=47))
    rng = np.random.default_rng(11)
    keep = []
    try:
        for fmt in ("s16", "s24", "s32"):
            x = pcm_model.random_frames(rng, fmt, T * B, M + 3, extremes=True)
            want, got, _ = render_pair(ctx, r, x, fmt, 3, False, False, [T], keep)
            assert bits_equal(got, want), fmt
    finally:
        r.close()


def test_f32_nan_inf_denormal_pass_through(ctx):
    """f32 frames holding NaN payloads, infinities and denormals, on a direct-bus-only renderer: bitwise what
    earhip_render_process makes of the same floats (the conversion moves the bits), finite denormal inputs included"""
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
    raw[:, 1:3] = np.resize(special, raw[:, 1:3].shape)  # (channels 1, 2: the specials; the others: random bits)
    fin = np.random.default_rng(14).uniform(-1, 1, size=(n, M + 2)).astype(np.float32)
    fin[::3, 1] = np.array([1e-40, -3e-42, 1.4e-45], np.float32)[np.arange(fin[::3, 1].size) % 3]
    keep = []
    try:
        for x in (raw.view(np.float32), fin):
            want, got, _ = render_pair(ctx, r, x, "f32", 1, False, False, [T], keep)
            assert bits_equal(got, want)
    finally:
        r.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_form_bit_identical_to_process_device(ctx, fmt):
    """earhip_render_process_frames_device against earhip_render_process_device on the converted rows (in_stride = frames), planar and
    interleaved outputs (frame stride N + 2); s24 frames starting at an odd byte; two consecutive calls"""
    import torch
    M, layout, B, T = 29, "0+5+0", 512, 8
    N = len(LAYOUTS[layout])
    n = T * B
    r = make_renderer(ctx, M, layout, B, T, scenes.ragged_curves(M, N, 2 * n, seed=49))
    rng = np.random.default_rng(17)
    C_, first = M + 3, 1
    x = pcm_model.random_frames(rng, fmt, 2 * n, C_, extremes=True)
    rows = torch.from_numpy(pcm_model.rows(x, fmt, first, M)).cuda()
    shift = 1 if fmt == "s24" else 0
    raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    buf = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
    buf[shift:shift + raw.size] = torch.from_numpy(raw).cuda()
    fbytes = n * raw.size // (2 * n)
    try:
        r.reset(0)
        want = []
        for k in range(2):
            part = rows[:, k * n:(k + 1) * n].contiguous()
            o = torch.empty((N, n), dtype=torch.float32, device="cuda")
            r.process_device(T, part.data_ptr(), n, o.data_ptr(), n)
            want.append(o)
        ctx.synchronize()
        want = torch.cat(want, 1).cpu().numpy()
        for interleaved in (False, True):
            r.reset(0)
            got = []
            for k in range(2):
                ptr = buf.data_ptr() + shift + k * fbytes
                if interleaved:
                    o = torch.full((n, N + 2), -7.0, dtype=torch.float32, device="cuda")
                    r.process_frames_device(T, ptr, fmt, C_, first, o.data_ptr(), N + 2, True)
                    got.append(o)
                else:
                    o = torch.empty((N, n), dtype=torch.float32, device="cuda")
                    r.process_frames_device(T, ptr, fmt, C_, first, o.data_ptr(), n, False)
                    got.append(o)
            ctx.synchronize()
            if interleaved:
                g = torch.cat(got, 0).cpu().numpy()
                assert (g[:, N:] == -7.0).all()  # (the stride's padding untouched)
                g = g[:, :N].T
            else:
                g = torch.cat(got, 1).cpu().numpy()
            assert bits_equal(g, want), (fmt, interleaved)
    finally:
        r.close()


def test_two_renderers_share_one_frame_buffer(ctx):
    """the sharded use: two renderers take channels [0, 30) and [30, 61) of the same s16 frames; their sum against one renderer of
    all 61 channels, within the 1e-6 relative-RMS bar (the summation order differs), short and long calls"""
    M1, M2, layout, B, T = 30, 31, "0+5+0", 512, 140
    N = len(LAYOUTS[layout])
    curves = scenes.ragged_curves(M1 + M2, N, T * B, seed=51)
    whole = make_renderer(ctx, M1 + M2, layout, B, T, curves)
    a = make_renderer(ctx, M1, layout, B, T, curves[:M1])
    b = make_renderer(ctx, M2, layout, B, T, curves[M1:])
    x = pcm_model.random_frames(np.random.default_rng(19), "s16", T * B, M1 + M2)
    try:
        for nb in (3, T):
            xs = np.ascontiguousarray(x[:nb * B])
            for rr in (whole, a, b):
                rr.reset(0)
            ref = whole.process_frames(xs, "s16", 0)
            s = a.process_frames(xs, "s16", 0) + b.process_frames(xs, "s16", M1)
            err = scenes.rel_rms_per_channel(s, ref)
            assert err <= 1e-6, (nb, err)
            print(f"sharded {nb} blocks: worst channel rel RMS {err:.3e}")
    finally:
        for rr in (whole, a, b):
            rr.close()


def test_every_error_case_leaves_out_untouched(ctx):
    from libear_amd import capi
    lib = capi.load()
    M, layout, B, T = 13, "0+5+0", 256, 2
    N = len(LAYOUTS[layout])
    n = T * B
    r = make_renderer(ctx, M, layout, B, T, scenes.ragged_curves(M, N, n, seed=53))
    raw = np.zeros(n * (M + 3) * 4 + 64, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data % 16)
    out = np.full((N, n), 3.25, np.float32)
    ptrs = capi._chan_ptrs(out)
    null_row = capi._chan_ptrs(out)
    null_row[2] = capi.f32p()

    def call(nblocks=T, frames=base, fmt=1, C_=M + 3, first=0, o=ptrs, ilv=0):
        return lib.earhip_render_process_frames(r.h, C.c_size_t(nblocks), C.c_void_p(frames), C.c_int(fmt), C.c_int(C_), C.c_int(first),
                                                o, ilv)
    cases = {
        "unknown format 0": dict(fmt=0), "unknown format 5": dict(fmt=5), "first < 0": dict(first=-1),
        "first + M > C": dict(first=4), "C < M": dict(C_=M - 1), "NULL frames": dict(frames=None), "NULL out": dict(o=None),
        "NULL out row": dict(o=null_row), "nblocks > max_blocks": dict(nblocks=T + 1), "s16 misaligned": dict(frames=base + 1),
        "s32 misaligned": dict(fmt=3, frames=base + 2), "f32 misaligned": dict(fmt=4, frames=base + 1),
    }
    try:
        assert call() == capi.OK  # (the same arguments otherwise valid)
        out[...] = 3.25
        for name, kw in cases.items():
            assert call(**kw) == capi.INVALID_ARGUMENT, name
            assert (out == 3.25).all(), name
        assert call(fmt=2, frames=base + 1) == capi.OK  # s24 frames may start at any byte
        import torch
        dev = torch.full((N, n), 3.25, dtype=torch.float32, device="cuda")
        fr = torch.zeros(n * (M + 3) * 2 + 16, dtype=torch.uint8, device="cuda")

        def dcall(nblocks=T, frames=fr.data_ptr(), fmt=1, C_=M + 3, first=0, o=dev.data_ptr(), stride=n, ilv=0):
            return lib.earhip_render_process_frames_device(r.h, C.c_size_t(nblocks), C.c_void_p(frames), C.c_int(fmt), C.c_int(C_),
                                                            C.c_int(first), C.c_void_p(o), C.c_size_t(stride), ilv)
        dcases = {"unknown format": dict(fmt=7), "first < 0": dict(first=-1), "first + M > C": dict(first=4), "NULL frames": dict(frames=None),
                  "NULL out": dict(o=None), "nblocks > max_blocks": dict(nblocks=T + 1), "s16 misaligned": dict(frames=fr.data_ptr() + 1),
                  "planar stride": dict(stride=n - 1), "interleaved stride": dict(stride=N - 1, ilv=1)}
        for name, kw in dcases.items():
            assert dcall(**kw) == capi.INVALID_ARGUMENT, name
        ctx.synchronize()
        assert (dev == 3.25).all()
    finally:
        r.close()
