"""CPU checks of the PCM frames output of the Objects renderer (include/earhip.h: earhip_render_process_frames_pcm): the numpy
model of the header's conversion against values worked out by hand, round trips through the input model, the dither model's
properties, the shared conversion header (libear_amd/csrc/pcm_convert.h: the code the device kernel runs) compiled for the host
against the model bit for bit, and the new symbols declared and exported."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import pcm_model
import pcm_out_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_BELOW_ONE = np.array([0x3F7FFFFF], np.uint32).view(np.float32)[0]  # 0x1.fffffep-1f


def conv(values, fmt, **kw):
    q, c = om.from_float(np.array([values], np.float32), fmt, **kw)
    return q[0], c[0]


def test_model_s16_by_hand():
    lsb = 2.0 ** -15
    x = [0.0, lsb, -lsb, 0.5 * lsb, -0.5 * lsb, 1.5 * lsb, 2.5 * lsb, -1.5 * lsb, 32767 / 32768, 1.0, -1.0, 32767.5 / 32768,
         32767.25 / 32768, -32768.5 / 32768, -32768.75 / 32768, np.inf, -np.inf, np.nan, 1e30, -1e30, 1e-42]
    want = [0, 1, -1, 0, 0, 2, 2, -2, 32767, 32767, -32768, 32767, 32767, -32768, -32768, 32767, -32768, 0, 32767, -32768, 0]
    clip = [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0]
    q, c = conv(x, "s16")
    assert q.dtype == np.int16
    assert q.tolist() == want
    assert c.astype(int).tolist() == clip


def test_model_s24_by_hand_byte_order_and_sign():
    lsb = 2.0 ** -23
    x = [0.0, lsb, -lsb, 0.5 * lsb, 1.5 * lsb, 2.5 * lsb, 0x123456 * lsb, -0.5, (2 ** 23 - 1) * lsb, 1.0, -1.0, np.inf, -np.inf, np.nan]
    want = [0, 1, -1, 0, 2, 2, 0x123456, -(1 << 22), (1 << 23) - 1, (1 << 23) - 1, -(1 << 23), (1 << 23) - 1, -(1 << 23), 0]
    clip = [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 1]
    q, c = conv(x, "s24")
    assert q.dtype == np.uint8 and q.shape == (3 * len(x),)
    b = q.reshape(-1, 3)
    assert b[1].tolist() == [0x01, 0x00, 0x00] and b[2].tolist() == [0xFF, 0xFF, 0xFF]
    assert b[6].tolist() == [0x56, 0x34, 0x12] and b[7].tolist() == [0x00, 0x00, 0xC0]
    assert b[8].tolist() == [0xFF, 0xFF, 0x7F] and b[10].tolist() == [0x00, 0x00, 0x80]
    assert np.array_equal(q[None, :], pcm_model.s24_pack(np.array([want])))
    assert c.astype(int).tolist() == clip


def test_model_s32_by_hand_the_edge_is_compared_in_float():
    above_one = float(np.nextafter(np.float32(1), np.float32(2)))
    x = [0.0, 2.0 ** -31, -(2.0 ** -31), 0.5, F32_BELOW_ONE, 1.0, -1.0, -above_one, np.inf, -np.inf, np.nan, 2.0 ** -32, 3 * 2.0 ** -32]
    want = [0, 1, -1, 2 ** 30, 2147483520, 2147483647, -2147483648, -2147483648, 2147483647, -2147483648, 0, 0, 2]
    clip = [0, 0, 0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 0]
    q, c = conv(x, "s32")
    assert q.dtype == np.int32
    assert q.tolist() == want
    assert c.astype(int).tolist() == clip


def test_model_f32_passes_the_bits_and_never_clips():
    raw = np.array([[0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000, 0x40000000]], np.uint32)
    q, c = om.from_float(raw.view(np.float32), "f32")
    assert np.array_equal(q.view(np.uint32), raw) and not c.any()
    assert om.peak(raw.view(np.float32).reshape(-1, 1)).view(np.uint32).tolist() == [0x7F800000]  # (NaN ignored, inf is a level)


def test_round_trip_through_the_input_model():
    v = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16).reshape(-1, 8)
    q, c = om.from_float(pcm_model.to_float(v, "s16"), "s16")
    assert np.array_equal(q, v) and not c.any()
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.integers(-(1 << 23), 1 << 23, size=4000), [-(1 << 23), (1 << 23) - 1, 0, -1, 1]]).reshape(-1, 5)
    b = pcm_model.s24_pack(v)
    q, c = om.from_float(pcm_model.to_float(b, "s24"), "s24")
    assert np.array_equal(q, b) and not c.any()
    # s32: only values float32 holds exactly (24 significant bits), the extreme negative included
    m = rng.integers(-(1 << 23), 1 << 23, size=3999) << rng.integers(0, 8, size=3999)
    v = np.concatenate([m, [-(1 << 31)]]).astype(np.int32).reshape(-1, 4)
    q, c = om.from_float(pcm_model.to_float(v, "s32"), "s32")
    assert np.array_equal(q, v) and not c.any()


def _mix(a):
    a ^= a >> 16
    a = (a * 0x7FEB352D) & 0xFFFFFFFF
    a ^= a >> 15
    a = (a * 0x846CA68B) & 0xFFFFFFFF
    return a ^ (a >> 16)


def test_dither_model_is_a_pure_function_of_seed_clock_and_channel():
    rng = np.random.default_rng(6)
    t = rng.integers(-(1 << 40), 1 << 40, size=20000)
    n = rng.integers(0, 64, size=20000)
    d = om.dither(7, t, n)
    assert d.dtype == np.float32 and np.all(d > -1) and np.all(d < 1)
    assert abs(float(np.mean(d))) < 0.02 and abs(float(np.var(d)) - 1 / 6) < 0.01  # (TPDF over (-1, 1): variance 1/6)
    p = rng.permutation(t.size)
    assert np.array_equal(om.dither(7, t[p], n[p]), d[p])
    assert np.mean(om.dither(8, t, n) != d) > 0.99
    assert np.mean(om.dither(7, t + (1 << 32), n) != d) > 0.99  # (both halves of the clock are hashed)
    assert np.mean(om.dither(7, t, n + 1) != d) > 0.99
    assert np.mean(om.dither(7, t + 1, n) != d) > 0.99
    # by hand, in Python integers: seed 0, t 0, n 0, and a case with every word set
    h = _mix(_mix(_mix(_mix(0x9E3779B9))))
    assert int(om.dither_hash(0, 0, 0)) == h
    assert float(om.dither(0, 0, 0)) == ((h & 0xFFFF) + (h >> 16) - 65535) / 65536
    h = _mix(_mix((_mix(_mix((5 + 0x9E3779B9) & 0xFFFFFFFF) ^ 2) + 3 * 0x85EBCA6B) & 0xFFFFFFFF) ^ 9)
    assert int(om.dither_hash(9, (2 << 32) + 5, 3)) == h


def test_dither_of_silence_is_one_lsb_at_most_and_follows_the_clock():
    z = np.zeros((4096, 3), np.float32)
    q, c = om.from_float(z, "s16", dither_on=True, seed=3, t0=1000)
    assert set(np.unique(q).tolist()) == {-1, 0, 1} and not c.any()
    q2, _ = om.from_float(z[:100], "s16", dither_on=True, seed=3, t0=1500)
    assert np.array_equal(q2, q[500:600])
    q3, _ = om.from_float(z, "s16", dither_on=True, seed=4, t0=1000)
    assert not np.array_equal(q3, q)


def edge_values():
    e = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e38, -1e38, float(F32_BELOW_ONE), -float(F32_BELOW_ONE)]
    for bits in (15, 23, 31):
        lsb = 2.0 ** -bits
        for k in (0.5, 1.0, 1.5, 2.5, 3.5, 2.0 ** bits - 1, 2.0 ** bits - 0.5, 2.0 ** bits - 1.5, 2.0 ** bits + 0.5, 2.0 ** bits + 1):
            e += [k * lsb, -k * lsb]
    x = np.array(e, np.float32)
    return np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))])


def test_level_fold_on_the_host(tmp_path):
    """pcm_convert.h, pcm_levels_fold (what both output_levels calls return): 64 slots x 3 channels of chosen bit patterns and
    counts — the largest pattern per channel, the sum of the counts (one above 2^32), an all-zero channel — under ASan + UBSan"""
    exe = tmp_path / "test_pcm_levels"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libear_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_pcm_levels.cpp"), "-o", str(exe)],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(res.stdout)
    assert res.returncode == 0, res.stdout


def test_shared_conversion_header_on_the_host_equals_the_model(tmp_path):
    """pcm_convert.h, the function k_rows_to_pcm calls, built with the host compiler: every edge value and a few thousand random
    ones, all formats, with and without dither, bit for bit the model's samples, clip flags and hash values (the samples laid
    out as frames of 7 channels from a clock t0: from_float itself is what is compared)"""
    exe = tmp_path / "test_pcm_convert"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "libear_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_pcm_convert.cpp"), "-o", str(exe)], check=True)
    rng = np.random.default_rng(7)
    x = np.concatenate([edge_values(), rng.uniform(-1.5, 1.5, 3000).astype(np.float32),
                        (rng.integers(-40000, 40000, 2000) / 65536.0).astype(np.float32),  # (halves and quarters of an s16 LSB: ties)
                        rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    xb = x.view(np.uint32)
    N = 7
    lines, want = [], []
    for fmt, code, dith, seed, t0 in (("s16", 1, 0, 0, 0), ("s16", 1, 1, 99, 12345), ("s16", 1, 1, 0xFFFFFFFF, -(1 << 41) - 5),
                                      ("s24", 2, 0, 0, 0), ("s32", 3, 0, 5, 0)):
        pad = (-x.size) % N
        xs = np.concatenate([x, np.zeros(pad, np.float32)]).reshape(-1, N)
        q, c = om.from_float(xs, fmt, dither_on=bool(dith), seed=seed, t0=t0)
        if fmt == "s24":
            b = q.reshape(q.shape[0], N, 3).astype(np.int64)
            q = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
            q = np.where(q >= 1 << 23, q - (1 << 24), q)
        q, c = q.reshape(-1)[:x.size], c.reshape(-1)[:x.size]
        t = t0 + np.arange(xs.shape[0])[:, None] + np.zeros((1, N), np.int64)
        n = np.zeros((xs.shape[0], 1), np.int64) + np.arange(N)[None, :]
        t, n = t.reshape(-1)[:x.size], n.reshape(-1)[:x.size]
        h = om.dither_hash(seed, t, n)
        lines += ["%d %d %d %d %d %x" % (code, dith, seed, t[i], n[i], xb[i]) for i in range(x.size)]
        want += ["%d %d %08x" % (q[i], c[i], h[i]) for i in range(x.size)]
    res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True)
    got = res.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    bad = [(lines[i], got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:10]


def test_pcm_out_symbols_declared_and_exported():
    from libear_amd import build, lib_path
    text = open(os.path.join(ROOT, "include", "earhip.h")).read()
    names = ("earhip_render_process_frames_pcm", "earhip_render_process_frames_pcm_device", "earhip_render_output_levels")
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert re.search(r"\}\s*earhip_pcm_out\s*;", text)
    build()
    lib = C.CDLL(lib_path())
    for name in names:
        assert hasattr(lib, name), name


def test_pcm_out_refuses_bad_arguments_without_a_device():
    """argument checks come before any device work: a NULL renderer is INVALID_ARGUMENT on any machine"""
    from libear_amd import capi
    lib = capi.load()
    buf = (C.c_int16 * 64)()
    out = (C.c_int16 * 64)()
    spec = capi.PcmOut(1, 0, 0)
    assert lib.earhip_render_process_frames_pcm(None, C.c_size_t(1), buf, 1, 4, 0, out, C.byref(spec)) == capi.INVALID_ARGUMENT
    assert lib.earhip_render_process_frames_pcm_device(None, C.c_size_t(1), buf, 1, 4, 0, out, C.c_size_t(8), C.c_size_t(0),
                                                       C.byref(spec)) == capi.INVALID_ARGUMENT
    peak, clipped = (C.c_float * 4)(), (C.c_uint64 * 4)()
    assert lib.earhip_render_output_levels(None, peak, clipped, 0) == capi.INVALID_ARGUMENT
    assert not any(out)
