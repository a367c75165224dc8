"""CPU checks of the interleaved-frames input of the Objects renderer (include/earhip.h: earhip_render_process_frames): the numpy
model of the header's conversion against hand-computed values, the contiguous staging copy and the shared chunk plan of
libear_amd/csrc/host_gather.h built and run on the CPU (tests/cpp/test_host_gather_frames.cpp), and the new symbols declared and
exported."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import pcm_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_model_s16_by_hand():
    x = np.array([[0, 1, -1, 32767, -32768, 16384]], np.int16)
    want = np.array([[0.0, 2.0 ** -15, -(2.0 ** -15), 32767 / 32768, -1.0, 0.5]], np.float32)
    assert np.array_equal(bits(pcm_model.to_float(x, "s16")), bits(want))


def test_model_s24_by_hand_sign_extension_included():
    b = np.array([[0x00, 0x00, 0x00, 0x01, 0x00, 0x00, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x7F, 0x00, 0x00, 0x80, 0x56, 0x34, 0x12,
                   0x00, 0x00, 0xC0]], np.uint8)
    want = np.array([[0.0, 2.0 ** -23, -(2.0 ** -23), (2 ** 23 - 1) / 2 ** 23, -1.0, 0x123456 / 2 ** 23, -0.5]], np.float32)
    got = pcm_model.to_float(b, "s24")
    assert got.shape == (1, 7)
    assert np.array_equal(bits(got), bits(want))
    v = np.array([[0, 1, -1, (1 << 23) - 1, -(1 << 23), 0x123456, -(1 << 22)]])
    assert np.array_equal(pcm_model.s24_pack(v), b)


def test_model_s32_by_hand_round_to_nearest_even():
    x = np.array([[0, 1, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 30 + 64, 2 ** 30 + 192]], np.int64).astype(np.int32)
    want = np.array([[0.0, 2.0 ** -31, -(2.0 ** -31), 1.0, -1.0, 2.0 ** -7, (2 ** 24 + 4) / 2 ** 31, 0.5, (2 ** 30 + 256) / 2 ** 31]],
                    np.float32)
    assert np.array_equal(bits(pcm_model.to_float(x, "s32")), bits(want))


def test_model_f32_passes_the_bits():
    raw = np.array([[0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000, 0x3F800000]], np.uint32)
    got = pcm_model.to_float(raw.view(np.float32), "f32")
    assert np.array_equal(got.view(np.uint32), raw)


def test_model_selects_the_channel_range():
    x = np.arange(5 * 9, dtype=np.int16).reshape(5, 9)
    r = pcm_model.rows(x, "s16", 3, 4)
    assert r.shape == (4, 5) and r.flags["C_CONTIGUOUS"]
    assert np.array_equal(r, (x[:, 3:7].T.astype(np.float32) * np.float32(2.0 ** -15)))


def test_contiguous_staging_copy_and_shared_chunk_plan_on_cpu(tmp_path):
    """host_gather.h: stream_copy_bytes == memcpy, range_slice tiles a range, the staging threads' sliced chunk copy == one memcpy,
    and plan_host_chunks == the plan earhip_render_process made inline (a sweep of B, M, nblocks, pinned / pageable, options),
    under ASan + UBSan"""
    exe = tmp_path / "test_host_gather_frames"
    src = os.path.join(ROOT, "tests", "cpp", "test_host_gather_frames.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libear_amd", "csrc"), src, "-o", str(exe), "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    m = re.search(r"(\d+) plans \((\d+) long, (\d+) of 3\+ chunks\) checked: 0 problem", res.stdout)
    assert m and int(m.group(2)) > 1000 and int(m.group(3)) > 100, res.stdout


def test_decorrelator_stage_decisions_on_cpu(tmp_path):
    """decor_plan.h: the partition size, partition count, run length and kernel choice of the renderer's decorrelator stage and
    the wave kernel's run length == what the renderer decided inline before the header existed (tests/golden/decor_plan.txt: block
    sizes 16 ... 4096, FIRs of 1 ... 2048 taps, options K2_OWN_BLOCK, K2_WG and RUN; calls of 1 ... 4096 blocks on 1 ... 24
    loudspeakers and 1 ... 256 CUs), under ASan + UBSan"""
    exe = tmp_path / "test_decor_plan"
    src = os.path.join(ROOT, "tests", "cpp", "test_decor_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "libear_amd", "csrc"), src, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "decor_plan.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, env=env)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert "144 run lengths, 540 plans, 0 failed" in res.stdout, res.stdout


def test_frames_symbols_declared_and_exported():
    from libear_amd import build, lib_path
    text = open(os.path.join(ROOT, "include", "earhip.h")).read()
    for name in ("earhip_render_process_frames", "earhip_render_process_frames_device"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    for name, v in (("EARHIP_PCM_S16", 1), ("EARHIP_PCM_S24", 2), ("EARHIP_PCM_S32", 3), ("EARHIP_PCM_F32", 4)):
        assert re.search(r"\b" + name + r"\s*=\s*" + str(v) + r"\b", text), name
    build()
    lib = C.CDLL(lib_path())
    assert hasattr(lib, "earhip_render_process_frames") and hasattr(lib, "earhip_render_process_frames_device")


def test_frames_refuse_bad_arguments_without_a_device():
    """argument checks come before any device work: a NULL renderer is INVALID_ARGUMENT on any machine"""
    from libear_amd import capi
    lib = capi.load()
    buf = (C.c_int16 * 64)()
    out = (C.POINTER(C.c_float) * 1)()
    assert lib.earhip_render_process_frames(None, C.c_size_t(1), buf, 1, 4, 0, out, 0) == capi.INVALID_ARGUMENT
    assert lib.earhip_render_process_frames_device(None, C.c_size_t(1), buf, 1, 4, 0, None, C.c_size_t(0), 0) == capi.INVALID_ARGUMENT
