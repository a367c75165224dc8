"""The block timeline's core without the library: libear_amd/csrc/timeline.h — the checks, the window, the rule and the code of
the renderer's two setters (timeline_bind) — compiled by plain g++ under ASan and UBSan (tests/cpp/timeline_host.cpp), run
directly as a program, and held to tests/timeline_model.py: the named cases and windows on them point for point, every
refusal, and the setters' rows and all-or-nothing rule against a sink that records what would have reached the curves."""
import os
import struct
import subprocess

import numpy as np
import pytest

import timeline_model as model
from test_timeline_cpu import GOOD, REFUSALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("timeline_host") / "timeline_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "timeline_host.cpp"), "-o", str(path)], check=True)
    return str(path)


def pack_blocks(blocks):
    # earhip_block_timing: three int64, one int32, four bytes of padding
    return b"".join(struct.pack("<qqqi4x", b[0], b[1], b[3] if len(b) > 3 else -1, b[2] if len(b) > 2 else 0) for b in blocks)


def execute(exe, tmp_path, command, blob):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([exe, command, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert res.returncode == 0, res.stdout
    return dst.read_bytes()


def run_points(exe, tmp_path, cases):
    """cases: [(mode, start, blocks, t0, t1)] -> per case (first, last, [(time, src)]) or (status, text)"""
    blob = struct.pack("<i", len(cases))
    for mode, start, blocks, t0, t1 in cases:
        blob += struct.pack("<iiqqq", mode, len(blocks), start, t0, t1) + pack_blocks(blocks)
    out, at, results = execute(exe, tmp_path, "points", blob), 0, []
    for _ in cases:
        status, = struct.unpack_from("<i", out, at)
        if status != 0:
            n, = struct.unpack_from("<i", out, at + 4)
            results.append((status, out[at + 8:at + 8 + n].decode()))
            at += 8 + n
            continue
        first, last, n = struct.unpack_from("<3i", out, at + 4)
        times = np.frombuffer(out, np.int64, n, at + 16).tolist()
        source = np.frombuffer(out, np.int32, n, at + 16 + 8 * n).tolist()
        results.append((first, last, list(zip(times, source))))
        at += 16 + 12 * n
    assert at == len(out)
    return results


def run_bind(exe, tmp_path, n_objects, n_out, n_buses, tracks, direct, diffuse, t0=model.INT64_MIN, t1=model.INT64_MAX,
             max_points=2 ** 18 - 1, offsets=None):
    """tracks: [(object, mode, start, blocks)] -> (status, text, [(object, times, rows[npoints][n_buses * n_out])])"""
    blocks = [b for t in tracks for b in t[3]]
    offsets = offsets if offsets is not None else np.cumsum([0] + [len(t[3]) for t in tracks]).tolist()
    blob = struct.pack("<5i", n_objects, n_out, n_buses, max_points, len(tracks))
    blob += np.asarray([t[0] for t in tracks], np.int32).tobytes() + np.asarray([t[1] for t in tracks], np.int32).tobytes()
    blob += np.asarray([t[2] for t in tracks], np.int64).tobytes() + np.asarray(offsets, np.int64).tobytes()
    blob += struct.pack("<qqq", t0, t1, len(blocks)) + pack_blocks(blocks)
    blob += np.ascontiguousarray(direct, np.float32).tobytes()
    if n_buses == 2:
        blob += np.ascontiguousarray(diffuse, np.float32).tobytes()
    out = execute(exe, tmp_path, "bind", blob)
    status, n = struct.unpack_from("<2i", out)
    text = out[8:8 + n].decode()
    n_calls, = struct.unpack_from("<i", out, 8 + n)
    at, calls, cols = 12 + n, [], n_buses * n_out
    for _ in range(n_calls):
        obj, npoints = struct.unpack_from("<2i", out, at)
        times = np.frombuffer(out, np.int64, npoints, at + 8)
        rows = np.frombuffer(out, np.float32, npoints * cols, at + 8 + 8 * npoints).reshape(npoints, cols)
        calls.append((obj, times.tolist(), rows))
        at += 8 + 8 * npoints + 4 * npoints * cols
    assert at == len(out)
    return status, text, calls


def test_core_equals_the_rule_on_the_named_cases_and_their_windows(exe, tmp_path):
    rng = np.random.default_rng(11)
    cases = []
    for name in sorted(model.NAMED):
        mode, start, blocks = model.NAMED[name]
        cases.append((mode, start, blocks, model.INT64_MIN, model.INT64_MAX))
        cases += [(mode, start, blocks, t0, t1) for t0, t1 in model.random_windows(rng, start, blocks, 5)]
    got = run_points(exe, tmp_path, cases)
    for (mode, start, blocks, t0, t1), (first, last, pts) in zip(cases, got):
        assert (first, last) == model.window(start, blocks, t0, t1)
        assert pts == model.points(mode, start, blocks, t0, t1)
        rows = model.rows_of(blocks)
        lo, hi = (model.span(start, blocks)[0], model.span(start, blocks)[-1] + 1) if t0 == model.INT64_MIN else (t0, t1)
        for n in range(lo, hi):
            assert model.evaluate(pts, rows, n) == model.gain_at(mode, start, blocks, rows, n)


def test_core_refuses_what_the_header_lists(exe, tmp_path):
    names = sorted(REFUSALS)
    cases = [(REFUSALS[k][0], REFUSALS[k][1], REFUSALS[k][2], model.INT64_MIN, model.INT64_MAX) for k in names]
    cases += [(0, 0, GOOD, 5, 5), (0, 0, GOOD, 6, 5)]
    got = run_points(exe, tmp_path, cases)
    for k, result in zip(names, got):
        assert result[0] == INVALID_ARGUMENT and REFUSALS[k][3] in result[1], (k, result)
    assert got[-2][0] == got[-1][0] == INVALID_ARGUMENT and "t0 < t1" in got[-1][1]


def programme():
    """three tracks on four objects, six channels: Objects with a jump and a gap, a stepped bed, Objects with an open end"""
    tracks = [(2, model.INTERPOLATED, 100, [(0, 10, 0, -1), (10, 8, 1, 3), (25, 5, 0, -1)]),
              (0, model.STEPPED, 0, [(0, 64, 0, -1), (64, 64, 0, -1)]),
              (3, model.INTERPOLATED, -20, [(5, 10, 0, -1), (15, 7, 0, -1), (22, 9, 1, 0), (31, -1, 1, 4)])]
    total = sum(len(t[3]) for t in tracks)
    rng = np.random.default_rng(3)
    direct = rng.integers(-8, 9, (total, 6)).astype(np.float32) / 8 + 16
    diffuse = rng.integers(-8, 9, (total, 6)).astype(np.float32) / 8 - 16
    return tracks, direct, diffuse


@pytest.mark.parametrize("n_buses", [1, 2])
def test_the_setters_rows_are_the_blocks_rows_at_the_rules_points(exe, tmp_path, n_buses):
    tracks, direct, diffuse = programme()
    status, text, calls = run_bind(exe, tmp_path, 4, 6, n_buses, tracks, direct, diffuse)
    assert (status, text) == (0, "") and [c[0] for c in calls] == [t[0] for t in tracks]
    first = 0
    for (obj, mode, start, blocks), (_, times, rows) in zip(tracks, calls):
        pts = model.points(mode, start, blocks)
        assert times == [t for t, _ in pts]
        for (_, src), row in zip(pts, rows):
            want_d = direct[first + src] if src >= 0 else np.zeros(6, np.float32)
            want_f = diffuse[first + src] if src >= 0 else np.zeros(6, np.float32)
            want = np.concatenate([want_d, want_f]) if n_buses == 2 else want_d
            assert row.tobytes() == want.astype(np.float32).tobytes()  # bits: silence is +0.0
        first += len(blocks)


def test_the_setters_read_only_rows_of_selected_blocks(exe, tmp_path):
    tracks, direct, diffuse = programme()
    t0, t1 = 112, 118  # inside block 1 of track 0 and block 0 of track 1; after block 3 of track 2 has started
    first, keep = 0, np.zeros(len(direct), bool)
    for obj, mode, start, blocks in tracks:
        b0, b1 = model.window(start, blocks, t0, t1)
        keep[first + b0:first + b1 + 1] = True
        first += len(blocks)
    assert keep.sum() < len(keep)
    direct[~keep], diffuse[~keep] = np.nan, np.nan
    status, text, calls = run_bind(exe, tmp_path, 4, 6, 2, tracks, direct, diffuse, t0, t1)
    assert (status, text) == (0, "")
    for (obj, mode, start, blocks), (_, times, rows) in zip(tracks, calls):
        assert times == [t for t, _ in model.points(mode, start, blocks, t0, t1)]
        assert not np.isnan(rows).any()


def test_a_refused_track_leaves_every_curve_alone(exe, tmp_path):
    """the bulk form checks every track first: with track 2 of 3 refused, set_object is not called for tracks 0 and 1 either"""
    tracks, direct, diffuse = programme()
    for what, bad in (("overlap", [(5, 10, 0, -1), (14, 7, 0, -1), (22, 9, 1, 0), (31, -1, 1, 4)]),
                      ("open end without a jump", [(5, 10, 0, -1), (15, 7, 0, -1), (22, 9, 1, 0), (31, -1, 0, -1)]),
                      ("a hold of 2^31 samples", [(5, 10, 0, -1), (15, 7, 0, -1), (22, 9, 1, 0), (31, 2 ** 31 + 4, 1, 4)])):
        broken = tracks[:2] + [(3, model.INTERPOLATED, -20, bad)]
        status, text, calls = run_bind(exe, tmp_path, 4, 6, 2, broken, direct, diffuse)
        assert status == INVALID_ARGUMENT and text.startswith("track 2: block") and calls == [], (what, text)
    # an object out of range, a mode nobody knows, too many points for one curve, offsets that do not ascend
    status, text, calls = run_bind(exe, tmp_path, 3, 6, 2, tracks, direct, diffuse)
    assert status == INVALID_ARGUMENT and text.startswith("track 2: object") and calls == []
    status, text, calls = run_bind(exe, tmp_path, 4, 6, 2, tracks[:2] + [(3, 7, -20, tracks[2][3])], direct, diffuse)
    assert status == INVALID_ARGUMENT and text.startswith("track 2: unknown") and calls == []
    status, text, calls = run_bind(exe, tmp_path, 4, 6, 2, tracks, direct, diffuse, max_points=8)
    assert status == INVALID_ARGUMENT and text.startswith("track 0: too many") and "window" in text and calls == []  # (its 10 points)
    status, text, calls = run_bind(exe, tmp_path, 4, 6, 2, tracks, direct, diffuse, offsets=[0, 3, 5, 5])
    assert status == INVALID_ARGUMENT and text.startswith("track 2: n_blocks") and calls == []
    status, text, calls = run_bind(exe, tmp_path, 4, 6, 2, tracks, direct, diffuse, offsets=[1, 3, 5, 9])
    assert status == INVALID_ARGUMENT and text.startswith("track 0: block_offsets") and calls == []
    # ... and the same three tracks as they are reach the sink, the too-long curve bound by a window as well
    assert len(run_bind(exe, tmp_path, 4, 6, 2, tracks, direct, diffuse)[2]) == 3
    status, text, calls = run_bind(exe, tmp_path, 4, 6, 2, tracks, direct, diffuse, 0, 4, max_points=8)
    assert (status, text) == (0, "") and all(len(c[1]) <= 8 for c in calls)
