"""The block timeline (include/earhip.h group W) without a device: earhip_timeline_points and earhip_timeline_window are pure host
functions of the library, held here to tests/timeline_model.py — the rule as a point list (a), point for point, and the gain of
every sample stated directly (b), through libear's point semantics — in exact integer and Fraction arithmetic.  No tolerance
appears: everything compared is an integer or an exact fraction.

The renderer's setters need a renderer and so a device: their refusals that a NULL renderer cannot show, and the bulk setter
leaving every curve alone when it refuses one track, are in tests/test_gpu_timeline.py on the renderer itself and in
tests/test_timeline_host_cpu.py on the setters' own code (libear_amd/csrc/timeline.h) under ASan and UBSan."""
import numpy as np
import pytest

import timeline_model as model
from libear_amd import capi

CASES = model.all_cases()
NAMED = sorted(model.NAMED)


def native_points(mode, start, blocks, t0=model.INT64_MIN, t1=model.INT64_MAX):
    times, source = capi.timeline_points(mode, start, blocks, t0, t1)
    return list(zip(times.tolist(), source.tolist()))


@pytest.mark.parametrize("name", NAMED)
def test_named_case_equals_the_rule_point_for_point(name):
    mode, start, blocks = CASES[name]
    got = native_points(mode, start, blocks)
    assert got == model.points(mode, start, blocks)
    assert len(got) <= 5 * len(blocks) + 1


@pytest.mark.parametrize("name", NAMED)
def test_named_case_equals_the_gain_of_every_sample(name):
    mode, start, blocks = CASES[name]
    rows = model.rows_of(blocks)
    pts = native_points(mode, start, blocks)
    for n in model.span(start, blocks):
        assert model.evaluate(pts, rows, n) == model.gain_at(mode, start, blocks, rows, n), n


def test_random_lists_equal_the_rule_and_the_gain_of_every_sample():
    """200 lists of 1 to 12 blocks with durations of 1 to 40 samples: gaps, jumps of every length, open ends, both modes"""
    seen_open = seen_gap = seen_jump = 0
    for name, (mode, start, blocks) in CASES.items():
        if not name.startswith("random"):
            continue
        rows = model.rows_of(blocks)
        pts = native_points(mode, start, blocks)
        assert pts == model.points(mode, start, blocks), name
        assert len(pts) <= 5 * len(blocks) + 1
        for n in model.span(start, blocks):
            assert model.evaluate(pts, rows, n) == model.gain_at(mode, start, blocks, rows, n), (name, n)
        seen_open += blocks[-1][1] == model.OPEN
        seen_gap += any(blocks[i + 1][0] > blocks[i][0] + blocks[i][1] for i in range(len(blocks) - 1))
        seen_jump += any(b[2] for b in blocks[1:])
    assert seen_open >= 10 and seen_gap >= 50 and seen_jump >= 50


def test_what_the_rule_means_for_the_boundaries():
    """the two silent mistakes, stated on a case by hand: no ramp into the first block and not one sample of the previous
    gains too many"""
    mode, start, blocks = model.INTERPOLATED, 0, [(4, 6, 0, -1), (10, 4, 1, 2), (20, 5, 0, -1)]
    rows = [1.0, 3.0, 5.0]
    pts = native_points(mode, start, blocks)
    g = [model.evaluate(pts, rows, n) for n in range(0, 30)]
    assert g[:4] == [0] * 4 and g[4:10] == [1] * 6  # silence, then the first block at once
    assert g[10:14] == [1, 2, 3, 3]  # a jump of 2: the previous gains at s, the block's from s + 2
    assert g[14:20] == [0] * 6  # the gap
    assert g[20:25] == [3 + (5 - 3) * model.Fraction(k, 5) for k in range(5)]  # ramp over the whole block from the row before the gap
    assert g[25:] == [0] * 5


def test_windows_equal_the_whole_list_on_their_samples_and_name_their_blocks():
    """every case, 20 windows each: on [t0, t1) the windowed points give (b) of the whole list, and earhip_timeline_window names
    exactly the blocks whose rows the points use"""
    rng = np.random.default_rng(7)
    narrowed = 0
    for name, (mode, start, blocks) in CASES.items():
        rows = model.rows_of(blocks)
        for t0, t1 in model.random_windows(rng, start, blocks):
            pts = native_points(mode, start, blocks, t0, t1)
            assert pts == model.points(mode, start, blocks, t0, t1), (name, t0, t1)
            first, last = capi.timeline_window(mode, start, blocks, t0, t1)
            assert (first, last) == model.window(start, blocks, t0, t1)
            assert sorted({src for _, src in pts if src >= 0}) == list(range(first, last + 1)), (name, t0, t1)
            for n in range(t0, t1):
                assert model.evaluate(pts, rows, n) == model.gain_at(mode, start, blocks, rows, n), (name, t0, t1, n)
            narrowed += last - first + 1 < len(blocks)
    assert narrowed >= 500
    # the widest window is the whole list
    mode, start, blocks = CASES["a gap"]
    assert capi.timeline_window(mode, start, blocks) == (0, len(blocks) - 1)
    assert native_points(mode, start, blocks, model.INT64_MIN, model.INT64_MAX) == model.points(mode, start, blocks)


def test_counting_and_capacity():
    import ctypes as C
    mode, start, blocks = CASES["a gap"]
    b = capi.block_timings(blocks)
    want = model.points(mode, start, blocks)
    lib, n = capi.load(), C.c_int(-1)
    args = (C.c_int(mode), C.c_int64(start), C.c_int(len(b)), C.c_void_p(b.ctypes.data), C.c_int64(model.INT64_MIN), C.c_int64(model.INT64_MAX))
    assert lib.earhip_timeline_points(*args, C.c_int(0), None, None, C.byref(n)) == capi.OK and n.value == len(want)
    times, source = np.full(len(want) + 2, -7, np.int64), np.full(len(want) + 2, -7, np.int32)
    tp, sp = C.c_void_p(times.ctypes.data), C.c_void_p(source.ctypes.data)
    assert lib.earhip_timeline_points(*args, C.c_int(len(want) - 1), tp, sp, C.byref(n)) == capi.INVALID_ARGUMENT
    assert (times == -7).all() and (source == -7).all()
    assert lib.earhip_timeline_points(*args, C.c_int(len(want) + 2), tp, sp, C.byref(n)) == capi.OK and n.value == len(want)
    assert list(zip(times[:n.value].tolist(), source[:n.value].tolist())) == want
    assert (times[n.value:] == -7).all() and (source[n.value:] == -7).all()
    assert lib.earhip_timeline_points(*args, C.c_int(len(want)), None, sp, C.byref(n)) == capi.INVALID_ARGUMENT
    assert lib.earhip_timeline_points(*args, C.c_int(-1), tp, sp, C.byref(n)) == capi.INVALID_ARGUMENT


GOOD = [(0, 10, 0, -1), (10, 8, 1, 3), (18, 5, 0, -1)]
REFUSALS = {
    "rtime < 0": (0, 0, [(-1, 10, 0, -1)] + GOOD[1:], "block 0"),
    "duration == 0": (0, 0, [GOOD[0], (10, 0, 1, 0), GOOD[2]], "block 1"),
    "duration < -1": (0, 0, GOOD[:2] + [(18, -2, 0, -1)], "block 2"),
    "open end on a block that is not the last": (0, 0, [GOOD[0], (10, -1, 1, 3), GOOD[2]], "block 1"),
    "blocks overlap": (0, 0, [GOOD[0], (9, 8, 1, 3), GOOD[2]], "block 1"),
    "blocks out of order": (0, 0, [GOOD[0], GOOD[2], GOOD[1]], "block 2"),
    "jump_position not 0 or 1": (0, 0, [GOOD[0], (10, 8, 2, 3), GOOD[2]], "block 1"),
    "jump_position negative": (0, 0, [GOOD[0], (10, 8, -1, 3), GOOD[2]], "block 1"),
    "interpolation_length < -1": (0, 0, [GOOD[0], (10, 8, 1, -2), GOOD[2]], "block 1"),
    "L > duration": (0, 0, [GOOD[0], (10, 8, 1, 9), GOOD[2]], "block 1"),
    "open end without a jump after another block": (0, 0, GOOD[:2] + [(18, -1, 0, -1)], "block 2"),
    "unknown mode": (2, 0, GOOD, "mode"),
    "negative mode": (-1, 0, GOOD, "mode"),
    "no blocks": (0, 0, [], "n_blocks"),
    "start beyond 2^61": (0, 2 ** 61 + 1, GOOD, "start"),
    "rtime beyond 2^61": (0, 0, GOOD + [(2 ** 61 + 1, 5, 0, -1)], "block 3"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_by_status_code_and_block(name):
    mode, start, blocks, names = REFUSALS[name]
    for call in (capi.timeline_points, capi.timeline_window):
        with pytest.raises(capi.InvalidArgument) as info:
            call(mode, start, blocks)
        assert info.value.code == capi.INVALID_ARGUMENT and names in str(info.value), str(info.value)
    # refused on the whole list, whatever the window
    if blocks:
        with pytest.raises(capi.InvalidArgument):
            capi.timeline_points(mode, start, blocks, 0, 5)


def test_what_is_not_refused():
    # without a jump the interpolation length is not read; STEPPED reads neither jump field
    assert native_points(0, 0, [GOOD[0], (10, 8, 0, -5)]) == model.points(0, 0, [GOOD[0], (10, 8, 0, -5)])
    assert native_points(1, 0, [GOOD[0], (10, 8, 9, -5)]) == model.points(1, 0, [GOOD[0], (10, 8, 9, -5)])
    # a jump of the whole block, and an open first block
    assert native_points(0, 0, [GOOD[0], (10, 8, 1, 8)]) == model.points(0, 0, [GOOD[0], (10, 8, 1, 8)])
    assert native_points(0, 0, [(0, -1, 0, -1)]) == [(0, -1), (0, 0)]


def test_window_refusals_and_null_arguments():
    import ctypes as C
    for t0, t1 in ((5, 5), (6, 5), (model.INT64_MAX, model.INT64_MIN)):
        with pytest.raises(capi.InvalidArgument):
            capi.timeline_points(0, 0, GOOD, t0, t1)
        with pytest.raises(capi.InvalidArgument):
            capi.timeline_window(0, 0, GOOD, t0, t1)
    lib, n = capi.load(), C.c_int(0)
    lo, hi = C.c_int64(model.INT64_MIN), C.c_int64(model.INT64_MAX)
    assert lib.earhip_timeline_points(C.c_int(0), C.c_int64(0), C.c_int(3), None, lo, hi, C.c_int(0), None, None, C.byref(n)) == capi.INVALID_ARGUMENT
    b = capi.block_timings(GOOD)
    assert lib.earhip_timeline_points(C.c_int(0), C.c_int64(0), C.c_int(3), C.c_void_p(b.ctypes.data), lo, hi, C.c_int(0), None, None, None) == capi.INVALID_ARGUMENT
    assert lib.earhip_timeline_window(C.c_int(0), C.c_int64(0), C.c_int(3), C.c_void_p(b.ctypes.data), lo, hi, None, None) == capi.INVALID_ARGUMENT
    # the setters refuse a NULL renderer before anything else
    o, m, s, ofs = (C.c_int * 1)(0), (C.c_int * 1)(0), (C.c_int64 * 1)(0), (C.c_int64 * 2)(0, 3)
    d = np.zeros((3, 6), np.float32)
    dp = C.c_void_p(d.ctypes.data)
    assert lib.earhip_render_set_object_blocks(None, C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int(3), C.c_void_p(b.ctypes.data), lo, hi, dp, dp) == capi.INVALID_ARGUMENT
    assert lib.earhip_render_set_objects_blocks(None, C.c_int(1), o, m, s, ofs, C.c_void_p(b.ctypes.data), lo, hi, dp, dp) == capi.INVALID_ARGUMENT
