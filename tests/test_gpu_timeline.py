"""The block timeline (include/earhip.h group W) through the renderer on the GPU: 4 objects, 0+5+0 (6 channels), blocks of 64
samples, 32 blocks per call; every row of gains is an exact float32.  No tolerance appears anywhere: what is compared is either
exact by construction or bit-identical to the path that exists without the timeline.

  * Curves bound by earhip_render_set_objects_blocks render bit for bit as the same points set one object at a time by
    earhip_render_set_object_points from tests/timeline_model.py's points — two buses, default kernels, the same launch plan.
  * Bound in two windows of 16 blocks, a commit between them, the output is bit for bit that of the curves bound whole (both
    rendered in the same two calls of 16 blocks, so that nothing but the binding differs).
  * One bus, strict mode, one object, an input of 1.0f: the output IS the gain.  Every sample no block owns is +0.0 by its
    bits, every sample of a hold has the row's bits, every sample of a ramp its exact value (the ramps have power-of-two
    lengths here, so each is a float32), the first and last sample of each block on the right side of the boundary.
  * On the renderer itself: the bulk setter refusing track 2 of 3 leaves the curves of tracks 0 and 1 as they were."""
import numpy as np
import pytest

import timeline_model as model
from _hip import ctx
from layouts import LAYOUTS

pytestmark = pytest.mark.gpu

N, B, NBLOCKS = 6, 64, 32
SAMPLES = B * NBLOCKS


def make_blocks(rng, until, first_rtime, jumps, gaps, durations=(20, 150), lengths=None, open_end=False):
    """blocks from first_rtime to beyond `until`; jumps / gaps: the share of blocks with one"""
    blocks, t = [], first_rtime
    while t < until:
        duration = int(rng.integers(durations[0], durations[1] + 1)) if lengths is None else int(rng.choice(lengths))
        jump = int(bool(blocks) and rng.random() < jumps)
        if lengths is None:
            length = int(rng.integers(-1, duration + 1)) if jump else -1
        else:
            length = int(rng.choice([v for v in lengths if v <= duration] + [0])) if jump else -1
            duration += int(rng.integers(0, 40)) if jump else 0  # an odd hold behind a jump's ramp
        blocks.append((t, duration, jump, length))
        t += duration + (int(rng.integers(1, 90)) if rng.random() < gaps else 0)
    if open_end:
        rtime, duration, jump, length = blocks[-1]
        blocks[-1] = (rtime, model.OPEN, 1, max(length, 0))
    return blocks


def programme(seed=2127, exact_ramps=False):
    """(tracks [(object, mode, start, blocks)], block_offsets, direct, diffuse): contiguous without jumps; with jumps, ending
    early; with gaps, jumps and a negative start; a stepped bed with gaps and an open end"""
    rng = np.random.default_rng(seed)
    lengths = [1, 2, 4, 8, 16, 32, 64] if exact_ramps else None
    tracks = [(0, model.INTERPOLATED, 0, make_blocks(rng, SAMPLES + 100, 0, 0.0, 0.0, lengths=lengths)),
              (1, model.INTERPOLATED, 37, make_blocks(rng, SAMPLES - 300, 0, 0.6, 0.0, lengths=lengths)),
              (2, model.INTERPOLATED, -50, make_blocks(rng, SAMPLES + 100, 70, 0.4, 0.4, lengths=lengths)),
              (3, model.STEPPED, 5, make_blocks(rng, SAMPLES - 500, 11, 0.3, 0.3, lengths=lengths, open_end=True))]
    offsets = np.cumsum([0] + [len(t[3]) for t in tracks])
    sign = rng.choice([-1.0, 1.0], (offsets[-1], N))
    direct = (sign * rng.integers(1, 17, (offsets[-1], N)) / 8).astype(np.float32)
    diffuse = (rng.integers(-16, 17, (offsets[-1], N)) / 16).astype(np.float32)
    return tracks, offsets, direct, diffuse


def bind_blocks(r, prog, t0=model.INT64_MIN, t1=model.INT64_MAX):
    tracks, offsets, direct, diffuse = prog
    r.set_objects_blocks([t[0] for t in tracks], [t[1] for t in tracks], [t[2] for t in tracks], offsets,
                         [b for t in tracks for b in t[3]], direct, diffuse if r.K == 2 else None, t0, t1)


def bind_points(r, prog, t0=model.INT64_MIN, t1=model.INT64_MAX):
    """the same curves by hand: the model's points, a block's row or zeros for each, one set_object_points call per object"""
    tracks, offsets, direct, diffuse = prog
    for (obj, mode, start, blocks), first in zip(tracks, offsets):
        pts = model.points(mode, start, blocks, t0, t1)
        d = np.array([direct[first + src] if src >= 0 else np.zeros(N, np.float32) for _, src in pts], np.float32)
        f = np.array([diffuse[first + src] if src >= 0 else np.zeros(N, np.float32) for _, src in pts], np.float32)
        r.set_object_points(obj, [t for t, _ in pts], d, f if r.K == 2 else None)


def render(steps, x, two_buses=True):
    """steps: [(bind(r), blocks to process)] -> (output, the launch plan of each call)"""
    from libear_amd import capi
    dec = capi.design_decorrelators(LAYOUTS["0+5+0"]) if two_buses else None
    r = capi.Renderer(ctx(), x.shape[0], N, B, dec, 255 if two_buses else 0, max_blocks=NBLOCKS)
    out, plans, at = [], [], 0
    for bind, nblocks in steps:
        bind(r)
        r.commit()
        out.append(r.process(x[:, at:at + nblocks * B]))
        plans.append(r.last_plan())
        at += nblocks * B
    r.close()
    return np.concatenate(out, axis=1), plans


@pytest.fixture(scope="module")
def audio():
    return np.random.default_rng(5).uniform(-1, 1, (4, SAMPLES)).astype(np.float32)


@pytest.fixture(scope="module")
def whole(audio):
    """the programme bound whole by the new setter and rendered in one call: shared, never changed"""
    prog = programme()
    out, plans = render([(lambda r: bind_blocks(r, prog), NBLOCKS)], audio)
    out.setflags(write=False)
    return prog, out, plans


def test_blocks_render_bit_for_bit_as_the_models_points_set_by_hand(audio, whole):
    prog, got, plans = whole
    want, want_plans = render([(lambda r: bind_points(r, prog), NBLOCKS)], audio)
    assert np.abs(want).max() > 0.1 and np.isfinite(want).all()
    assert got.tobytes() == want.tobytes()
    assert plans == want_plans


def test_the_single_form_is_the_bulk_form(audio, whole):
    prog, want, plans = whole
    tracks, offsets, direct, diffuse = prog

    def bind(r):
        for (obj, mode, start, blocks), first in zip(tracks, offsets):
            r.set_object_blocks(obj, mode, start, blocks, direct[first:first + len(blocks)], diffuse[first:first + len(blocks)])

    got, got_plans = render([(bind, NBLOCKS)], audio)
    assert got.tobytes() == want.tobytes() and got_plans == plans


def test_two_windows_render_bit_for_bit_as_the_whole_timeline(audio):
    prog = programme()
    half = NBLOCKS // 2
    windows = [(0, half * B), (half * B, SAMPLES)]
    want, _ = render([(lambda r: bind_blocks(r, prog), half), (lambda r: None, half)], audio)
    got, _ = render([(lambda r, w=w: bind_blocks(r, prog, *w), half) for w in windows], audio)
    by_hand, _ = render([(lambda r, w=w: bind_points(r, prog, *w), half) for w in windows], audio)
    # the windows do narrow the curves: fewer blocks than the whole list, for every track
    for obj, mode, start, blocks in prog[0]:
        for w in windows:
            first, last = model.window(start, blocks, *w)
            assert last - first + 1 < len(blocks)
    assert got.tobytes() == by_hand.tobytes()
    assert got.tobytes() == want.tobytes()


def test_the_gain_itself_in_strict_mode():
    from libear_amd import capi
    tracks, offsets, direct, _ = programme(seed=9, exact_ramps=True)
    x = np.ones((1, SAMPLES), np.float32)
    zero = np.zeros(N, np.float32).tobytes()
    silent = holds = ramped = 0
    ctx().set_strict(True)
    try:
        for (obj, mode, start, blocks), first in zip(tracks, offsets):
            rows = direct[first:first + len(blocks)]
            r = capi.Renderer(ctx(), 1, N, B, None, 0, max_blocks=NBLOCKS)
            r.set_object_blocks(0, mode, start, blocks, rows)
            out = r.process(x)
            r.close()
            for n in range(SAMPLES):
                own, got = model.owner(mode, start, blocks, n), np.ascontiguousarray(out[:, n])
                if own is None:
                    assert got.tobytes() == zero, (obj, n)
                    silent += 1
                elif own[1] == 1:
                    assert got.tobytes() == rows[own[0]].tobytes(), (obj, n)
                    holds += 1
                else:
                    b, p = own
                    want = rows[b - 1].astype(np.float64) + float(p) * (rows[b].astype(np.float64) - rows[b - 1].astype(np.float64))
                    assert (want.astype(np.float32).astype(np.float64) == want).all()  # exact by construction
                    assert np.array_equal(got, want.astype(np.float32)), (obj, n)
                    ramped += 1
            # the boundaries, said once more on their own: the block's first sample still has the gains it starts from — the
            # previous block's, or its own where nothing ramps —, the sample before it is the previous block's or silence, its
            # last sample is its own and the sample after its end is not
            for b, (rtime, duration, jump, length) in enumerate(blocks):
                s = start + rtime
                ramps = mode == model.INTERPOLATED and b > 0 and model.ramp(blocks[b]) > 0
                if 0 <= s < SAMPLES:
                    assert out[:, s].tobytes() == rows[b - 1 if ramps else b].tobytes(), (obj, b)
                if 0 <= s - 1 < SAMPLES and (b == 0 or s > start + blocks[b - 1][0] + blocks[b - 1][1]):
                    assert out[:, s - 1].tobytes() == zero, (obj, b)
                if duration == model.OPEN:
                    assert out[:, SAMPLES - 1].tobytes() == rows[b].tobytes()
                    continue
                e = s + duration
                if 0 <= e - 1 < SAMPLES:
                    assert model.owner(mode, start, blocks, e - 1)[0] == b and out[:, e - 1].tobytes() != zero, (obj, b)
                    if not ramps or model.ramp(blocks[b]) < duration:
                        assert out[:, e - 1].tobytes() == rows[b].tobytes(), (obj, b)
                if 0 <= e < SAMPLES and (b == len(blocks) - 1 or start + blocks[b + 1][0] > e):
                    assert out[:, e].tobytes() == zero, (obj, b)
    finally:
        ctx().set_strict(False)
    assert silent > 1000 and holds > 2000 and ramped > 2000, (silent, holds, ramped)  # of the 4 x 2048 samples


def test_a_refused_bulk_call_leaves_the_curves_as_they_were(audio, whole):
    from libear_amd import capi
    prog, want, _ = whole
    tracks, offsets, direct, diffuse = prog
    dec = capi.design_decorrelators(LAYOUTS["0+5+0"])
    r = capi.Renderer(ctx(), 4, N, B, dec, 255, max_blocks=NBLOCKS)
    bind_blocks(r, prog)
    r.commit()
    assert r.process(audio).tobytes() == want.tobytes()
    # tracks 0 and 1 with other rows, track 2 with two blocks that overlap
    three = tracks[:3]
    bad = list(three[2][3])
    bad[1] = (bad[0][0] + bad[0][1] - 1,) + bad[1][1:]
    broken = three[:2] + [(2, model.INTERPOLATED, three[2][2], bad)]
    with pytest.raises(capi.InvalidArgument) as info:
        bind_blocks(r, (broken, offsets[:4], -direct[:offsets[3]], diffuse[:offsets[3]]))
    assert str(info.value).startswith("track 2: block 1:"), str(info.value)
    with pytest.raises(capi.InvalidArgument):
        r.set_object_blocks(7, 0, 0, three[0][3], direct[:offsets[1]], diffuse[:offsets[1]])
    r.commit()
    r.reset(0)
    assert r.process(audio).tobytes() == want.tobytes()
    # and the same call with track 2 as it was does change them
    bind_blocks(r, (three, offsets[:4], -direct[:offsets[3]], diffuse[:offsets[3]]))
    r.commit()
    r.reset(0)
    assert r.process(audio).tobytes() != want.tobytes()
    r.close()
