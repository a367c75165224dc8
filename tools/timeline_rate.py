"""Cost of binding a programme's block timeline to the renderer's curves (include/earhip.h group W): one
earhip_render_set_objects_blocks call for all objects + earhip_render_commit, next to the loop it replaces — one
earhip_render_set_object_points call per object over the same points, built by earhip_timeline_points outside the timed region,
+ the same commit — in the same run; one JSON line.  Both go through the ctypes binding, as a caller's would: the loop pays one
foreign call per object, with its arrays made beforehand.

The workload: 1024 objects x 220 blocks each on 9+10+3 (24 channels), two buses.  A third of the objects have contiguous blocks
without jumps, a third jumps (interpolationLength from 0 to the block), a third gaps between blocks.  Blocks per second counts
the blocks of all objects; the median of 5 alternating rounds and their spread.

usage: python tools/timeline_rate.py [objects (1024)] [blocks per object (220)] [layout (9+10+3)]"""
import json
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: it ships its own HIP runtime, which the library then binds to)

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from libear_amd import capi  # noqa: E402

n_objects = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
per_object = int(sys.argv[2]) if len(sys.argv) > 2 else 220
layout = sys.argv[3] if len(sys.argv) > 3 else "9+10+3"
names = [c[0] for c in capi.layout_channels(layout)]
n_out, block_size = len(names), 512
rng = np.random.default_rng(2127)

blocks = np.zeros(n_objects * per_object, capi.BLOCK_TIMING)
offsets = np.arange(n_objects + 1, dtype=np.int64) * per_object
kinds = []
for m in range(n_objects):
    kind = ("contiguous", "jumps", "gaps")[m % 3]
    kinds.append(kind)
    duration = rng.integers(240, 961, per_object)
    gap = rng.integers(1, 480, per_object) * (rng.random(per_object) < 0.5) if kind == "gaps" else np.zeros(per_object, np.int64)
    b = blocks[offsets[m]:offsets[m + 1]]
    b["duration"] = duration
    b["rtime"] = np.concatenate([[0], np.cumsum(duration + gap)[:-1]])
    b["jump_position"] = rng.random(per_object) < 0.5 if kind == "jumps" else 0
    b["interpolation_length"] = np.where(b["jump_position"] == 1, rng.integers(0, duration + 1), -1)
objects = np.arange(n_objects, dtype=np.int32)
modes = np.zeros(n_objects, np.int32)
starts = rng.integers(0, 4800, n_objects).astype(np.int64)
direct = rng.uniform(0, 1, (len(blocks), n_out)).astype(np.float32)
diffuse = rng.uniform(0, 1, (len(blocks), n_out)).astype(np.float32)

# the loop's inputs, made outside the timed region: each object's points and their rows
by_hand = []
direct_0, diffuse_0 = (np.vstack([a, np.zeros((1, n_out), np.float32)]) for a in (direct, diffuse))  # (row -1: silence)
for m in range(n_objects):
    times, source = capi.timeline_points(0, int(starts[m]), blocks[offsets[m]:offsets[m + 1]])
    rows = np.where(source >= 0, offsets[m] + source, len(blocks))
    by_hand.append((times, np.ascontiguousarray(direct_0[rows]), np.ascontiguousarray(diffuse_0[rows])))
points_total = sum(len(t) for t, _, _ in by_hand)

ctx = capi.Context(0)
r = capi.Renderer(ctx, n_objects, n_out, block_size, capi.design_decorrelators(names), 255, max_blocks=1)


def bulk():
    r.set_objects_blocks(objects, modes, starts, offsets, blocks, direct, diffuse)
    r.commit()


def loop():
    for m, (times, d, f) in enumerate(by_hand):
        r.set_object_points(m, times, d, f)
    r.commit()


def timed(step):
    ctx.synchronize()
    t0 = time.perf_counter()
    step()
    ctx.synchronize()
    return time.perf_counter() - t0


for step in (bulk, loop, bulk, loop):  # the first commit of a size allocates
    step()
seconds = {"set_objects_blocks_commit": [], "set_object_points_loop_commit": []}
for _ in range(5):
    seconds["set_objects_blocks_commit"].append(timed(bulk))
    seconds["set_object_points_loop_commit"].append(timed(loop))
# where the bulk call's time goes: the binding alone, then the commit alone
bind_only = []
for _ in range(5):
    t0 = time.perf_counter()
    r.set_objects_blocks(objects, modes, starts, offsets, blocks, direct, diffuse)
    bind_only.append(time.perf_counter() - t0)
    r.commit()
ctx.synchronize()

res = {"metric": "audioBlockFormats per second bound to the renderer's curves: earhip_render_set_objects_blocks + commit, and "
                 "the per-object earhip_render_set_object_points loop + commit over the same points",
       "unit": "Mblocks/s", "objects": n_objects, "blocks_per_object": per_object, "blocks": len(blocks), "points": points_total,
       "layout": layout, "n_out": n_out, "n_buses": 2, "rounds": 5,
       "objects_by_kind": {k: kinds.count(k) for k in ("contiguous", "jumps", "gaps")}}
for name, s in seconds.items():
    rate = [len(blocks) / v / 1e6 for v in s]
    res[name] = round(float(np.median(rate)), 3)
    res[name + "_spread"] = [round(min(rate), 3), round(max(rate), 3)]
    res[name + "_ms"] = round(float(np.median(s)) * 1e3, 2)
res["set_objects_blocks_alone_ms"] = round(float(np.median(bind_only)) * 1e3, 2)
res["bulk_vs_loop"] = round(res["set_objects_blocks_commit"] / res["set_object_points_loop_commit"], 3)
r.close()
ctx.close()
print(json.dumps(res))
