"""What switching and crossfading filter sets of the FIR filter matrix costs (include/earhip.h, group M, FILTER SETS), on one GPU,
as one JSON line.  The monitoring case, 24 -> 2 x 2048 taps at B = 512, a matrix with two sets over device-resident rows:
  (a) one block per call (the head-tracking pattern): steady, against a select(other, 1) before every call — every block a fade
      block, the fade kernel instead of the steady kernel;
  (b) 1024 blocks per call: without and with one select(other, 1) before the call — one fade launch of one block beside the
      steady launch of 1023;
  (c) one load_set (host taps: the check, the pair lists, the staging copy and the transforms) and one load_set_device (device
      taps: a strided copy and the transforms) of the idle set.
Medians of alternating repetitions in one process, so that drift of the box hits all alike.  Times are HIP events around each
call on the context's stream, after 40 ms of untimed load (an idle MI355X needs 10-20 ms of load to leave its low-power clocks,
as in bench.py); load_set's host work is inside its figure as wall time too (`load_set_wall_us`: call to synchronised).

usage: python tools/firmix_switch_rate.py [--reps 20] [--blocks 1024] [--calls 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: one HIP runtime per process, as bench.py)
from libear_amd import capi  # noqa: E402


def taps(K, C, J, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, (K, C, J)) * np.exp(-4.0 * np.arange(J) / J)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=64, help="one-block calls per timed repetition of (a)")
    ap.add_argument("--precondition-ms", type=float, default=40.0)
    a = ap.parse_args()
    C, K, J, B, T = 24, 2, 2048, 512, a.blocks
    n = T * B
    stream = torch.cuda.Stream()  # (the context enqueues on it, and the timing events are recorded on it)
    ctx = capi.Context(0, stream.cuda_stream)
    h = [taps(K, C, J, 1), taps(K, C, J, 2)]
    h_dev = torch.from_numpy(h[1]).cuda()
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1.0, 1.0, (C, n)).astype(np.float32)).cuda()
    out = torch.zeros((K, n), dtype=torch.float32, device="cuda")
    m = capi.FirMatrix(ctx, h[0], B, max_blocks=T, n_sets=3)
    m.load_set(1, h[1])
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def other():
        return 1 - m.state()["current"]

    def one_block_calls(fade):
        def go():
            for i in range(a.calls):
                if fade:
                    m.select(other(), 1)
                m.process_device(1, x[:, i * B:].data_ptr(), n, out[:, i * B:].data_ptr(), n)
        return timed(go) / a.calls

    def long_call(fade):
        if fade:
            m.select(other(), 1)
        return timed(lambda: m.process_device(T, x.data_ptr(), n, out.data_ptr(), n))

    def load_host():
        t0 = time.perf_counter()
        us = timed(lambda: m.load_set(2, h[1]))
        return us, (time.perf_counter() - t0) * 1e6

    def load_device():
        return timed(lambda: m.load_set_device(2, h_dev.data_ptr()))

    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.precondition_ms:
        long_call(False)
    for _ in range(3):
        one_block_calls(False), one_block_calls(True), long_call(False), long_call(True), load_host(), load_device()
    t = {k: [] for k in ("steady_1", "fade_1", "steady_T", "fade_T", "load", "load_wall", "load_dev")}
    for _ in range(a.reps):
        t["steady_1"].append(one_block_calls(False))
        t["fade_1"].append(one_block_calls(True))
        t["steady_T"].append(long_call(False))
        t["fade_T"].append(long_call(True))
        us, wall = load_host()
        t["load"].append(us)
        t["load_wall"].append(wall)
        t["load_dev"].append(load_device())
    med = {k: float(np.median(v)) for k, v in t.items()}
    span = {k: [float(min(v)), float(max(v))] for k, v in t.items()}
    res = {"tool": "firmix_switch_rate", "device": torch.cuda.get_device_name(0), "n_in": C, "n_out": K, "taps": J, "block": B,
           "reps": a.reps, "one_block_calls_per_rep": a.calls, "blocks_per_long_call": T,
           "one_block_call_steady_us": med["steady_1"], "one_block_call_steady_us_min_max": span["steady_1"],
           "one_block_call_fade_us": med["fade_1"], "one_block_call_fade_us_min_max": span["fade_1"],
           "one_block_fade_over_steady": med["fade_1"] / med["steady_1"],
           "long_call_us": med["steady_T"], "long_call_us_min_max": span["steady_T"],
           "long_call_with_select_us": med["fade_T"], "long_call_with_select_us_min_max": span["fade_T"],
           "long_call_select_cost_us": med["fade_T"] - med["steady_T"],
           "load_set_us": med["load"], "load_set_us_min_max": span["load"], "load_set_wall_us": med["load_wall"],
           "load_set_device_us": med["load_dev"], "load_set_device_us_min_max": span["load_dev"]}
    m.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
