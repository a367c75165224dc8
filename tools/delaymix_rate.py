"""What the delay matrix (include/earhip.h, group S) costs, on one GPU, as one JSON line: earhip_delaymix_process_device over
24 x 524,288 device-resident samples, us per call, for
  (a) "align_t1": a diagonal alignment with one tap per channel (a gain) and whole delays spread over 0 .. 300 samples;
  (b) "align_t16": the same delays as 16-tap fractional delays (earhip_delaymix_fractional);
  (c) "bass_9_10_3": the 9+10+3 list — the diagonal of all 24 channels and the 22 mains into each of the 2 LFEs (68 routes,
      23 into each LFE) — every route behind a 4800-sample (100 ms) delay;
  (d) "copy": beside them, in the same run, a plain device copy of the same bytes (24 rows read and 24 written).  A diagonal
      one-tap matrix moves exactly these bytes, so the copy is the stage's yardstick: `vs_copy` is stage time over copy time.
Times are HIP events around each call on the context's stream, after 40 ms of untimed load (an idle MI355X needs 10-20 ms of
load to leave its low-power clocks, as in bench.py); medians of alternating repetitions in one process.

usage: python tools/delaymix_rate.py [--reps 20] [--samples 524288] [--channels 24]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: one HIP runtime per process, as bench.py)
from layouts import LAYOUTS  # noqa: E402
from libear_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--channels", type=int, default=24)
    ap.add_argument("--precondition-ms", type=float, default=40.0)
    a = ap.parse_args()
    C, n = a.channels, a.samples
    stream = torch.cuda.Stream()  # (the context enqueues on it, and the timing events are recorded on it)
    ctx = capi.Context(0, stream.cuda_stream)
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 1.0, (C, n)).astype(np.float32)).cuda()
    delays = [300.0 * c / max(C - 1, 1) for c in range(C)]
    lists = {"align_t1": [(c, c, capi.delaymix_fractional(d, 1)[0], [1.0 - 0.01 * c]) for c, d in enumerate(delays)],
             "align_t16": [(c, c) + capi.delaymix_fractional(d + 7.0, 16, 8.0) for c, d in enumerate(delays)]}
    names = LAYOUTS["9+10+3"]
    if C == len(names):
        lfe = [i for i, nm in enumerate(names) if nm.startswith("LFE")]
        mains = [i for i, nm in enumerate(names) if not nm.startswith("LFE")]
        lists["bass_9_10_3"] = [(c, c, 4800, [1.0]) for c in range(C)] + [(i, k, 4800, [1.0 / len(lfe)]) for k in lfe for i in mains]
    stages = {name: capi.DelayMatrix(ctx, C, C, routes, max_samples=n) for name, routes in lists.items()}
    out = torch.zeros((C, n), dtype=torch.float32, device="cuda")
    src, dst = torch.zeros((C, n), dtype=torch.float32, device="cuda"), torch.zeros((C, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def stage(name):
        s = stages[name]
        return timed(lambda: s.process_device(n, x.data_ptr(), n, out.data_ptr(), n))

    def copy():
        with torch.cuda.stream(stream):
            return timed(lambda: dst.copy_(src))

    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.precondition_ms:
        stage("align_t1")
    keys = list(stages) + ["copy"]
    t = {k: [] for k in keys}
    for rep in range(a.reps + 3):
        row = {name: stage(name) for name in stages}
        row["copy"] = copy()
        if rep >= 3:  # (three untimed rounds)
            for k in keys:
                t[k].append(row[k])
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"tool": "delaymix_rate", "device": torch.cuda.get_device_name(0), "channels": C, "samples_per_channel": n, "reps": a.reps,
           "bytes_moved": 8 * C * n, "copy_us": med["copy"], "copy_us_min_max": [float(min(t["copy"])), float(max(t["copy"]))],
           "copy_gb_s": 8 * C * n / med["copy"] / 1e3}
    for name, s in stages.items():
        info = s.info()
        res[f"{name}_routes"] = info["routes"]
        res[f"{name}_total_taps"] = info["total_taps"]
        res[f"{name}_max_fan_in"] = info["max_fan_in"]
        res[f"{name}_history"] = info["history"]
        res[f"{name}_us"] = med[name]
        res[f"{name}_us_min_max"] = [float(min(t[name])), float(max(t[name]))]
        res[f"{name}_msamples_s"] = C * n / med[name]
        res[f"{name}_vs_copy"] = med[name] / med["copy"]
        s.close()
    res["tile_out"] = info["tile_out"]
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
