"""What the polyphase sample-rate converter (include/earhip.h, group P) costs, on one GPU, as one JSON line:
  (a) the stage stand-alone (earhip_src_process_device) over 24 x 524,288 device-resident input samples: 160/147 (44.1 -> 48 kHz)
      and 147/160 (48 -> 44.1 kHz) with 48 taps per phase, 2/1 and 1/2 with 96: us per call;
  (b) beside each, in the same run, a plain device copy that moves the same bytes (rows of (n_in + n_out) / 2 floats read and
      written: the stage reads n_in and writes n_out per row): the yardstick for a stage that should be bound by its LDS reads,
      not by memory;
  (c) scipy.signal.upfirdn in float64 over the same rows on one core of the same box (skipped, null, where scipy is missing).
Times are HIP events around each call on the context's stream, after 40 ms of untimed load (an idle MI355X needs 10-20 ms of
load to leave its low-power clocks, as in bench.py); medians of alternating repetitions in one process.

usage: python tools/src_rate.py [--reps 20] [--samples 524288] [--channels 24] [--no-cpu]"""
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

CASES = [("160_147", 160, 147, 48), ("147_160", 147, 160, 48), ("2_1", 2, 1, 96), ("1_2", 1, 2, 96)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--channels", type=int, default=24)
    ap.add_argument("--precondition-ms", type=float, default=40.0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    C, n = a.channels, a.samples
    stream = torch.cuda.Stream()  # (the context enqueues on it, and the timing events are recorded on it)
    ctx = capi.Context(0, stream.cuda_stream)
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 1.0, (C, n)).astype(np.float32)).cuda()
    stages, outs, copies, taps = {}, {}, {}, {}
    for name, L, M, T in CASES:
        taps[name] = capi.src_design(L, M, T)
        stages[name] = capi.SampleRateConverter(ctx, C, L, M, T, taps[name], max_samples=n)
        outs[name] = torch.zeros((C, stages[name].max_out), dtype=torch.float32, device="cuda")
        half = (n + stages[name].max_out) // 2
        copies[name] = (torch.zeros((C, half), dtype=torch.float32, device="cuda"), torch.zeros((C, half), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def stage(name):
        s, o = stages[name], outs[name]
        s.reset()
        return timed(lambda: s.process_device(n, x.data_ptr(), n, o.data_ptr(), o.shape[1], o.shape[1]))

    def copy(name):
        src, dst = copies[name]
        with torch.cuda.stream(stream):
            return timed(lambda: dst.copy_(src))

    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.precondition_ms:
        stage("160_147")
    keys = [k for name, _, _, _ in CASES for k in (name, "copy_" + name)]
    t = {k: [] for k in keys}
    for rep in range(a.reps + 3):
        row = {}
        for name, _, _, _ in CASES:
            row[name] = stage(name)
            row["copy_" + name] = copy(name)
        if rep >= 3:  # (three untimed rounds)
            for k in keys:
                t[k].append(row[k])
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"tool": "src_rate", "device": torch.cuda.get_device_name(0), "channels": C, "samples_per_channel": n, "reps": a.reps}
    for name, L, M, T in CASES:
        info = stages[name].info()
        n_out = info["max_out"]
        res[f"src_{name}_taps_per_phase"] = T
        res[f"src_{name}_us"] = med[name]
        res[f"src_{name}_us_min_max"] = [float(min(t[name])), float(max(t[name]))]
        res[f"src_{name}_moutputs_s"] = C * n_out / med[name]
        res[f"src_{name}_gfma_s"] = C * n_out * T / med[name] / 1e3
        res[f"copy_{name}_us"] = med["copy_" + name]
        res[f"copy_{name}_us_min_max"] = [float(min(t["copy_" + name])), float(max(t["copy_" + name]))]
        res[f"src_{name}_over_copy"] = med[name] / med["copy_" + name]
        res[f"src_{name}_lds"] = [info["table_in_lds"], info["window_in_lds"]]
        res[f"cpu_upfirdn_{name}_ms"] = None
    if not a.no_cpu:
        try:
            from scipy.signal import upfirdn
            rows = x.cpu().numpy().astype(np.float64)
            try:
                os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
            except (AttributeError, OSError):
                pass
            for name, L, M, T in CASES:
                t0 = time.perf_counter()
                y = upfirdn(taps[name], rows, L, M, axis=1)
                float(np.sum(y))
                res[f"cpu_upfirdn_{name}_ms"] = (time.perf_counter() - t0) * 1e3
        except ImportError:
            pass
    for s in stages.values():
        s.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
