"""What the biquad filter matrix (include/earhip.h, group O) costs, on one GPU, as one JSON line:
  (a) the headline-shaped earhip_render_process_device (1024 objects -> 9+10+3, block 512, 1024 blocks per call) alone, and
      FOLLOWED on the same stream by the stage over the rows it wrote (the 9+10+3 bass-management list): medians of alternating
      repetitions in one process, so that drift of the box hits both alike;
  (b) the stage stand-alone (earhip_iir_process_device) over 24 x 524,288 device-resident samples, for 24 diagonal routes of 2
      sections, the 9+10+3 bass-management list (68 routes, 23 into each LFE) and 24 diagonal routes of 8 sections: us per call;
  (c) the stand-alone loudness meter (earhip_loudness_process_device) over the same rows in the same run: the yardstick — the
      same technique, a 2-section cascade, rows read twice, no samples written;
  (d) scipy.signal.sosfilt in float64 over the same rows on one core of the same box, 2 sections per row (skipped, null, where
      scipy is missing).
Times are HIP events around each call on the context's stream, after 40 ms of untimed load (an idle MI355X needs 10-20 ms of
load to leave its low-power clocks, as in bench.py).

usage: python tools/iir_rate.py [--reps 20] [--blocks 1024] [--objects 1024] [--no-cpu]"""
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
import scenes  # noqa: E402
from layouts import LAYOUTS  # noqa: E402
from libear_amd import capi  # noqa: E402

FS = 48000.0


def lr4(kind, f0):
    return [capi.iir_design(kind, FS, f0)] * 2


def bass_management(names, fc=80.0):
    lfe = [i for i, n in enumerate(names) if n.startswith("LFE")]
    mains = [i for i, n in enumerate(names) if not n.startswith("LFE")]
    routes = [(i, i, 1.0, lr4("highpass", fc)) for i in mains]
    for k in lfe:
        routes.append((k, k, 1.0, None))
        routes += [(i, k, 1.0 / len(lfe), lr4("lowpass", fc)) for i in mains]
    return routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--objects", type=int, default=1024)
    ap.add_argument("--precondition-ms", type=float, default=40.0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    B, T, M = 512, a.blocks, a.objects
    names = LAYOUTS["9+10+3"]
    N = len(names)
    n = T * B
    stream = torch.cuda.Stream()  # (the context enqueues on it, and the timing events are recorded on it)
    ctx = capi.Context(0, stream.cuda_stream)
    r = capi.Renderer(ctx, M, N, B, capi.design_decorrelators(names), 255, max_blocks=T)
    for m, (t, d, f) in enumerate(scenes.dense_curves(M, N, B, T, seed=7)):
        r.set_object_points(m, t, d, f)
    r.commit()
    x = torch.from_numpy(scenes.audio(M, n)).cuda()
    out = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    sink = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eight = lr4("lowpass", 80.0) + lr4("highpass", 20.0) + [capi.iir_design("peaking", FS, 200.0, 2.0, 6.0),
                                                           capi.iir_design("peaking", FS, 1000.0, 1.0, -4.0),
                                                           capi.iir_design("low_shelf", FS, 120.0, 0.7071, 3.0),
                                                           capi.iir_design("high_shelf", FS, 8000.0, 0.7071, -2.0)]
    banks = {"diagonal_2": capi.IirBank(ctx, N, N, [(i, i, 1.0, lr4("highpass", 80.0)) for i in range(N)], max_samples=n),
             "bass_management": capi.IirBank(ctx, N, N, bass_management(names), max_samples=n),
             "diagonal_8": capi.IirBank(ctx, N, N, [(i, i, 1.0, eight) for i in range(N)], max_samples=n)}
    meter = capi.Loudness(ctx, N, 48000, max_steps=n // (48000 // 10) + 1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def render(with_stage):
        bank = banks["bass_management"]
        bank.reset()
        r.reset(0)

        def call():
            r.process_device(T, x.data_ptr(), n, out.data_ptr(), n)
            if with_stage:
                bank.process_device(n, out.data_ptr(), n, sink.data_ptr(), n)
        return timed(call)

    def alone(name):
        banks[name].reset()
        return timed(lambda: banks[name].process_device(n, out.data_ptr(), n, sink.data_ptr(), n))

    def meter_alone():
        meter.reset()
        return timed(lambda: meter.process_device(n, out.data_ptr(), n))

    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.precondition_ms:
        render(False)
    keys = ["plain", "staged", "meter"] + list(banks)
    t = {k: [] for k in keys}
    for rep in range(a.reps + 3):
        row = {"plain": render(False), "staged": render(True), "meter": meter_alone()}
        for name in banks:
            row[name] = alone(name)
        if rep >= 3:  # (three untimed rounds)
            for k in keys:
                t[k].append(row[k])
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"tool": "iir_rate", "device": torch.cuda.get_device_name(0), "objects": M, "channels": N, "block": B, "blocks": T,
           "samples_per_channel": n, "reps": a.reps, "info": banks["bass_management"].info(),
           "render_us": med["plain"], "render_with_iir_us": med["staged"],
           "render_us_min_max": [float(min(t["plain"])), float(max(t["plain"]))],
           "render_with_iir_us_min_max": [float(min(t["staged"])), float(max(t["staged"]))],
           "iir_cost_us": med["staged"] - med["plain"], "iir_cost_share": (med["staged"] - med["plain"]) / med["plain"],
           "meter_alone_us": med["meter"], "meter_alone_us_min_max": [float(min(t["meter"])), float(max(t["meter"]))],
           "cpu_sosfilt_ms": None, "cpu_msamples_s": None}
    for name in banks:
        res[f"iir_alone_{name}_us"] = med[name]
        res[f"iir_alone_{name}_us_min_max"] = [float(min(t[name])), float(max(t[name]))]
        res[f"iir_alone_{name}_msamples_s"] = N * n / med[name]
    if not a.no_cpu:
        try:
            from scipy.signal import sosfilt
            rows = out.cpu().numpy().astype(np.float64)
            sos = np.array([[c[0], c[1], c[2], 1.0, c[3], c[4]] for c in lr4("highpass", 80.0)])
            try:
                os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
            except (AttributeError, OSError):
                pass
            t0 = time.perf_counter()
            y = sosfilt(sos, rows, axis=1)
            float(np.sum(y))
            dt = time.perf_counter() - t0
            res["cpu_sosfilt_ms"] = dt * 1e3
            res["cpu_msamples_s"] = N * n / dt / 1e6
        except ImportError:
            pass
    for b in banks.values():
        b.close()
    meter.close()
    r.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
