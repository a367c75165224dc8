"""What the programme loudness meter (include/earhip.h, group L) costs, on one GPU, as one JSON line:
  (a) the headline-shaped earhip_render_process_device (1024 objects -> 9+10+3, block 512, 1024 blocks per call) WITHOUT and WITH
      a meter attached: medians of alternating repetitions in one process, so that drift of the box hits both alike;
  (b) the stand-alone meter (earhip_loudness_process_device) over 24 x 524,288 device-resident samples: us per call and GB/s of
      rows read (once: the kernels read them twice);
  (c) scipy.signal.sosfilt in float64 over the same rows on one core of the same box (skipped, null, where scipy is missing).
Times are HIP events around each call on the context's stream, after 40 ms of untimed load (an idle MI355X needs 10-20 ms of
load to leave its low-power clocks, as in bench.py).

usage: python tools/loudness_rate.py [--reps 20] [--blocks 1024] [--objects 1024] [--no-cpu]"""
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

COEFFS = [[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
          [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]]


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
    torch.cuda.synchronize()
    steps_per_call = n // (48000 // 10) + 1
    meter = capi.Loudness(ctx, N, 48000, max_steps=steps_per_call)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def render(with_meter):
        r.attach_loudness(meter if with_meter else None)
        meter.reset()
        r.reset(0)
        return timed(lambda: r.process_device(T, x.data_ptr(), n, out.data_ptr(), n))

    def alone():
        meter.reset()
        return timed(lambda: meter.process_device(n, out.data_ptr(), n))

    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.precondition_ms:
        render(False)
    for _ in range(3):
        render(False), render(True), alone()
    t = {"plain": [], "metered": [], "alone": []}
    for _ in range(a.reps):
        t["plain"].append(render(False))
        t["metered"].append(render(True))
        t["alone"].append(alone())
    r.attach_loudness(None)
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"tool": "loudness_rate", "device": torch.cuda.get_device_name(0), "objects": M, "channels": N, "block": B, "blocks": T,
           "samples_per_channel": n, "reps": a.reps, "tail_blocks": r.last_tail_blocks(),
           "render_us": med["plain"], "render_with_meter_us": med["metered"],
           "render_us_min_max": [float(min(t["plain"])), float(max(t["plain"]))],
           "render_with_meter_us_min_max": [float(min(t["metered"])), float(max(t["metered"]))],
           "meter_cost_us": med["metered"] - med["plain"], "meter_cost_share": (med["metered"] - med["plain"]) / med["plain"],
           "meter_alone_us": med["alone"], "meter_alone_us_min_max": [float(min(t["alone"])), float(max(t["alone"]))],
           "meter_alone_rows_gb_s": N * n * 4 / (med["alone"] * 1e-6) / 1e9, "cpu_sosfilt_ms": None, "cpu_msamples_s": None}
    if not a.no_cpu:
        try:
            from scipy.signal import sosfilt
            rows = out.cpu().numpy().astype(np.float64)
            sos = np.array([[c[0], c[1], c[2], 1.0, c[3], c[4]] for c in COEFFS])
            try:
                os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
            except (AttributeError, OSError):
                pass
            t0 = time.perf_counter()
            y = sosfilt(sos, rows, axis=1)
            float(np.sum(y * y))
            dt = time.perf_counter() - t0
            res["cpu_sosfilt_ms"] = dt * 1e3
            res["cpu_msamples_s"] = N * n / dt / 1e6
        except ImportError:
            pass
    meter.close()
    r.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
