"""What true-peak metering (include/earhip.h, group L: BS.1770-4 annex 2) costs, on one GPU, as one JSON line:
  (a) the stand-alone meter (earhip_loudness_process_device) over 24 x 524,288 device-resident samples with true peak OFF and ON;
  (b) the headline-shaped earhip_render_process_device (1024 objects -> 9+10+3, block 512, 1024 blocks per call) with NO meter,
      with a meter, and with a meter that measures true peak;
  (c) the float64 model of the interpolator (numpy, the 4 x 12 table) over the same rows on one core of the same box.
Medians of alternating repetitions in one process, so that drift of the box hits all legs alike.  Times are HIP events around
each call on the context's stream, after 40 ms of untimed load (an idle MI355X needs 10-20 ms of load to leave its low-power
clocks, as in bench.py).

usage: python tools/true_peak_rate.py [--reps 20] [--blocks 1024] [--objects 1024] [--no-cpu]"""
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

H0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
H1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]


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
    meters = {"meter": capi.Loudness(ctx, N, 48000, max_steps=steps_per_call),
              "true_peak": capi.Loudness(ctx, N, 48000, max_steps=steps_per_call, true_peak=True)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def render(which):
        meter = meters.get(which)
        r.attach_loudness(meter)
        if meter is not None:
            meter.reset()
        r.reset(0)
        return timed(lambda: r.process_device(T, x.data_ptr(), n, out.data_ptr(), n))

    def alone(which):
        meters[which].reset()
        return timed(lambda: meters[which].process_device(n, out.data_ptr(), n))

    legs = [("render", lambda: render(None)), ("render_meter", lambda: render("meter")), ("render_true_peak", lambda: render("true_peak")),
            ("alone_meter", lambda: alone("meter")), ("alone_true_peak", lambda: alone("true_peak"))]
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.precondition_ms:
        render(None)
    for _ in range(3):
        for _, fn in legs:
            fn()
    t = {k: [] for k, _ in legs}
    for _ in range(a.reps):
        for k, fn in legs:
            t[k].append(fn())
    r.attach_loudness(None)
    med = {k: float(np.median(v)) for k, v in t.items()}
    tp, sp = meters["true_peak"].peaks()
    res = {"tool": "true_peak_rate", "device": torch.cuda.get_device_name(0), "objects": M, "channels": N, "block": B, "blocks": T,
           "samples_per_channel": n, "reps": a.reps, "tail_blocks": r.last_tail_blocks(),
           "render_us": med["render"], "render_with_meter_us": med["render_meter"], "render_with_true_peak_us": med["render_true_peak"],
           "meter_cost_us": med["render_meter"] - med["render"], "true_peak_cost_us": med["render_true_peak"] - med["render_meter"],
           "meter_alone_us": med["alone_meter"], "meter_alone_true_peak_us": med["alone_true_peak"],
           "true_peak_alone_cost_us": med["alone_true_peak"] - med["alone_meter"],
           "us_min_max": {k: [float(min(v)), float(max(v))] for k, v in t.items()},
           "true_peak_pass_rows_gb_s": N * n * 4 / (max(med["alone_true_peak"] - med["alone_meter"], 1e-3) * 1e-6) / 1e9,
           "max_true_peak_dbtp": float(20 * np.log10(max(float(tp.max()), 1e-30))),
           "max_sample_peak_dbfs": float(20 * np.log10(max(float(sp.max()), 1e-30))),
           "cpu_model_ms": None, "cpu_msamples_s": None}
    if not a.no_cpu:
        rows = out.cpu().numpy()
        try:
            os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
        except (AttributeError, OSError):
            pass
        h = np.array([H0, H1, H1[::-1], H0[::-1]], np.float64) / 8192.0
        t0 = time.perf_counter()
        worst = 0.0
        for c in range(N):
            xr = np.concatenate([np.zeros(11), rows[c].astype(np.float64)])
            for p in range(4):
                worst = max(worst, float(np.abs(np.convolve(xr, h[p], mode="valid")).max()))
        dt = time.perf_counter() - t0
        res["cpu_model_ms"] = dt * 1e3
        res["cpu_msamples_s"] = N * n / dt / 1e6
        res["cpu_model_max_true_peak_dbtp"] = float(20 * np.log10(max(worst, 1e-30)))
    for v in meters.values():
        v.close()
    r.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
