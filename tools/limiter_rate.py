"""What the look-ahead limiter (include/earhip.h, group N) costs, on one GPU, as one JSON line:
  (a) the stand-alone device pass (earhip_limiter_process_device) over 24 x 524,288 device-resident samples at L = 64, H = 480,
      with detect = 1 (true peak) and detect = 0 (sample peak), in microseconds and as bytes per second — 2 reads and 1 write of
      the rows — against the linear read stream of earhip_debug_read_bandwidth over the same rows; next to them the true-peak
      pass of the meter (1 read), the nearest yardstick;
  (b) the headline-shaped earhip_render_process_device (1024 objects -> 9+10+3, block 512, 1024 blocks per call) with NO limiter
      and with one attached: what attaching adds;
  (c) the float64 model of the limiter (tests/limiter_model.py) over the same rows on one core of the same box.
Medians of alternating repetitions in one process, so that drift of the box hits all legs alike.  Times are HIP events around
each call on the context's stream, after 40 ms of untimed load (an idle MI355X needs 10-20 ms of load to leave its low-power
clocks, as in bench.py).

usage: python tools/limiter_rate.py [--reps 20] [--blocks 1024] [--objects 1024] [--lookahead 64] [--hold 480] [--no-cpu]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--objects", type=int, default=1024)
    ap.add_argument("--lookahead", type=int, default=64)
    ap.add_argument("--hold", type=int, default=480)
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
    limited = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    gain = torch.zeros((n,), dtype=torch.float32, device="cuda")
    r.process_device(T, x.data_ptr(), n, out.data_ptr(), n)
    torch.cuda.synchronize()
    bus_peak = float(out.abs().max())
    c = 0.25 * bus_peak  # the bus passes the ceiling by 12 dB: the limiter works
    lims = {"true": capi.Limiter(ctx, N, c, a.lookahead, a.hold, true_peak=True, max_samples=n),
            "sample": capi.Limiter(ctx, N, c, a.lookahead, a.hold, true_peak=False, max_samples=n)}
    meters = {"meter": capi.Loudness(ctx, N, 48000, max_steps=n // 4800 + 1),
              "true_peak": capi.Loudness(ctx, N, 48000, max_steps=n // 4800 + 1, true_peak=True)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def render(lim):
        if lim is None:
            r.attach_limiter(None)
        else:
            r.attach_limiter(lim, limited.data_ptr(), n, n)
            lim.reset()
        r.reset(0)
        return timed(lambda: r.process_device(T, x.data_ptr(), n, out.data_ptr(), n))

    def alone(which, with_gain):
        lims[which].reset()
        return timed(lambda: lims[which].process_device(n, out.data_ptr(), n, limited.data_ptr(), n, gain.data_ptr() if with_gain else None))

    def meter(which):
        meters[which].reset()
        return timed(lambda: meters[which].process_device(n, out.data_ptr(), n))

    legs = [("render", lambda: render(None)), ("render_limiter", lambda: render(lims["true"])),
            ("alone_true", lambda: alone("true", False)), ("alone_true_gain", lambda: alone("true", True)),
            ("alone_sample", lambda: alone("sample", False)), ("meter", lambda: meter("meter")), ("meter_true_peak", lambda: meter("true_peak"))]
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
    r.attach_limiter(None)
    med = {k: float(np.median(v)) for k, v in t.items()}
    read_ms = ctx.read_bandwidth(out.data_ptr(), N, n, n, reps=10)[0]
    rows_bytes = N * n * 4
    stats = lims["true"].stats()
    res = {"tool": "limiter_rate", "device": torch.cuda.get_device_name(0), "objects": M, "channels": N, "block": B, "blocks": T,
           "samples_per_channel": n, "lookahead": a.lookahead, "hold": a.hold, "reps": a.reps, "ceiling_over_bus_peak": c / bus_peak,
           "min_gain": float(stats[0]), "limited_fraction": stats[1] / n,
           "limiter_true_peak_us": med["alone_true"], "limiter_true_peak_with_gain_row_us": med["alone_true_gain"],
           "limiter_sample_peak_us": med["alone_sample"],
           "limiter_true_peak_gb_s": 3 * rows_bytes / (med["alone_true"] * 1e-6) / 1e9,
           "limiter_sample_peak_gb_s": 3 * rows_bytes / (med["alone_sample"] * 1e-6) / 1e9,
           "read_stream_gb_s": rows_bytes / (read_ms * 1e-3) / 1e9,
           "true_peak_pass_us": med["meter_true_peak"] - med["meter"],
           "render_us": med["render"], "render_with_limiter_us": med["render_limiter"],
           "limiter_attached_cost_us": med["render_limiter"] - med["render"],
           "us_min_max": {k: [float(min(v)), float(max(v))] for k, v in t.items()},
           "cpu_model_ms": None, "cpu_msamples_s": None}
    if not a.no_cpu:
        import limiter_model  # noqa: E402
        rows = out.cpu().numpy()
        try:
            os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
        except (AttributeError, OSError):
            pass
        t0 = time.perf_counter()
        m = limiter_model.limit(rows, c, a.lookahead, a.hold, True)
        dt = time.perf_counter() - t0
        res["cpu_model_ms"] = dt * 1e3
        res["cpu_msamples_s"] = N * n / dt / 1e6
        res["cpu_model_min_gain"] = m["min_gain"]
    for v in list(lims.values()) + list(meters.values()):
        v.close()
    r.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
