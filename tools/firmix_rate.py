"""What the FIR filter matrix (include/earhip.h, group M) costs, on one GPU, as one JSON line:
  (a) the stand-alone matrix (earhip_firmix_process_device) over device-resident rows, 1024 blocks of 512 per call: the monitoring
      case, 24 -> 2 x 2048 taps, and a diagonal 24 x 24 x 512 taps (24 pairs): us per call, and bytes per second by two
      accountings — `once`: every datum once (rows in, spectra written and read once, filters once, rows out), `requested`: what
      the workgroups ask the caches for (each block re-reads P windows per input channel and the filters of its group);
  (b) the headline-shaped earhip_render_process_device (1024 objects -> 9+10+3, block 512, 1024 blocks per call) WITHOUT and WITH
      a 24 -> 2 x 2048 matrix attached: medians of alternating repetitions in one process, so that drift of the box hits both
      alike; and the decorrelator kernel's (K2) time for the same call, from the renderer's own event timing in a pass of its own;
  (c) scipy.signal.oaconvolve in float64 over the monitoring case on one core of the same box (skipped, null, without scipy).
Times are HIP events around each call on the context's stream, after 40 ms of untimed load (an idle MI355X needs 10-20 ms of
load to leave its low-power clocks, as in bench.py).

usage: python tools/firmix_rate.py [--reps 20] [--blocks 1024] [--objects 1024] [--no-cpu]"""
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


def taps(K, C, J, seed, diagonal=False):
    rng = np.random.default_rng(seed)
    h = (rng.uniform(-1.0, 1.0, (K, C, J)) * np.exp(-4.0 * np.arange(J) / J)).astype(np.float32)
    if diagonal:
        h *= np.eye(K, C, dtype=np.float32)[:, :, None]
    return h


def accounting(h, B, T):
    """(bytes once, bytes requested, complex multiply-adds) of a call of T blocks"""
    K, C, J = h.shape
    P = -(-J // B)
    nz = np.any(h != 0, axis=2)  # [K][C]
    used = int(nz.any(axis=0).sum())
    pairs = int(nz.sum())
    entries = sum(int((nz[g] | (nz[g + 1] if g + 1 < K else False)).sum()) for g in range(0, K, 2))
    rows_in, rows_out = used * T * B * 4, K * T * B * 4
    spectra = used * T * B * 8
    filters = pairs * P * B * 8
    once = rows_in + 2 * spectra + filters + rows_out
    requested = rows_in + spectra + T * (entries * P * B * 8 + filters) + rows_out
    return once, requested, T * pairs * P * B


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
    h_mon, h_diag = taps(2, N, 2048, 1), taps(N, N, 512, 2, diagonal=True)
    mon = capi.FirMatrix(ctx, h_mon, B, max_blocks=T)
    diag = capi.FirMatrix(ctx, h_diag, B, max_blocks=T)
    assert mon.info()["pairs"] == 2 * N and diag.info()["pairs"] == N
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def render(attached):
        r.attach_fir_matrix(mon if attached else None, sink.data_ptr(), n, n)
        r.reset(0)
        return timed(lambda: r.process_device(T, x.data_ptr(), n, out.data_ptr(), n))

    def alone(m):
        return timed(lambda: m.process_device(T, out.data_ptr(), n, sink.data_ptr(), n))

    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.precondition_ms:
        render(False)
    for _ in range(3):
        render(False), render(True), alone(mon), alone(diag)
    t = {"plain": [], "attached": [], "mon": [], "diag": []}
    for _ in range(a.reps):
        t["plain"].append(render(False))
        t["attached"].append(render(True))
        t["mon"].append(alone(mon))
        t["diag"].append(alone(diag))
    r.attach_fir_matrix(None)
    # K2's time for the same call, from the renderer's own events (a pass of its own: timing serialises the kernels)
    r.enable_timing(True)
    k2 = []
    for _ in range(5):
        r.reset(0)
        r.process_device(T, x.data_ptr(), n, out.data_ptr(), n)
        ctx.synchronize()
        k2.append(r.get_timing()["decor_ms"] * 1e3)
    r.enable_timing(False)
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"tool": "firmix_rate", "device": torch.cuda.get_device_name(0), "objects": M, "channels": N, "block": B, "blocks": T,
           "samples_per_channel": n, "reps": a.reps,
           "render_us": med["plain"], "render_with_matrix_us": med["attached"],
           "render_us_min_max": [float(min(t["plain"])), float(max(t["plain"]))],
           "render_with_matrix_us_min_max": [float(min(t["attached"])), float(max(t["attached"]))],
           "matrix_cost_us": med["attached"] - med["plain"], "matrix_cost_share": (med["attached"] - med["plain"]) / med["plain"],
           "k2_us": float(np.median(k2)), "cpu_oaconvolve_ms": None}
    for key, hh in (("mon", h_mon), ("diag", h_diag)):
        once, requested, macs = accounting(hh, B, T)
        name = {"mon": "monitoring_24x2x2048", "diag": "diagonal_24x24x512"}[key]
        res[name] = {"us": med[key], "us_min_max": [float(min(t[key])), float(max(t[key]))], "bytes_once": once,
                     "bytes_requested": requested, "once_gb_s": once / (med[key] * 1e-6) / 1e9,
                     "requested_gb_s": requested / (med[key] * 1e-6) / 1e9, "share_of_8_tb_s_once": once / (med[key] * 1e-6) / 8e12,
                     "complex_mac_gflop_s": 8 * macs / (med[key] * 1e-6) / 1e9}
    if not a.no_cpu:
        try:
            from scipy.signal import oaconvolve
            rows = out.cpu().numpy().astype(np.float64)
            try:
                os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
            except (AttributeError, OSError):
                pass
            hd = h_mon.astype(np.float64)
            t0 = time.perf_counter()
            y = np.zeros((2, n))
            for k in range(2):
                for c in range(N):
                    y[k] += oaconvolve(rows[c], hd[k, c])[:n]
            res["cpu_oaconvolve_ms"] = (time.perf_counter() - t0) * 1e3
        except ImportError:
            pass
    mon.close()
    diag.close()
    r.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
