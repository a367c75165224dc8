"""Rate of the file-to-file call (earhip_render_process_frames_pcm: PCM frames in, PCM frames out) against the best the float
outputs allow for the same use (earhip_render_process_frames with interleaved float32 outputs), from host memory, at shapes
where the outputs are a real share of the bus traffic: the headline (1024 -> 24), the reference's matrix_benchmark shape
(32 -> 24) and an HOA-like programme (16 -> 24, more out than in); 256 blocks of 512 per call, pageable and pinned
(earhip_host_alloc) memory.  The forms — in/out: s16/float, s16/s16, s24/s24 — run in one process, alternating call by call
after a warm-up, so that drift of the box hits every form alike.  Per form: median and spread (min / max) of the calls'
Gsamples/s (input samples), the bus bytes per frame each way, and the H2D / D2H rate of a plain pinned copy measured in the same run.

usage: python tools/frames_out_rate.py [--reps 7] [--shapes 1024,32,16] [--blocks 256] [--forms s16/float,s16/s16,s24/s24]
                                       [--memory pageable,pinned] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (first: one HIP runtime per process, as bench.py)
import pcm_model  # noqa: E402
import scenes  # noqa: E402
from layouts import LAYOUTS  # noqa: E402
from libear_amd import capi  # noqa: E402

FORMS = ("s16/float", "s16/s16", "s24/s24")
BYTES = {"float": 4, "s16": 2, "s24": 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="1024,32,16")
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--memory", default="pageable,pinned")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    forms = [f for f in FORMS if f in a.forms.split(",")]
    B, T = 512, a.blocks
    names = LAYOUTS["9+10+3"]
    N = len(names)
    dec = capi.design_decorrelators(names)
    ctx = capi.Context(0)
    probe = ctx.pinned_array((64 << 20,))
    h2d_ms, d2h_ms = ctx.copy_bandwidth(probe, reps=5)
    h2d, d2h = probe.nbytes / (h2d_ms * 1e-3) / 1e9, probe.nbytes / (d2h_ms * 1e-3) / 1e9
    print(f"pinned {probe.nbytes >> 20} MB copy: H2D {h2d:.1f} GB/s, D2H {d2h:.1f} GB/s", flush=True)
    ctx.release(probe)
    results = []
    rng = np.random.default_rng(3)
    n = T * B
    for M in (int(v) for v in a.shapes.split(",")):
        curves = scenes.dense_curves(M, N, B, T, seed=7)
        r = capi.Renderer(ctx, M, N, B, dec, 255, max_blocks=T)
        for m, (t, d, f) in enumerate(curves):
            r.set_object_points(m, t, d, f)
        r.commit()
        frames = {k: pcm_model.random_frames(rng, k, n, M) for k in ("s16", "s24")}
        for memory in a.memory.split(","):
            keep = []

            def buf(shape, dtype, init=None):
                if memory == "pinned":
                    p = ctx.pinned_array(shape, dtype)
                    keep.append(p)
                else:
                    p = np.zeros(shape, dtype)
                if init is not None:
                    p[...] = init
                return p
            src = {k: buf(v.shape, v.dtype, v) for k, v in frames.items()}
            out = {"float": buf((n, N), np.float32), "s16": buf((n, N), np.int16), "s24": buf((n, 3 * N), np.uint8)}

            def call(form):
                fi, fo = form.split("/")
                r.reset(0)
                t0 = time.perf_counter()
                if fo == "float":
                    r.process_frames_into(src[fi], out[fo], fi, 0, interleaved_out=True)
                else:
                    r.process_frames_pcm_into(src[fi], out[fo], fi, 0, fo)
                return time.perf_counter() - t0

            for _ in range(2):
                for form in forms:
                    call(form)
            times = {f: [] for f in forms}
            for _ in range(a.reps):
                for form in forms:
                    times[form].append(call(form))
            chunks = r.last_host_chunks()
            base = None
            for form in forms:
                fi, fo = form.split("/")
                gs = np.array([M * n / t / 1e9 for t in times[form]])
                med = float(np.median(gs))
                base = med if base is None else base
                b_in, b_out = M * BYTES[fi], N * BYTES[fo]
                ms = float(np.median(times[form])) * 1e3
                res = {"M": M, "N": N, "T": T, "memory": memory, "form": form, "gsamples_s": med, "gsamples_s_min": float(gs.min()),
                       "gsamples_s_max": float(gs.max()), "ms_per_call": ms, "bus_bytes_in_per_frame": b_in, "bus_bytes_out_per_frame": b_out,
                       "bus_gb_s": (b_in + b_out) * n / (ms * 1e-3) / 1e9, "h2d_gb_s": h2d, "d2h_gb_s": d2h, "vs_first_form": med / base,
                       "chunks": chunks, "reps": a.reps}
                results.append(res)
                print(f"{M:5d}->{N} T={T} {memory:8s} {form:9s}: {med:7.3f} Gsamples/s (min {gs.min():.3f} max {gs.max():.3f}), {ms:7.3f} ms/call, "
                      f"bus {b_in} + {b_out} B/frame = {res['bus_gb_s']:5.1f} GB/s, {res['vs_first_form']:.2f} x {forms[0]}", flush=True)
            for p in keep:
                ctx.release(p)
        r.close()
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"h2d_gb_s": h2d, "d2h_gb_s": d2h, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
