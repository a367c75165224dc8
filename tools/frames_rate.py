"""Rate of the interleaved-frames input (earhip_render_process_frames) against the float path (earhip_render_process) from host
memory, on the headline scene (C4: 1024 objects -> 9+10+3 (24 ch), block 512, dense ramps), 64 and 256 blocks per call, from
pageable and from pinned (earhip_host_alloc) memory.  Float rows, s16, s24 and s32 frames run in the same process, alternating
call by call after a warm-up, so that drift of the box hits every form alike.  Per form: median and spread (min / max) of the
calls' Gsamples/s, the bus bytes per second that rate means (4 / 2 / 3 / 4 bytes a sample), and its share of the H2D rate of a
plain pinned copy measured in the same run.

usage: python tools/frames_rate.py [--reps 7] [--blocks 64,256] [--forms float,s16,s24,s32] [--memory pageable,pinned] [--json out.json]
(a subset of forms / memories: e.g. the calls of one form under a kernel trace)"""
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

FORMS = ("float", "s16", "s24", "s32")
BYTES = {"float": 4, "s16": 2, "s24": 3, "s32": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blocks", default="64,256")
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--memory", default="pageable,pinned")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    forms = [f for f in FORMS if f in a.forms.split(",")]
    assert forms and forms[0] == "float", "the float path is the yardstick: --forms starts with float"
    M, B = 1024, 512
    names = LAYOUTS["9+10+3"]
    N = len(names)
    dec = capi.design_decorrelators(names)
    ctx = capi.Context(0)
    # the bus: a plain copy of a pinned 256 MB buffer, each direction
    probe = ctx.pinned_array((64 << 20,))
    h2d_ms, _ = ctx.copy_bandwidth(probe, reps=5)
    h2d = probe.nbytes / (h2d_ms * 1e-3) / 1e9
    print(f"H2D of a pinned {probe.nbytes >> 20} MB copy: {h2d:.1f} GB/s", flush=True)
    ctx.release(probe)
    results = []
    rng = np.random.default_rng(3)
    for T in (int(v) for v in a.blocks.split(",")):
        n = T * B
        curves = scenes.dense_curves(M, N, B, T, seed=7)
        r = capi.Renderer(ctx, M, N, B, dec, 255, max_blocks=T)
        for m, (t, d, f) in enumerate(curves):
            r.set_object_points(m, t, d, f)
        r.commit()
        frames = {"s16": pcm_model.random_frames(rng, "s16", n, M), "s24": pcm_model.random_frames(rng, "s24", n, M),
                  "s32": pcm_model.random_frames(rng, "s32", n, M)}
        rows = pcm_model.rows(frames["s16"], "s16", 0, M)
        for memory in a.memory.split(","):
            keep = []
            if memory == "pinned":
                src = {}
                for k, v in list(frames.items()) + [("float", rows)]:
                    p = ctx.pinned_array(v.shape, v.dtype)
                    p[...] = v
                    src[k] = p
                    keep.append(p)
                out = ctx.pinned_array((N, n))
                keep.append(out)
            else:
                src = dict(frames, float=rows)
                out = np.empty((N, n), np.float32)

            def call(form):
                r.reset(0)
                t0 = time.perf_counter()
                if form == "float":
                    r.process_into(src["float"], out)
                else:
                    r.process_frames_into(src[form], out, form, 0)
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
                gs = np.array([M * n / t / 1e9 for t in times[form]])
                med = float(np.median(gs))
                base = med if form == "float" else base
                res = {"T": T, "memory": memory, "form": form, "gsamples_s": med, "gsamples_s_min": float(gs.min()),
                       "gsamples_s_max": float(gs.max()), "bus_gb_s": med * BYTES[form], "h2d_gb_s": h2d,
                       "share_of_h2d": med * BYTES[form] / h2d, "vs_float": med / base, "chunks": chunks, "reps": a.reps}
                results.append(res)
                print(f"T={T:4d} {memory:8s} {form:5s}: {med:6.2f} Gsamples/s (min {gs.min():.2f} max {gs.max():.2f}), "
                      f"{res['bus_gb_s']:5.1f} GB/s on the bus = {res['share_of_h2d']:.2f} of H2D, {res['vs_float']:.2f} x float",
                      flush=True)
            for p in keep:
                ctx.release(p)
        r.close()
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"h2d_gb_s": h2d, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
