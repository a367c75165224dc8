"""Long calls from host memory, timed: 1024 objects x 64 blocks of 512 samples on 9+10+3, two buses (128 MB of input rows: the
pipeline of time chunks of host_pipeline.h), from three sources — pageable rows (earhip_render_process: staging threads, 16 MB
chunks), earhip_host_alloc rows both ways (the same entry, 32 MB chunks by strided DMA, no staging) and pageable s24 frames to s16
frames (earhip_render_process_frames_pcm: the contiguous-range job of the staging threads).
    python tools/host_call_ab.py run LABEL OUT.json        (EARHIP_LIB=<another build of libearhip.so>: that build)
    python tools/host_call_ab.py compare PARENT.json PARENT_AGAIN.json NEW.json OUT.json
    python tools/host_call_ab.py alternate PARENT_LIB OUTDIR   (parent, new and parent again in turn, ROUNDS times, then compare)
run: 3 warm-up calls, then the median of CALLS calls on a host clock (ms; a call ends drained).  compare: the margin is the
largest relative difference of the two parent runs' medians over the three sources; a source passes when its new median is not
above its parent median (the first run's) by more than that margin.  Exit status 1 when a source fails.  alternate: the three runs
as ROUNDS short ones each (CALLS / ROUNDS timed calls a source), one fresh process per run, taken in turn with the order rotated
from round to round, the calls of a label pooled: a machine that others use drifts by more in the minute between three long runs
than the builds differ, and in turn each label sees the same of it.  The result: OUTDIR/host_lanes_ab.json."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

M, B, T, LAYOUT, WARM, CALLS, ROUNDS = 1024, 512, 64, "9+10+3", 3, 72, 9


def run(label, out_path, calls=CALLS):
    import scenes
    from layouts import LAYOUTS
    from libear_amd import capi
    from libear_amd.build import lib_path
    names = LAYOUTS[LAYOUT]
    N = len(names)
    ctx = capi.Context(0)  # raises without a GPU: nothing is timed on a CPU
    r = capi.Renderer(ctx, M, N, B, capi.design_decorrelators(names), 255, max_blocks=T)
    for m, (t, d, f) in enumerate(scenes.dense_curves(M, N, B, T, seed=7)):
        r.set_object_points(m, t, d, f)
    r.commit()
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (M, B * T)).astype(np.float32)
    out = np.empty((N, B * T), np.float32)
    px, pout = ctx.pinned_array((M, B * T)), ctx.pinned_array((N, B * T))
    px[...] = x
    frames = rng.integers(0, 256, (B * T, 3 * M), dtype=np.uint8)
    pcm = np.empty((B * T, N), np.int16)
    sources = {
        "pageable_rows": lambda: r.process_into(x, out),
        "host_alloc_rows": lambda: r.process_into(px, pout),
        "pageable_s24_to_s16": lambda: r.process_frames_pcm_into(frames, pcm, "s24", 0, "s16"),
    }
    result = {"label": label, "lib": os.path.relpath(lib_path(), ROOT), "objects": M, "blocks": T, "block": B, "layout": LAYOUT,
              "calls": calls, "sources": {}}
    for name, call in sources.items():
        times = []
        for i in range(WARM + calls):
            r.reset(0)
            t0 = time.perf_counter()
            call()
            times.append(1e3 * (time.perf_counter() - t0))
        t = np.array(times[WARM:])
        result["sources"][name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                                   "chunks": r.last_host_chunks(), "times_ms": [round(float(v), 4) for v in t]}
    r.close()
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


def compare(parent, again, new, out_path):
    a, b, c = (json.load(open(p)) for p in (parent, again, new))
    med = lambda r, s: r["sources"][s]["median_ms"]
    names = list(a["sources"])
    margin = max(abs(med(a, s) - med(b, s)) / min(med(a, s), med(b, s)) for s in names)
    verdict = {s: {"parent_ms": med(a, s), "parent_again_ms": med(b, s), "new_ms": med(c, s), "new_over_parent": med(c, s) / med(a, s) - 1.0,
                   "within_margin": med(c, s) <= med(a, s) * (1.0 + margin)} for s in names}
    for r in (a, b, c):  # (the pooled medians and the rounds' stay; the single calls do not)
        for s in r["sources"].values():
            s.pop("times_ms", None)
    out = {"margin": margin, "verdict": verdict, "runs": [a, b, c]}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"margin": margin, "verdict": verdict}))
    return all(v["within_margin"] for v in verdict.values())


def alternate(parent_lib, outdir):
    os.makedirs(outdir, exist_ok=True)
    labels = [("parent", parent_lib), ("new", None), ("parent_again", parent_lib)]
    parts = {label: [] for label, _ in labels}
    for r in range(ROUNDS):
        for label, lib in labels[r % 3:] + labels[:r % 3]:
            env = dict(os.environ)
            env.pop("EARHIP_LIB", None)
            if lib:
                env["EARHIP_LIB"] = os.path.abspath(lib)
            part = os.path.join(outdir, f"{label}_round{r}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "run", label, part, str(CALLS // ROUNDS)], env=env, check=True,
                           stdout=subprocess.DEVNULL, timeout=300)
            parts[label].append(json.load(open(part)))
            os.remove(part)
            print(f"round {r} {label}: " + ", ".join(f"{s} {v['median_ms']:.3f} ms" for s, v in parts[label][-1]["sources"].items()), flush=True)
    pooled = {}
    for label, rs in parts.items():
        m = dict(rs[0], calls=sum(q["calls"] for q in rs), rounds=ROUNDS, sources={})
        for name in rs[0]["sources"]:
            t = np.concatenate([q["sources"][name]["times_ms"] for q in rs])
            m["sources"][name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                                  "chunks": rs[0]["sources"][name]["chunks"],
                                  "round_medians_ms": [q["sources"][name]["median_ms"] for q in rs]}
        pooled[label] = os.path.join(outdir, f"{label}.json")
        with open(pooled[label], "w") as f:
            json.dump(m, f, indent=1)
    ok = compare(pooled["parent"], pooled["parent_again"], pooled["new"], os.path.join(outdir, "host_lanes_ab.json"))
    for p in pooled.values():
        os.remove(p)
    return ok


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"] and len(sys.argv) in (4, 5):
        run(sys.argv[2], sys.argv[3], *[int(v) for v in sys.argv[4:]])
    elif sys.argv[1:2] == ["alternate"] and len(sys.argv) == 4:
        sys.exit(0 if alternate(sys.argv[2], sys.argv[3]) else 1)
    elif sys.argv[1:2] == ["compare"] and len(sys.argv) == 6:
        sys.exit(0 if compare(*sys.argv[2:6]) else 1)
    else:
        sys.exit(__doc__)
