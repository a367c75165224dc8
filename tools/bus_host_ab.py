"""The host forms of the output-bus stages, timed: FIR matrix, limiter, biquad matrix, sample-rate converter and delay matrix, each
at 24 rows x 48000 samples per call (host rows in, host rows out, the call ends in a synchronise), and one create of each.
    python tools/bus_host_ab.py run LABEL OUT.json        (EARHIP_LIB=<another build of libearhip.so>: that build)
    python tools/bus_host_ab.py compare PARENT.json PARENT_AGAIN.json NEW.json OUT.json
    python tools/bus_host_ab.py alternate PARENT_LIB OUTDIR   (parent, new and parent again in turn, ROUNDS times, then compare)
run: 20 warm-up calls, then the median of 400 calls on a host clock (ms; a call is under a millisecond: fewer calls time the
scheduler as much as the stage), and the time of the second create of the stage (the first loads the code objects).
compare: the margin is the largest relative difference of the two parent runs' medians over the five stages; a stage passes
when its new median is not above its parent median (the first run's) by more than that margin.  Exit status 1 when a stage
fails.  alternate: the three runs as ROUNDS short ones each (CALLS / ROUNDS timed calls a stage), one fresh process per run, taken
in turn with the order rotated from round to round, the calls of a label pooled: a machine that others use drifts by more in the
minute between three long runs than the builds differ, and in turn each label sees the same of it."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, N, WARM, CALLS, ROUNDS = 24, 48000, 20, 400, 5


def stages(capi, ctx):
    rng = np.random.default_rng(3)
    fir = np.zeros((ROWS, ROWS, 64), np.float32)
    for k in range(ROWS):
        fir[k, k] = rng.uniform(-0.1, 0.1, 64)
    lp = capi.iir_design("lowpass", 48000, 1000.0)
    src_taps = capi.src_design(3, 2, 8)
    return {
        "firmix": lambda: capi.FirMatrix(ctx, fir, 64, max_blocks=N // 64),
        "limiter": lambda: capi.Limiter(ctx, ROWS, 0.5, max_samples=N),
        "iir": lambda: capi.IirBank(ctx, ROWS, ROWS, [(c, c, 1.0, [lp]) for c in range(ROWS)], max_samples=N),
        "src": lambda: capi.SampleRateConverter(ctx, ROWS, 3, 2, 8, src_taps, max_samples=N),
        "delaymix": lambda: capi.DelayMatrix(ctx, ROWS, ROWS, [(c, c, 7 * c, [0.5, 0.25]) for c in range(ROWS)], max_samples=N),
    }


def run(label, out_path, calls=CALLS):
    from libear_amd import capi
    from libear_amd.build import lib_path
    ctx = capi.Context(0)  # raises without a GPU: nothing is timed on a CPU
    x = np.random.default_rng(4).uniform(-1.0, 1.0, (ROWS, N)).astype(np.float32)
    result = {"label": label, "lib": os.path.relpath(lib_path(), ROOT), "rows": ROWS, "samples": N, "calls": calls, "stages": {}}
    for name, make in stages(capi, ctx).items():
        make().close()
        ctx.synchronize()
        t0 = time.perf_counter()
        st = make()
        create_ms = 1e3 * (time.perf_counter() - t0)
        times = []
        for i in range(WARM + calls):
            t0 = time.perf_counter()
            st.process(x)
            times.append(1e3 * (time.perf_counter() - t0))
        st.close()
        t = np.array(times[WARM:])
        result["stages"][name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                                  "create_ms": create_ms, "times_ms": [round(float(v), 4) for v in t]}
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


def compare(parent, again, new, out_path):
    a, b, c = (json.load(open(p)) for p in (parent, again, new))
    med = lambda r, s: r["stages"][s]["median_ms"]
    names = list(a["stages"])
    margin = max(abs(med(a, s) - med(b, s)) / min(med(a, s), med(b, s)) for s in names)
    verdict = {s: {"parent_ms": med(a, s), "parent_again_ms": med(b, s), "new_ms": med(c, s), "new_over_parent": med(c, s) / med(a, s) - 1.0,
                   "within_margin": med(c, s) <= med(a, s) * (1.0 + margin)} for s in names}
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
    pooled = {}
    for label, rs in parts.items():
        m = dict(rs[0], calls=sum(q["calls"] for q in rs), rounds=ROUNDS, stages={})
        for name in rs[0]["stages"]:
            t = np.concatenate([q["stages"][name]["times_ms"] for q in rs])
            m["stages"][name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                                 "create_ms": float(np.median([q["stages"][name]["create_ms"] for q in rs])),
                                 "round_medians_ms": [q["stages"][name]["median_ms"] for q in rs]}
        pooled[label] = os.path.join(outdir, f"{label}.json")
        with open(pooled[label], "w") as f:
            json.dump(m, f, indent=1)
    return compare(pooled["parent"], pooled["parent_again"], pooled["new"], os.path.join(outdir, "bus_stage_host_ab.json"))


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"] and len(sys.argv) in (4, 5):
        run(sys.argv[2], sys.argv[3], *[int(v) for v in sys.argv[4:]])
    elif sys.argv[1:2] == ["alternate"] and len(sys.argv) == 4:
        sys.exit(0 if alternate(sys.argv[2], sys.argv[3]) else 1)
    elif sys.argv[1:2] == ["compare"] and len(sys.argv) == 6:
        sys.exit(0 if compare(*sys.argv[2:6]) else 1)
    else:
        sys.exit(__doc__)
