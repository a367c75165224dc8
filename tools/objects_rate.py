"""Rate of the Objects gain producer with channelLock, objectDivergence and zoneExclusion
(earhip_panner_calculate_objects_device) on resident arrays, next to earhip_panner_calculate_extent_device on the same
positions in the same run; one JSON line.  The positions are those of `bench.py --producer`: widths 0-120, heights 0-60 degrees,
distances 0.5-1.5, a quarter with depth.  Three mixes of the new metadata: (a) none (arrays of zeros: every row takes the front
pass and then the extent form's kernels), (b) every object diverged, (c) a third locked, a third diverged, a third with a zone.

usage: python tools/objects_rate.py [positions (262144)] [layout (9+10+3)] [steps per window (50)]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from libear_amd import capi  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
layout = sys.argv[2] if len(sys.argv) > 2 else "9+10+3"
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = capi.Context(0, stream.cuda_stream)
pan = capi.Panner(ctx, layout)
rng = np.random.default_rng(21)
host = {"az": rng.uniform(-180, 180, n), "el": np.degrees(np.arcsin(rng.uniform(-1, 1, n))), "dist": rng.uniform(0.5, 1.5, n),
        "width": rng.uniform(0, 120, n), "height": rng.uniform(0, 60, n),
        "depth": np.where(rng.uniform(0, 1, n) < 0.25, rng.uniform(0, 0.5, n), 0.0), "gain": rng.uniform(0.1, 1, n),
        "diffuse": rng.choice([0.0, 0.3, 1.0], n)}
zone = capi.objects_excluded_channels(layout, [dict(min_azimuth=-180.0, max_azimuth=180.0, min_elevation=10.0, max_elevation=90.0)])
third = rng.integers(0, 3, n)
mixes = {
    "a_none": dict(lock=np.zeros(n, np.uint8), div=np.zeros(n), mask=np.zeros(n, np.uint32)),
    "b_all_diverged": dict(lock=np.zeros(n, np.uint8), div=rng.uniform(0.1, 1.0, n), mask=np.zeros(n, np.uint32)),
    "c_thirds": dict(lock=(third == 0).astype(np.uint8), div=np.where(third == 1, rng.uniform(0.1, 1.0, n), 0.0),
                     mask=np.where(third == 2, zone, 0).astype(np.uint32)),
}
d_in = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
az_range = torch.from_numpy(rng.uniform(10.0, 60.0, n)).to(dev)
direct = torch.empty((n, pan.n_out), dtype=torch.float32, device=dev)
diffuse = torch.empty_like(direct)
common = (n, d_in["az"].data_ptr(), d_in["el"].data_ptr(), d_in["dist"].data_ptr(), d_in["gain"].data_ptr(),
          d_in["diffuse"].data_ptr(), direct.data_ptr(), diffuse.data_ptr(), d_in["width"].data_ptr(), d_in["height"].data_ptr(),
          d_in["depth"].data_ptr())


def window(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return n * steps / (time.perf_counter() - t0) / 1e6


t_in = {name: {k: torch.from_numpy(v).to(dev) for k, v in m.items()} for name, m in mixes.items()}
calls = {"calculate_extent_device": lambda: pan.calculate_device(*common)}
for name, t in t_in.items():
    calls["calculate_objects_device_" + name] = lambda t=t: pan.calculate_objects_device(
        *common, t["lock"].data_ptr(), None, t["div"].data_ptr(), az_range.data_ptr(), t["mask"].data_ptr())
for step in calls.values():  # warm up every shape
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    assert pan.missed() == 0
# the four alternate, five rounds; the median window of each
rates = {name: [] for name in calls}
for _ in range(5):
    for name, step in calls.items():
        rates[name].append(window(step))
out = {"metric": "gain vectors per second of the Objects gain producer with channelLock, objectDivergence and zoneExclusion",
       "unit": "Mpositions/s", "positions": n, "layout": layout, "steps_per_window": steps, "windows": 5}
for name, r in rates.items():
    out[name] = round(float(np.median(r)), 2)
    out[name + "_spread"] = [round(min(r), 2), round(max(r), 2)]
for name in t_in:
    out["ratio_" + name] = round(out["calculate_objects_device_" + name] / out["calculate_extent_device"], 3)
pan.close()
print(json.dumps(out))
