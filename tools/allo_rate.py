"""Rate of the allocentric panner's device form (earhip_allo_calculate_device) on resident arrays for 0+5+0 (6 channels) and
9+10+3 (24 channels), with and without exclusion masks, next to a device copy of the same output bytes (direct and diffuse
rows) and to earhip_panner_calculate_device (the polar point-source panner) on the same positions converted to polar, in the
same run; one JSON line.

usage: python tools/allo_rate.py [positions (262144)] [steps per window (500)]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from libear_amd import capi  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 500  # (a window of the fastest call is then 8 ms or more)
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = capi.Context(0, stream.cuda_stream)
rng = np.random.default_rng(21)
x, y, z = (torch.from_numpy(rng.uniform(-1, 1, n)).to(dev) for _ in range(3))
gain = torch.from_numpy(rng.uniform(0.1, 1, n)).to(dev)
diffuse = torch.from_numpy(rng.uniform(0, 1, n)).to(dev)
status = torch.empty(n, dtype=torch.int32, device=dev)
az, el, dist = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
capi.to_polar_device(ctx, n, x, y, z, az, el, dist)

calls, shapes, keep = {}, {}, []
for layout in ("0+5+0", "9+10+3"):
    allo = capi.Allo(layout)
    pan = capi.Panner(ctx, layout)
    nc = allo.n_out
    speakers = sum(1 << c for c, ch in enumerate(capi.layout_channels(layout)) if not ch[3])
    m = rng.integers(0, 1 << nc, n, dtype=np.uint32) & rng.integers(0, 1 << nc, n, dtype=np.uint32) & speakers
    mask = torch.from_numpy(m.view(np.int32)).to(dev)
    direct = torch.empty((n, nc), dtype=torch.float32, device=dev)
    diffuse_out = torch.empty_like(direct)
    src = torch.rand((2, n, nc), dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    keep.append((allo, pan))
    shapes[layout] = src.numel() * 4
    calls[f"allo_{layout}"] = lambda a=allo, d=direct, f=diffuse_out: capi.allo_calculate_device(
        ctx, a, n, x, y, z, gain, diffuse, None, d, f, status=status)
    calls[f"allo_{layout}_masks"] = lambda a=allo, d=direct, f=diffuse_out, k=mask: capi.allo_calculate_device(
        ctx, a, n, x, y, z, gain, diffuse, k, d, f, status=status)
    calls[f"device_copy_{layout}"] = lambda s=src, d=dst: d.copy_(s)
    calls[f"panner_calculate_device_{layout}"] = lambda p=pan, d=direct, f=diffuse_out: p.calculate_device(
        n, az.data_ptr(), el.data_ptr(), dist.data_ptr(), gain.data_ptr(), diffuse.data_ptr(), d.data_ptr(), f.data_ptr())


def window(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return n * steps / (time.perf_counter() - t0) / 1e6


for name, step in calls.items():  # warm up every shape
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    if name.startswith("allo"):
        assert int(status.sum().item()) == 0
assert all(p.missed() == 0 for _, p in keep)
# the calls alternate, five rounds; the median window of each
rates = {name: [] for name in calls}
for _ in range(5):
    for name, step in calls.items():
        rates[name].append(window(step))
res = {"metric": "gain vectors (a direct and a diffuse row) per second of the allocentric panner on resident positions",
       "unit": "Mvectors/s", "positions": n, "steps_per_window": steps, "windows": 5}
for name, r in rates.items():
    res[name] = round(float(np.median(r)), 2)
    res[name + "_spread"] = [round(min(r), 2), round(max(r), 2)]
for layout, nbytes in shapes.items():
    res[f"{layout}_output_bytes"] = nbytes
    res[f"{layout}_output_GBps"] = round(res[f"allo_{layout}"] * 1e6 / n * nbytes / 1e9, 1)
    res[f"{layout}_vs_copy"] = round(res[f"allo_{layout}"] / res[f"device_copy_{layout}"], 3)
    res[f"{layout}_masks_vs_copy"] = round(res[f"allo_{layout}_masks"] / res[f"device_copy_{layout}"], 3)
    res[f"{layout}_vs_polar_panner"] = round(res[f"allo_{layout}"] / res[f"panner_calculate_device_{layout}"], 3)
for allo, pan in keep:
    allo.close()
    pan.close()
print(json.dumps(res))
