"""Rate of the allocentric panner's device form with extent, channelLock and divergence (earhip_allo_calculate_objects_device)
on resident arrays for 0+5+0 (6 channels) and 9+10+3 (24 channels), five cases each: plain rows; all with extent; all diverged
with extent; a third each locked, diverged and masked; all masked with extent.  In the same run: a device copy of the same
output bytes (direct and diffuse rows), earhip_allo_calculate_device on the same positions, and
earhip_panner_calculate_objects_device (the polar producer) on the positions and sizes converted to polar, with the extent
case's sizes; one JSON line.

usage: python tools/allo_objects_rate.py [positions (262144)] [most steps per window (200)]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from libear_amd import capi  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = capi.Context(0, stream.cuda_stream)
rng = np.random.default_rng(21)


def resident(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


x, y, z = (resident(rng.uniform(-1, 1, n)) for _ in range(3))
gain = resident(rng.uniform(0.1, 1, n))
diffuse = resident(rng.uniform(0, 1, n))
sizes = [resident(rng.choice([0.03, 0.1, 0.2, 0.5, 1.0], n)) for _ in range(3)]  # width, height, depth
v_all = resident(rng.uniform(0.1, 1.0, n))
r_all = resident(rng.uniform(0.0, 0.5, n))
third = np.arange(n) % 3
lock_third = resident((third == 0).astype(np.uint8))
v_third = resident(np.where(third == 1, rng.uniform(0.1, 1.0, n), 0.0))
r_third = resident(np.where(third == 1, rng.uniform(0.0, 0.5, n), 0.0))
status = torch.empty(n, dtype=torch.int32, device=dev)
az, el, dist, pw, ph, pd = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(6))
capi.to_polar_device(ctx, n, x, y, z, az, el, dist, *sizes, pw, ph, pd)

calls, shapes, keep = {}, {}, []
for layout in ("0+5+0", "9+10+3"):
    allo = capi.Allo(layout)
    pan = capi.Panner(ctx, layout)
    nc = allo.n_out
    speakers = sum(1 << c for c, ch in enumerate(capi.layout_channels(layout)) if not ch[3])
    m = rng.integers(0, 1 << nc, n, dtype=np.uint32) & rng.integers(0, 1 << nc, n, dtype=np.uint32) & speakers
    mask = resident(m.view(np.int32))
    mask_third = resident(np.where(third == 2, m, 0).astype(np.uint32).view(np.int32))
    direct = torch.empty((n, nc), dtype=torch.float32, device=dev)
    diffuse_out = torch.empty_like(direct)
    src = torch.rand((2, n, nc), dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    keep.append((allo, pan))
    shapes[layout] = src.numel() * 4

    def objects(a=allo, d=direct, f=diffuse_out, size=(None, None, None), lock=None, v=None, r=None, k=None):
        capi.allo_calculate_objects_device(ctx, a, n, x, y, z, *size, gain, diffuse, lock, None, v, r, k, d, f, status=status)

    calls[f"objects_{layout}_plain"] = objects
    calls[f"objects_{layout}_extent"] = lambda o=objects: o(size=sizes)
    calls[f"objects_{layout}_diverged_extent"] = lambda o=objects: o(size=sizes, v=v_all, r=r_all)
    calls[f"objects_{layout}_thirds"] = lambda o=objects, k=mask_third: o(lock=lock_third, v=v_third, r=r_third, k=k)
    calls[f"objects_{layout}_masked_extent"] = lambda o=objects, k=mask: o(size=sizes, k=k)
    calls[f"device_copy_{layout}"] = lambda s=src, d=dst: d.copy_(s)
    calls[f"allo_calculate_device_{layout}"] = lambda a=allo, d=direct, f=diffuse_out: capi.allo_calculate_device(
        ctx, a, n, x, y, z, gain, diffuse, None, d, f, status=status)
    calls[f"panner_calculate_objects_device_{layout}"] = lambda p=pan, d=direct, f=diffuse_out: p.calculate_objects_device(
        n, az.data_ptr(), el.data_ptr(), dist.data_ptr(), gain.data_ptr(), diffuse.data_ptr(), d.data_ptr(), f.data_ptr(),
        width=pw.data_ptr(), height=ph.data_ptr(), depth=pd.data_ptr())


def window(step, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        step()
    torch.cuda.synchronize()
    return n * count / (time.perf_counter() - t0) / 1e6


counts = {}
for name, step in calls.items():  # warm up every shape; a window is `steps` calls, or fewer once they fill 0.2 s
    step()
    once = n / window(step, 1) / 1e6
    counts[name] = max(1, min(steps, int(0.2 / once)))
    if name.startswith(("objects", "allo")):
        assert int(status.sum().item()) == 0
# the calls alternate, five rounds; the median window of each
rates = {name: [] for name in calls}
for _ in range(5):
    for name, step in calls.items():
        rates[name].append(window(step, counts[name]))
res = {"metric": "gain vectors (a direct and a diffuse row) per second of the allocentric panner with extent, channelLock and "
                 "divergence on resident positions", "unit": "Mvectors/s", "positions": n, "steps_per_window": counts, "windows": 5}
for name, r in rates.items():
    res[name] = round(float(np.median(r)), 2)
    res[name + "_spread"] = [round(min(r), 2), round(max(r), 2)]
for layout, nbytes in shapes.items():
    res[f"{layout}_output_bytes"] = nbytes
    res[f"{layout}_plain_vs_copy"] = round(res[f"objects_{layout}_plain"] / res[f"device_copy_{layout}"], 4)
    res[f"{layout}_plain_vs_allo_calculate_device"] = round(res[f"objects_{layout}_plain"] / res[f"allo_calculate_device_{layout}"], 4)
    res[f"{layout}_extent_vs_polar_objects"] = round(res[f"objects_{layout}_extent"] / res[f"panner_calculate_objects_device_{layout}"], 4)
    res[f"{layout}_masked_extent_vs_extent"] = round(res[f"objects_{layout}_masked_extent"] / res[f"objects_{layout}_extent"], 4)
for allo, pan in keep:
    allo.close()
    pan.close()
print(json.dumps(res))
