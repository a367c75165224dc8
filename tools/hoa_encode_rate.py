"""Rate of the Ambisonic encoder's device form (earhip_hoa_encode_device) on resident arrays at order 3 (16 channels) and order 7
(64 channels), next to a device copy of the same output bytes and to earhip_panner_calculate_device (the loudspeaker gain
producer) on the same positions, in the same run; one JSON line.

usage: python tools/hoa_encode_rate.py [positions (262144)] [layout of the panner (9+10+3)] [steps per window (50)]"""
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
az = torch.from_numpy(rng.uniform(-180, 180, n)).to(dev)
el = torch.from_numpy(np.degrees(np.arcsin(rng.uniform(-1, 1, n)))).to(dev)
gain = torch.from_numpy(rng.uniform(0.1, 1, n)).to(dev)
diffuse = torch.zeros(n, dtype=torch.float64, device=dev)
direct = torch.empty((n, pan.n_out), dtype=torch.float32, device=dev)
diffuse_out = torch.empty_like(direct)
status = torch.empty(n, dtype=torch.int32, device=dev)

calls = {"panner_calculate_device": lambda: pan.calculate_device(n, az.data_ptr(), el.data_ptr(), None, gain.data_ptr(),
                                                                 diffuse.data_ptr(), direct.data_ptr(), diffuse_out.data_ptr())}
outs = {}
for order in (3, 7):
    o, d = capi.hoa_acn(order)
    out = torch.empty((n, len(o)), dtype=torch.float32, device=dev)
    src = torch.rand((n, len(o)), dtype=torch.float32, device=dev)
    outs[order] = (out, src)
    calls[f"hoa_encode_device_order{order}"] = lambda o=o, d=d, out=out: capi.hoa_encode_device(
        ctx, n, az, el, gain, out, o, d, "SN3D", status=status)
    calls[f"device_copy_order{order}"] = lambda out=out, src=src: out.copy_(src)


def window(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return n * steps / (time.perf_counter() - t0) / 1e6


for step in calls.values():  # warm up every shape
    for _ in range(3):
        step()
    torch.cuda.synchronize()
assert pan.missed() == 0 and int(status.sum().item()) == 0
# the calls alternate, five rounds; the median window of each
rates = {name: [] for name in calls}
for _ in range(5):
    for name, step in calls.items():
        rates[name].append(window(step))
res = {"metric": "gain vectors per second of the Ambisonic encoder (Objects -> HOA bus) on resident positions",
       "unit": "Mvectors/s", "positions": n, "panner_layout": layout, "steps_per_window": steps, "windows": 5}
for name, r in rates.items():
    res[name] = round(float(np.median(r)), 2)
    res[name + "_spread"] = [round(min(r), 2), round(max(r), 2)]
for order, (out, _) in outs.items():
    nbytes = out.numel() * 4
    res[f"order{order}_output_bytes"] = nbytes
    res[f"order{order}_output_GBps"] = round(res[f"hoa_encode_device_order{order}"] * 1e6 / n * nbytes / 1e9, 1)
    res[f"order{order}_vs_copy"] = round(res[f"hoa_encode_device_order{order}"] / res[f"device_copy_order{order}"], 3)
pan.close()
print(json.dumps(res))
