"""Rate of the screen stage's device form (earhip_screen_apply_device: screenRef scaling and screenEdgeLock, include/earhip.h
group R) on resident arrays, next to a device copy of the float64 bytes it moves and to the two stages it stands between,
earhip_conversion_to_polar_device and earhip_panner_calculate_objects_device, on the same positions in the same run; one JSON
line.  Every object has screenRef set (default reference screen, a 30 degree reproduction screen), a quarter a horizontal and
a quarter a vertical lock.  The stage reads 16 + 3 bytes and writes 16 per element; the copy reads 16 and writes 16.

A call of the stage is a few microseconds, so each call gets its own number of steps per window: as many as fill about a
quarter of a second, found by a short calibration.

usage: python tools/screen_rate.py [positions (262144)] [layout of the panner (9+10+3)] [seconds per window (0.25)]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from libear_amd import capi  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
layout = sys.argv[2] if len(sys.argv) > 2 else "9+10+3"
seconds = float(sys.argv[3]) if len(sys.argv) > 3 else 0.25
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = capi.Context(0, stream.cuda_stream)
pan = capi.Panner(ctx, layout)
rng = np.random.default_rng(21)
xyz = [torch.from_numpy(rng.uniform(-1, 1, n)).to(dev) for _ in range(3)]
polar = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3)]     # written by the conversion
scaled = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2)]    # written by the screen stage
copied = torch.empty((2, n), dtype=torch.float64, device=dev)
screen_ref = torch.ones(n, dtype=torch.uint8, device=dev)
lock_h = torch.from_numpy(np.where(rng.uniform(0, 1, n) < 0.25, rng.integers(1, 3, n), 0).astype(np.uint8)).to(dev)
lock_v = torch.from_numpy(np.where(rng.uniform(0, 1, n) < 0.25, rng.integers(1, 3, n), 0).astype(np.uint8)).to(dev)
status = torch.empty(n, dtype=torch.int32, device=dev)
direct = torch.empty((n, pan.n_out), dtype=torch.float32, device=dev)
diffuse = torch.empty_like(direct)
reproduction = capi.Screen.polar(1.78, 0.0, 0.0, 1.0, 30.0)
copy_src = torch.stack(polar[:2])

calls = {
    "conversion_to_polar_device": lambda: capi.to_polar_device(ctx, n, *xyz, *polar),
    "screen_apply_device": lambda: capi.screen_apply_device(ctx, n, polar[0], polar[1], scaled[0], scaled[1], reproduction, None,
                                                            screen_ref, lock_h, lock_v, status=status),
    "device_copy": lambda: copied.copy_(copy_src),
    "panner_calculate_objects_device": lambda: pan.calculate_objects_device(
        n, scaled[0].data_ptr(), scaled[1].data_ptr(), polar[2].data_ptr(), None, None, direct.data_ptr(), diffuse.data_ptr()),
}


def window(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


steps = {}
for name, step in calls.items():  # in pipeline order: warm up every shape, then calibrate
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    if name == "device_copy":
        copy_src = torch.stack(polar[:2])  # (the same values the stage reads)
    steps[name] = int(min(max(seconds / (window(step, 20) / 20), 20), 50000))
assert pan.missed() == 0 and int(status.sum().item()) == 0
# the screen stage gave the host form's bits on these positions
h_az, h_el = capi.screen_apply(polar[0].cpu().numpy(), polar[1].cpu().numpy(), reproduction, None, screen_ref.cpu().numpy(),
                               lock_h.cpu().numpy(), lock_v.cpu().numpy())
assert np.array_equal(scaled[0].cpu().numpy().view(np.uint64), h_az.view(np.uint64))
assert np.array_equal(scaled[1].cpu().numpy().view(np.uint64), h_el.view(np.uint64))
# the calls alternate, five rounds; the median window of each
rates = {name: [] for name in calls}
for _ in range(5):
    for name, step in calls.items():
        rates[name].append(n * steps[name] / window(step, steps[name]) / 1e6)
res = {"metric": "positions per second of the screen stage (screenRef scaling and screenEdgeLock) on resident positions",
       "unit": "Mpositions/s", "positions": n, "panner_layout": layout, "seconds_per_window": seconds, "windows": 5,
       "steps_per_window": steps}
for name, r in rates.items():
    res[name] = round(float(np.median(r)), 2)
    res[name + "_spread"] = [round(min(r), 2), round(max(r), 2)]
res["screen_bytes_per_position"] = 35
res["copy_bytes_per_position"] = 32
res["screen_GBps"] = round(res["screen_apply_device"] * 35 / 1e3, 1)
res["copy_GBps"] = round(res["device_copy"] * 32 / 1e3, 1)
res["screen_us_per_call"] = round(n / res["screen_apply_device"], 2)
res["screen_vs_copy"] = round(res["screen_apply_device"] / res["device_copy"], 3)
res["screen_share_of_chain_time"] = round(
    (1 / res["screen_apply_device"]) / sum(1 / res[k] for k in ("conversion_to_polar_device", "screen_apply_device",
                                                                 "panner_calculate_objects_device")), 5)
pan.close()
print(json.dumps(res))
