"""Rate of the screen stage for Cartesian positions (earhip_screen_apply_cartesian_device, include/earhip.h group V) on resident
arrays, next to the three launches it fuses (earhip_conversion_to_polar_device, earhip_screen_apply_device,
earhip_conversion_to_cartesian_device on the same arrays), a device copy of the three float64 arrays, and the stage it stands in
front of, earhip_allo_calculate_objects_device, on the same positions in the same run; one JSON line.  Every object has
screenRef set (default reference screen, a 30 degree reproduction screen), a quarter a horizontal and a quarter a vertical
lock.  The fused stage reads 24 + 3 bytes and writes 24 per element; the three launches move 48 + 35 + 48; the copy 24 + 24.

A call is a few microseconds to a few tens, so each call gets its own number of steps per window: as many as fill about a
quarter of a second, found by a short calibration.

usage: python tools/screen_cart_rate.py [positions (262144)] [layout of the panner (9+10+3)] [seconds per window (0.25)]"""
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
allo = capi.Allo(layout)
rng = np.random.default_rng(21)
xyz = [torch.from_numpy(rng.uniform(-1, 1, n)).to(dev) for _ in range(3)]
fused = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3)]    # written by the fused stage
polar = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3)]    # the chain's intermediate
chained = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3)]  # written by the chain's last launch
copy_src = torch.stack(xyz)
copied = torch.empty_like(copy_src)
screen_ref = torch.ones(n, dtype=torch.uint8, device=dev)
lock_h = torch.from_numpy(np.where(rng.uniform(0, 1, n) < 0.25, rng.integers(1, 3, n), 0).astype(np.uint8)).to(dev)
lock_v = torch.from_numpy(np.where(rng.uniform(0, 1, n) < 0.25, rng.integers(1, 3, n), 0).astype(np.uint8)).to(dev)
status = torch.empty(n, dtype=torch.int32, device=dev)
direct = torch.empty((n, allo.n_out), dtype=torch.float32, device=dev)
reproduction = capi.Screen.polar(1.78, 0.0, 0.0, 1.0, 30.0)


def chain():
    capi.to_polar_device(ctx, n, *xyz, *polar)
    capi.screen_apply_device(ctx, n, polar[0], polar[1], polar[0], polar[1], reproduction, None, screen_ref, lock_h, lock_v)
    capi.to_cartesian_device(ctx, n, *polar, *chained)


calls = {
    "screen_apply_cartesian_device": lambda: capi.screen_apply_cartesian_device(ctx, n, *xyz, *fused, reproduction, None,
                                                                                screen_ref, lock_h, lock_v, status=status),
    "three_launch_chain": chain,
    "device_copy": lambda: copied.copy_(copy_src),
    "allo_calculate_objects_device": lambda: capi.allo_calculate_objects_device(ctx, allo, n, *fused, *[None] * 10, direct, None),
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
    steps[name] = int(min(max(seconds / (window(step, 20) / 20), 20), 50000))
assert int(status.sum().item()) == 0
# the fused stage gave the bits of the three launches on these positions
for a, b in zip(fused, chained):
    assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))
# the calls alternate, five rounds; the median window of each
rates = {name: [] for name in calls}
for _ in range(5):
    for name, step in calls.items():
        rates[name].append(n * steps[name] / window(step, steps[name]) / 1e6)
res = {"metric": "positions per second of the screen stage for Cartesian positions (to polar, screenRef scaling and "
                 "screenEdgeLock, back to Cartesian, in one kernel) on resident positions",
       "unit": "Mpositions/s", "positions": n, "panner_layout": layout, "seconds_per_window": seconds, "windows": 5,
       "steps_per_window": steps}
for name, r in rates.items():
    res[name] = round(float(np.median(r)), 2)
    res[name + "_spread"] = [round(min(r), 2), round(max(r), 2)]
res["fused_bytes_per_position"] = 51
res["chain_bytes_per_position"] = 131
res["copy_bytes_per_position"] = 48
res["fused_GBps"] = round(res["screen_apply_cartesian_device"] * 51 / 1e3, 1)
res["copy_GBps"] = round(res["device_copy"] * 48 / 1e3, 1)
res["fused_us_per_call"] = round(n / res["screen_apply_cartesian_device"], 2)
res["fused_vs_chain"] = round(res["screen_apply_cartesian_device"] / res["three_launch_chain"], 3)
res["fused_vs_copy"] = round(res["screen_apply_cartesian_device"] / res["device_copy"], 3)
res["stage_share_of_stage_plus_panner_time"] = round(
    (1 / res["screen_apply_cartesian_device"]) / (1 / res["screen_apply_cartesian_device"]
                                                  + 1 / res["allo_calculate_objects_device"]), 5)
allo.close()
print(json.dumps(res))
