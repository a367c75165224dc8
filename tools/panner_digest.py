"""SHA-256 of what the Objects gain producer's entry points (include/earhip.h group I) compute for a fixed list of calls:
    python tools/panner_digest.py            (EARHIP_LIB=<another build of libearhip.so>: the same list through that build)
One line per case: its name, earhip_panner_missed after the call, the digests of the direct and the diffuse rows.  4,096 seeded
positions per call — directions on the 15-degree grid and on the loudspeakers among them, distances 0.1 to 2, extents with depth
— through the plain, the extent and the Objects forms (lock, divergence and zones each alone, together, and all five arrays
absent), each in its host and its _device form, on 0+2+0, 0+5+0, 4+5+0, 9+10+3, 4+5+0 at real positions and a defined layout;
an empty call; the HOA decode matrix at orders 1 and 3 in the three normalisations with and without positions; every field of
the self-check report; a DirectSpeakers call whose channels fall back to the panner.  Every job of the device writes its own
rows, so two runs of one build print the same file, and two builds whose host code enqueues the same kernels on the same data
print the same file: a refactor of the producer's host code is compared this way."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch  # (before the library touches the device: one HIP runtime per process, torch's — as bench.py does)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import custom_layout_model as model  # noqa: E402
from libear_amd import capi  # noqa: E402

N = 4096
F64 = ("az", "el", "dist", "width", "height", "depth", "gain", "diffuse", "lock_max", "divergence", "az_range")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def inputs(channels, seed):
    rng = np.random.default_rng(seed)
    q = N // 4
    v = {"az": rng.uniform(-180.0, 180.0, N), "el": rng.uniform(-90.0, 90.0, N)}
    v["az"][:q] = rng.integers(-12, 13, q) * 15.0
    v["el"][:q] = rng.integers(-6, 7, q) * 15.0
    real = [c for c in channels if not c[3]]
    pick = rng.integers(0, len(real), q)
    v["az"][q:2 * q] = [real[k][1] for k in pick]
    v["el"][q:2 * q] = [real[k][2] for k in pick]
    v["dist"] = np.where(rng.random(N) < 0.3, 1.0, rng.uniform(0.1, 2.0, N))
    v["width"] = np.where(rng.random(N) < 0.3, 0.0, rng.uniform(0.0, 360.0, N))
    v["height"] = np.where(rng.random(N) < 0.3, 0.0, rng.uniform(0.0, 180.0, N))
    v["depth"] = np.where(rng.random(N) < 0.5, 0.0, rng.uniform(0.0, 1.0, N))
    v["gain"] = rng.uniform(0.0, 2.0, N)
    v["diffuse"] = rng.uniform(0.0, 1.0, N)
    v["lock"] = (rng.random(N) < 0.5).astype(np.uint8)
    v["lock_max"] = np.where(rng.random(N) < 0.5, np.inf, rng.uniform(0.0, 1.0, N))
    v["divergence"] = np.where(rng.random(N) < 0.3, 0.0, rng.uniform(0.0, 1.0, N))
    v["az_range"] = rng.uniform(0.0, 180.0, N)
    v["excluded"] = np.where(rng.random(N) < 0.3, 0, rng.integers(0, 1 << len(channels), N)).astype(np.uint32)
    return v


# which arrays a form passes besides az, el, gain and diffuse
POINT = ("dist",)
EXTENT = POINT + ("width", "height", "depth")
FORMS = [("plain", POINT), ("extent", EXTENT), ("objects_none", EXTENT), ("objects_lock", EXTENT + ("lock", "lock_max")),
         ("objects_divergence", EXTENT + ("divergence", "az_range")), ("objects_zones", EXTENT + ("excluded",)),
         ("objects_all", EXTENT + ("lock", "lock_max", "divergence", "az_range", "excluded")),
         ("objects_all_points", ("lock", "lock_max", "divergence", "az_range", "excluded"))]
ORDER = ("dist", "width", "height", "depth", "gain", "diffuse", "lock", "lock_max", "divergence", "az_range", "excluded")


def call(p, ctx, form, use, v, n, device):
    """one entry point through the library's own symbols -> (status, direct, diffuse)"""
    lib = capi.load()
    use = use + ("gain", "diffuse")
    d = np.full((max(n, 1), p.n_out), 7.5, np.float32)  # (an empty call still gets pointers)
    f = np.full((max(n, 1), p.n_out), 7.5, np.float32)
    if device:
        keep = {k: torch.from_numpy(np.ascontiguousarray(v[k][:max(n, 1)])).cuda() for k in ("az", "el") + use}
        dd, df = torch.from_numpy(d).cuda(), torch.from_numpy(f).cuda()
        torch.cuda.synchronize()
        ptr = {k: C.c_void_p(t.data_ptr()) for k, t in keep.items()}
        out = (C.c_void_p(dd.data_ptr()), C.c_void_p(df.data_ptr()))
    else:
        keep = {k: np.ascontiguousarray(v[k][:max(n, 1)]) for k in ("az", "el") + use}
        ptr = {k: C.c_void_p(a.ctypes.data) for k, a in keep.items()}
        out = (C.c_void_p(d.ctypes.data), C.c_void_p(f.ctypes.data))
    names = {"plain": ("dist", "gain", "diffuse"), "extent": ORDER[:6]}.get(form, ORDER)
    fn = getattr(lib, "earhip_panner_calculate" + {"plain": "", "extent": "_extent"}.get(form, "_objects") + ("_device" if device else ""))
    status = fn(p.h, C.c_size_t(n), ptr["az"], ptr["el"], *[ptr.get(k) for k in names], *out)
    if device:
        ctx.synchronize()
        d, f = dd.cpu().numpy(), df.cpu().numpy()
    return status, d, f


def panner_cases(ctx, name, layout, positions, seed):
    channels = capi.layout_channels(layout)
    v = inputs(channels, seed)
    p = capi.Panner(ctx, layout, positions)
    for form, use in FORMS:
        for device in (False, True):
            status, d, f = call(p, ctx, form, use, v, N, device)
            print(f"{name + ' ' + form + ('_device' if device else ''):48s} status {status} missed {p.missed()} {sha(d)} {sha(f)}")
    for device in (False, True):
        status, d, f = call(p, ctx, "objects_all", FORMS[6][1], v, 0, device)
        print(f"{name + ' empty' + ('_device' if device else ''):48s} status {status} missed {p.missed()}")
    r = p.self_check()
    print(f"{name + ' self_check':48s} " + " ".join(f"{k} {getattr(r, k)!r}" for k, _ in capi.PannerReport._fields_) +
          f" {sha(np.array([r.max_power_error, r.min_own_gain]))}")
    p.close()


def moved(layout, seed=5):
    channels = capi.layout_channels(layout)
    rng = np.random.default_rng(seed)
    return (np.array([c[1] for c in channels]) + rng.uniform(-3, 3, len(channels)),
            np.array([c[2] for c in channels]) + rng.uniform(-3, 3, len(channels)))


if __name__ == "__main__":
    capi.define_layout("6+9+0", model.CUSTOM["6+9+0"][0])
    ctx = capi.Context(0)
    for seed, (name, layout, positions) in enumerate([("0+2+0", "0+2+0", None), ("0+5+0", "0+5+0", None), ("4+5+0", "4+5+0", None),
                                                      ("9+10+3", "9+10+3", None), ("4+5+0_moved", "4+5+0", moved("4+5+0")),
                                                      ("defined_6+9+0", "6+9+0", None)]):
        panner_cases(ctx, name, layout, positions, 100 + seed)
    for order in (1, 3):
        orders = [n for n in range(order + 1) for _ in range(2 * n + 1)]
        degrees = [m for n in range(order + 1) for m in range(-n, n + 1)]
        for norm in ("N3D", "SN3D", "FuMa"):
            for name, layout, positions in (("0+2+0", "0+2+0", None), ("9+10+3", "9+10+3", None), ("4+5+0_moved", "4+5+0", moved("4+5+0")),
                                            ("defined_6+9+0", "6+9+0", None)):
                D = capi.hoa_decode_matrix(ctx, layout, orders, degrees, norm, positions)
                print(f"{'decode ' + name + ' order ' + str(order) + ' ' + norm:48s} {sha(D)}")
    for name, layout, positions in (("9+10+3", "9+10+3", None), ("4+5+0_moved", "4+5+0", moved("4+5+0"))):
        ds = capi.DirectSpeakers(ctx, layout, positions=positions)
        rng = np.random.default_rng(77)
        md = [{"speakerLabels": ["X%d" % k], "azimuth": float(a), "elevation": float(e)}
              for k, (a, e) in enumerate(zip(rng.uniform(-180, 180, 256), rng.uniform(-90, 90, 256)))]
        gains, warnings = ds.calculate(md)
        print(f"{'direct_speakers ' + name:48s} missed {ds.missed()} {sha(gains)} {sha(warnings)}")
        ds.close()
    ctx.close()
