"""channelLock, objectDivergence and zoneExclusion on the device (libearhip group I, earhip_panner_calculate_objects:
k_pan_objects_front and k_pan_objects_meta) against tests/objects_model.py, which restates the header's specification in
numpy float64 over the oracle's PolarExtent.

Tolerance: everything goes through the extent panner's float sums, so the bound is that of tests/test_gpu_extent.py — 1e-5 of
a gain vector's norm, the bound libear's tests put between its own cores.  What comes after the extent panner (a weighted sum
of three powers, a downmix with weights 1/m, one square root, all in double) adds rounding errors of the order of 1e-16.

A channel lock is a discontinuous choice: an object within 1e-6 of a tie between two loudspeakers, or of its maxDistance, may
lock differently in the model (the distances themselves are only good to 1e-16, but the positions come from different sin /
cos).  Such objects are left out of the comparison; they must be at most 1 % of the objects (random positions give 5e-6)."""
import numpy as np
import pytest

import objects_model as om
from _hip import ctx
from layouts import LAYOUTS
from test_gpu_extent import TOL, rel, scene

pytestmark = pytest.mark.gpu

N = 1500


def metadata(rng, layout, n):
    """a quarter locked (half of those with a maxDistance), a quarter diverged, a quarter with a zone mask, an eighth with
    all three, the rest plain -> dict of the five arrays"""
    n_full = len(LAYOUTS[layout])
    real = [i for i, nm in enumerate(LAYOUTS[layout]) if not nm.startswith("LFE")]
    lfe = sum(1 << i for i in range(n_full) if i not in real)
    every = sum(1 << i for i in real)
    kind = rng.choice(5, n, p=[0.25, 0.25, 0.25, 0.125, 0.125])  # lock, divergence, mask, all three, plain
    lock = np.isin(kind, (0, 3)).astype(np.uint8)
    lock_max = np.where(rng.uniform(0, 1, n) < 0.5, rng.uniform(0.1, 1.5, n), np.inf)
    div = np.where(np.isin(kind, (1, 3)), 1.0 - rng.uniform(0.0, 1.0, n), 0.0)  # (0, 1]
    div[np.isin(kind, (1, 3)) & (rng.uniform(0, 1, n) < 0.1)] = 1.0
    az_range = rng.uniform(0.0, 90.0, n)
    masks = rng.integers(0, 1 << n_full, n).astype(np.uint32)
    pick = rng.uniform(0, 1, n)
    masks[pick < 0.05] = every
    masks[(pick >= 0.05) & (pick < 0.1)] = every | lfe
    masks[(pick >= 0.1) & (pick < 0.15)] = lfe
    masks[~np.isin(kind, (2, 3))] = 0
    masks[(kind == 4) & (pick < 0.3)] = lfe  # (LFE bits alone: still a plain row)
    plain = (lock == 0) & (div == 0.0) & ((masks & every) == 0)
    return dict(channel_lock=lock, lock_max_distance=lock_max, divergence=div, azimuth_range=az_range, excluded=masks), plain


def draw(rng, layout, n):
    az, el, dist, width, height, depth, gain, diffuse = scene(rng, n)
    # the poles, the origin, the loudspeakers themselves
    el[:4] = [90.0, -90.0, 90.0 - 1e-6, -90.0 + 1e-6]
    dist[4:8] = [0.0, 1e-12, 1.0, 1.0]
    depth[4:6] = [0.0, 0.5]
    from libear_amd import capi
    for i, (_, caz, cel, _) in enumerate(capi.layout_channels(layout)):
        az[10 + i], el[10 + i] = caz, cel
    # point sources on the sphere too (no job for the extent kernel)
    dist[40:140] = 1.0
    width[40:140] = height[40:140] = depth[40:140] = 0.0
    return az, el, dist, width, height, depth, gain, diffuse


def compare(layout, positions, seed):
    from libear_amd import capi
    rng = np.random.default_rng(seed)
    az, el, dist, width, height, depth, gain, diffuse = draw(rng, layout, N)
    md, plain = metadata(rng, layout, N)
    p = capi.Panner(ctx(), layout, positions)
    d, f = p.calculate_objects(az, el, dist, gain, diffuse, width, height, depth, **md)
    d0, f0 = p.calculate(az, el, dist, gain, diffuse, width, height, depth)
    p.close()
    model = om.Model(layout, positions)
    wd, wf = model.calculate(az, el, dist, width, height, depth, gain, diffuse, md["channel_lock"], md["lock_max_distance"],
                             md["divergence"], md["azimuth_range"], md["excluded"])
    margin = np.array([model.tie_margin(om.cart(az[i], el[i], dist[i]), md["lock_max_distance"][i]) if md["channel_lock"][i]
                       else np.inf for i in range(N)])
    sure = margin >= 1e-6
    assert np.count_nonzero(~sure) <= N // 100, np.count_nonzero(~sure)
    has_d, has_f = sure & (diffuse < 1.0), sure & (diffuse > 0.0)
    worst = max(np.max(rel(d[has_d], wd[has_d])), np.max(rel(f[has_f], wf[has_f])))
    print(f"{layout}: worst error {worst:.3e} of the norm, {np.count_nonzero(~sure)} objects near a tie")
    assert worst <= TOL, (np.argmax(rel(d, wd) * has_d), worst)
    assert not d[diffuse == 1.0].any() and not f[diffuse == 0.0].any()
    lfe = [i for i, nm in enumerate(LAYOUTS[layout]) if nm.startswith("LFE")]
    real = [i for i in range(len(LAYOUTS[layout])) if i not in lfe]
    assert not d[:, lfe].any() and not f[:, lfe].any()
    every = sum(1 << i for i in real)
    for c in real:  # an excluded channel is silent (unless the set holds every loudspeaker: that excludes nothing)
        gone = ((md["excluded"] >> c) & 1 == 1) & ((md["excluded"] & every) != every)
        assert not d[gone, c].any() and not f[gone, c].any()
    # plain rows have the bits of the extent form, whatever their neighbours are
    assert plain.sum() > N // 16
    assert np.array_equal(d[plain], d0[plain]) and np.array_equal(f[plain], f0[plain])


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_objects_equal_the_model(layout):
    compare(layout, None, sum(map(ord, layout)))


def test_objects_equal_the_model_with_real_positions():
    """loudspeakers anywhere inside the ranges BS.2051 allows them: the lock goes to the real positions, the priority order and
    the zone groups follow the nominal ones"""
    from libear_amd import capi
    layout = "4+7+0"
    rng = np.random.default_rng(77)
    az, el = [], []
    for (a0, a1), (e0, e1) in capi.layout_channel_ranges(layout):
        end = a1 + 360.0 if a1 < a0 else a1
        a = rng.uniform(a0, end)
        az.append(a - 360.0 if a > 180.0 else a)
        el.append(rng.uniform(e0, e1))
    compare(layout, (np.array(az), np.array(el)), 78)


def test_exact_ties_go_by_priority():
    from libear_amd import capi
    for layout, (az, el), want in (("9+10+3", (0.0, 0.0), "M+000"), ("0+2+0", (0.0, 0.0), "M-030"), ("0+5+0", (0.0, 90.0), "M+000"),
                                   ("4+5+0", (0.0, 90.0), "U-030")):
        p = capi.Panner(ctx(), layout)
        d, _ = p.calculate_objects(az, el, channel_lock=1)
        p.close()
        want_row = np.zeros(len(LAYOUTS[layout]))
        want_row[LAYOUTS[layout].index(want)] = 1.0
        assert np.max(np.abs(d[0] - want_row)) <= 1e-6, (layout, d[0])
    # out of reach of every loudspeaker: the object stays where it is
    p = capi.Panner(ctx(), "0+5+0")
    d, _ = p.calculate_objects(70.0, 0.0, channel_lock=1, lock_max_distance=0.1)
    d0, _ = p.calculate(70.0, 0.0)
    d1, _ = p.calculate_objects(70.0, 0.0, channel_lock=1, lock_max_distance=0.8)
    p.close()
    assert np.max(np.abs(d - d0)) <= 1e-6 and np.count_nonzero(d0[0]) == 2
    assert np.max(np.abs(d1[0] - np.eye(6)[LAYOUTS["0+5+0"].index("M+030")])) <= 1e-6


def test_plain_rows_permute_with_the_batch():
    from libear_amd import capi
    layout = "9+10+3"
    rng = np.random.default_rng(5)
    n = 2000
    az, el, dist, width, height, depth, gain, diffuse = scene(rng, n)
    dist[:300] = 1.0
    width[:300] = height[:300] = depth[:300] = 0.0
    md, plain = metadata(rng, layout, n)
    p = capi.Panner(ctx(), layout)
    d0, f0 = p.calculate(az, el, dist, gain, diffuse, width, height, depth)
    d, f = p.calculate_objects(az, el, dist, gain, diffuse, width, height, depth, **md)
    perm = rng.permutation(n)
    dp, fp = p.calculate_objects(az[perm], el[perm], dist[perm], gain[perm], diffuse[perm], width[perm], height[perm], depth[perm],
                                 **{k: v[perm] for k, v in md.items()})
    # no metadata arrays at all, and arrays of zeros: the extent form's bits
    da, fa = p.calculate_objects(az, el, dist, gain, diffuse, width, height, depth)
    dz, fz = p.calculate_objects(az, el, dist, gain, diffuse, width, height, depth, channel_lock=0, divergence=0.0, excluded=0)
    # ... and point sources without distance or extent arrays
    dq, fq = p.calculate_objects(az, el, gain=gain, diffuse=diffuse, divergence=np.where(plain, 0.0, 0.3))
    dq0, fq0 = p.calculate(az, el, gain=gain, diffuse=diffuse)
    p.close()
    assert np.array_equal(d[plain], d0[plain]) and np.array_equal(f[plain], f0[plain])
    assert np.array_equal(dp, d[perm]) and np.array_equal(fp, f[perm])
    assert np.array_equal(da, d0) and np.array_equal(fa, f0)
    assert np.array_equal(dz, d0) and np.array_equal(fz, f0)
    assert np.array_equal(dq[plain], dq0[plain]) and np.array_equal(fq[plain], fq0[plain])
    assert not np.array_equal(dq[~plain], dq0[~plain])


def test_invariants_without_the_model():
    from libear_amd import capi
    layout = "9+10+3"
    names = LAYOUTS[layout]
    rng = np.random.default_rng(9)
    n = 800
    az, el, dist, width, height, depth, _, _ = scene(rng, n)
    md, _ = metadata(rng, layout, n)
    # every combination of the three: each on for half of the objects, independently
    combo = rng.integers(0, 8, n)
    md["channel_lock"] = (combo & 1).astype(np.uint8)
    md["divergence"] = np.where(combo & 2, np.maximum(md["divergence"], 0.05), 0.0)
    md["excluded"] = np.where(combo & 4, rng.integers(1, 1 << len(names), n), 0).astype(np.uint32)
    assert all(np.count_nonzero(combo == c) > n // 16 for c in range(8))
    p = capi.Panner(ctx(), layout)
    # unit norm for every combination
    d, f = p.calculate_objects(az, el, dist, None, None, width, height, depth, **md)
    assert np.max(np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0)) <= 1e-5
    assert not f.any()
    # v = 1: the power mean of the two side positions rendered alone
    r = rng.uniform(0.0, 90.0, n)
    side = [np.empty((n, 3)), np.empty((n, 3))]
    for i in range(n):
        pts, _ = om.Model.diverge(om.cart(az[i], el[i], dist[i]), 1.0, r[i])
        side[0][i], side[1][i] = pts[1], pts[2]
    alone = []
    for s in side:
        saz = -np.degrees(np.arctan2(s[:, 0], s[:, 1]))
        sel = np.degrees(np.arctan2(s[:, 2], np.hypot(s[:, 0], s[:, 1])))
        alone.append(p.calculate(saz, sel, np.linalg.norm(s, axis=1), None, None, width, height, depth)[0].astype(np.float64))
    d, _ = p.calculate_objects(az, el, dist, None, None, width, height, depth, divergence=1.0, azimuth_range=r)
    assert np.max(rel(d, np.sqrt((alone[0] ** 2 + alone[1] ** 2) / 2.0))) <= TOL
    # a locked object without extent is one loudspeaker at 1
    d, _ = p.calculate_objects(az, el, dist, channel_lock=1)
    assert np.all(np.sort(d, axis=1)[:, -1] >= 1.0 - 1e-6) and np.all(np.sort(np.abs(d), axis=1)[:, -2] <= 1e-6)
    assert not d[:, [i for i, nm in enumerate(names) if nm.startswith("LFE")]].any()
    # the host form refuses a mask bit beyond the layout and names the object
    with pytest.raises(capi.InvalidArgument, match=r"excluded\[1\] has a bit set beyond the layout's 24 channels"):
        p.calculate_objects([0.0, 1.0], [0.0, 0.0], excluded=np.array([0, 1 << 24], np.uint32))
    p.close()


def test_device_form_equals_the_host_form():
    import torch
    from libear_amd import capi
    layout = "4+5+1"
    rng = np.random.default_rng(21)
    n = 3000
    az, el, dist, width, height, depth, gain, diffuse = scene(rng, n)
    md, _ = metadata(rng, layout, n)
    p = capi.Panner(ctx(), layout)
    d, f = p.calculate_objects(az, el, dist, gain, diffuse, width, height, depth, **md)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(
        az=az, el=el, dist=dist, gain=gain, diffuse=diffuse, width=width, height=height, depth=depth, **md).items()}
    dd = torch.empty((n, p.n_out), dtype=torch.float32, device="cuda")
    df = torch.empty_like(dd)
    torch.cuda.synchronize()
    p.calculate_objects_device(n, dev["az"].data_ptr(), dev["el"].data_ptr(), dev["dist"].data_ptr(), dev["gain"].data_ptr(),
                               dev["diffuse"].data_ptr(), dd.data_ptr(), df.data_ptr(), dev["width"].data_ptr(),
                               dev["height"].data_ptr(), dev["depth"].data_ptr(), dev["channel_lock"].data_ptr(),
                               dev["lock_max_distance"].data_ptr(), dev["divergence"].data_ptr(), dev["azimuth_range"].data_ptr(),
                               dev["excluded"].data_ptr())
    assert p.missed() == 0
    assert np.array_equal(dd.cpu().numpy(), d) and np.array_equal(df.cpu().numpy(), f)
    # values the device form cannot refuse: a divergence is clamped (NaN: 0), a NaN maxDistance locks to nothing
    k = 64
    odd = torch.tensor([-0.5, 1.5, float("nan"), 0.5] * (k // 4), dtype=torch.float64, device="cuda")
    nan = torch.full((k,), float("nan"), dtype=torch.float64, device="cuda")
    ones = torch.ones(k, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p.calculate_objects_device(k, dev["az"].data_ptr(), dev["el"].data_ptr(), None, None, None, dd.data_ptr(), df.data_ptr(),
                               channel_lock=ones.data_ptr(), lock_max_distance=nan.data_ptr(), divergence=odd.data_ptr())
    assert p.missed() == 0
    got = dd[:k].cpu().numpy()
    want, _ = p.calculate_objects(az[:k], el[:k], channel_lock=1, lock_max_distance=0.0,
                                  divergence=np.array([0.0, 1.0, 0.0, 0.5] * (k // 4)))
    p.close()
    assert np.array_equal(got, want)
