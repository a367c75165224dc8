"""Loudspeaker layouts of the caller's own on the device (earhip_layout_define, include/earhip.h group H): copies of the
nine tabled BS.2051 layouts — whose facets now come from the hull — against the layouts themselves through every
producer; the three new layouts of tests/custom_layout_model.py against that model (held to the oracle's panner by
tests/test_custom_layout_cpu.py); and the panner's self-check (earhip_panner_self_check, one launch of k_pan_self_check).
Every case pans at most 5,400 positions."""
import numpy as np
import pytest

import _oracle
import custom_layout_model as model
from _hip import ctx
from layouts import LAYOUTS

pytestmark = pytest.mark.gpu

TABLED = [name for name in sorted(LAYOUTS) if name != "0+2+0"]
STEP = 2.0 ** -23  # one float32 step at 1.0, two steps just below it


@pytest.fixture(scope="module")
def design():
    """the 5,200 directions of the t-design (computed once, shared, never written to)"""
    xyz = _oracle.tdesign_points()
    xyz.setflags(write=False)
    return xyz


def directions(design, channels, positions=None):
    """-> (azimuth, elevation) of the t-design's directions plus every loudspeaker's (LFE included)"""
    az, el = model.polar(design)
    saz = [c[1] for c in channels] if positions is None else positions[0]
    sel = [c[2] for c in channels] if positions is None else positions[1]
    return np.r_[az, saz], np.r_[el, sel]


def device_gains(p, az, el, objects=False, **extra):
    """the _device forms on arrays made here -> (direct, diffuse) float32 [n][n_out]"""
    import torch
    dtype = {"channel_lock": np.uint8, "excluded": np.uint32}
    dev = {k: torch.from_numpy(np.array(np.broadcast_to(np.asarray(v, dtype.get(k, np.float64)), (len(az),)))).cuda()
           for k, v in dict(az=az, el=el, **extra).items()}
    d = torch.full((len(az), p.n_out), float("nan"), dtype=torch.float32, device="cuda")
    f = torch.full_like(d, float("nan"))
    ptr = {k: v.data_ptr() for k, v in dev.items()}
    torch.cuda.synchronize()
    call = p.calculate_objects_device if objects else p.calculate_device
    call(len(az), ptr.pop("az"), ptr.pop("el"), ptr.pop("dist", None), ptr.pop("gain", None), ptr.pop("diffuse", None),
         d.data_ptr(), f.data_ptr(), **ptr)
    assert p.missed() == 0  # (synchronises)
    return d.cpu().numpy(), f.cpu().numpy()


def relative(a, b):
    """per row: |a - b| over the smaller of the two norms"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    den = np.maximum(np.minimum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)), 1e-30)
    return np.linalg.norm(a - b, axis=1) / den


def define_copy(name):
    from libear_amd import capi
    capi.define_layout("copy:" + name, [c + r for c, r in zip(capi.layout_channels(name), capi.layout_channel_ranges(name))])
    return "copy:" + name


@pytest.mark.parametrize("name", TABLED)
def test_copy_of_a_bs2051_layout_pans_like_the_layout(name, design):
    """Only the order of the regions differs between a BS.2051 layout (its table) and its copy (the hull).  A direction
    within 1e-11 of an edge two regions share may be taken by the other one, whose gains there are the same up to double
    rounding: the float32 outputs differ by at most 2^-23 (one step at 1.0, two below it).  More would be a discontinuity
    between regions."""
    from libear_amd import capi
    copy = define_copy(name)
    channels = capi.layout_channels(name)
    az, el = directions(design, channels)
    rng = np.random.default_rng(sum(map(ord, name)))
    diffuse = rng.choice([0.0, 0.3, 1.0], len(az))
    a, b = capi.Panner(ctx(), name), capi.Panner(ctx(), copy)
    try:
        assert a.n_out == b.n_out == len(channels)
        (da, fa), (db, fb) = (device_gains(p, az, el, diffuse=diffuse) for p in (a, b))
        worst = max(np.abs(da - db).max(), np.abs(fa - fb).max())
        print(f"{name}: largest difference between the layout and its copy {worst:.3e} ({worst / STEP:.2f} steps of 2^-23), "
              f"{int((da != db).any(axis=1).sum())} of {len(az)} rows differ")
        assert worst <= STEP
        # the extent panner: float sums over a grid the point source panner filled, 1e-5 of a vector's norm between cores
        for depth in (0.0, 0.3):
            (da, fa), (db, fb) = (device_gains(p, az, el, diffuse=diffuse, width=40.0, height=20.0, depth=depth) for p in (a, b))
            worst = max(relative(da[diffuse < 1], db[diffuse < 1]).max(), relative(fa[diffuse > 0], fb[diffuse > 0]).max())
            print(f"{name}: extent 40 x 20, depth {depth}: {worst:.3e} of the norm")
            assert worst <= 1e-5
        # channel lock, divergence and zone exclusion: a third of the positions each
        n = len(az)
        kind = np.arange(n) % 3
        full = [i for i, c in enumerate(channels) if not c[3]]
        zone = sum(1 << i for i in full[::3])
        md = dict(channel_lock=(kind == 0).astype(np.uint8), lock_max_distance=np.where(kind == 0, 0.8, np.inf),
                  divergence=np.where(kind == 1, 0.4, 0.0), azimuth_range=np.full(n, 30.0),
                  excluded=np.where(kind == 2, zone, 0).astype(np.uint32))
        (da, fa), (db, fb) = (device_gains(p, az, el, objects=True, diffuse=diffuse, **md) for p in (a, b))
        worst = max(relative(da[diffuse < 1], db[diffuse < 1]).max(), relative(fa[diffuse > 0], fb[diffuse > 0]).max())
        print(f"{name}: lock / divergence / zone: {worst:.3e} of the norm")
        assert worst <= 1e-5
    finally:
        a.close()
        b.close()
    # the HOA decoder of order 3
    orders = [n for n in range(4) for _ in range(2 * n + 1)]
    degrees = [m for n in range(4) for m in range(-n, n + 1)]
    Da, Db = (capi.hoa_decode_matrix(ctx(), which, orders, degrees, "SN3D") for which in (name, copy))
    print(f"{name}: HOA order 3: {np.abs(Da - Db).max() / np.abs(Da).max():.3e} of the largest entry")
    assert np.abs(Da - Db).max() <= 1e-6 * np.abs(Da).max()
    # DirectSpeakers: a labelled channel is that channel
    md = [{"speakerLabels": [f"urn:itu:bs:2051:0:speaker:{c[0]}"], **({"lowPass": 120.0} if c[3] else {})} for c in channels]
    ga, gb = (capi.DirectSpeakers(ctx(), which) for which in (name, copy))
    try:
        assert np.array_equal(ga.calculate(md)[0], gb.calculate(md)[0]) and np.array_equal(ga.calculate(md)[0], np.eye(len(channels)))
    finally:
        ga.close()
        gb.close()


def moved_positions(channels, seed):
    """every loudspeaker up to 3 degrees off its nominal position (one straight overhead stays where it is)"""
    rng = np.random.default_rng(seed)
    az = np.array([c[1] for c in channels]) + rng.uniform(-3, 3, len(channels))
    el = np.array([c[2] for c in channels]) + rng.uniform(-3, 3, len(channels))
    pole = np.array([abs(c[2]) == 90.0 for c in channels])
    az[pole], el[pole] = [c[1] for c, p in zip(channels, pole) if p], [c[2] for c, p in zip(channels, pole) if p]
    return az, np.clip(el, -90.0, 90.0)


@pytest.mark.parametrize("moved", [False, True], ids=["nominal", "moved"])
@pytest.mark.parametrize("name", sorted(model.CUSTOM))
def test_new_layout_against_the_model(name, moved, design):
    from libear_amd import capi
    channels = model.CUSTOM[name][0]
    capi.define_layout(name, channels)
    positions = moved_positions(channels, len(name)) if moved else None
    az, el = directions(design, channels, positions)
    lfe = np.array([c[3] for c in channels])
    az, el = np.r_[az[:5200], az[5200:][~lfe]], np.r_[el[:5200], el[5200:][~lfe]]  # (an LFE's position is no loudspeaker direction)
    reference = model.Panner(channels, positions)
    want, want_missed = reference.pan(model.cart(az, el))
    assert not want_missed.any()
    p = capi.Panner(ctx(), name, positions)
    try:
        got, diffuse = device_gains(p, az, el)
    finally:
        p.close()
    assert got.shape == (len(az), len(channels)) and not diffuse.any()
    worst = np.abs(got - reference.full(want, len(channels))).max()
    print(f"{name} ({'moved' if moved else 'nominal'}): largest difference between the device and the model {worst:.3e}")
    assert worst <= 1e-6
    assert not got[:, lfe].any()
    own = got[5200:][:, ~lfe]
    assert np.abs(own - np.eye(own.shape[0])).max() <= 1e-6
    assert np.abs((got.astype(np.float64) ** 2).sum(axis=1) - 1.0).max() <= 1e-6
    if not moved:
        names = [c[0] for c in channels]
        swap = [names.index(nm.replace("+", "-") if "+" in nm else nm.replace("-", "+"))
                if not nm.endswith(("000", "180")) and not nm.startswith("LFE") else i for i, nm in enumerate(names)]
        p = capi.Panner(ctx(), name)
        try:
            mirrored, _ = device_gains(p, -az, el)
        finally:
            p.close()
        assert np.abs(mirrored[:, swap] - got).max() <= 1e-6


def report_fields(r):
    return {k: getattr(r, k) for k, _ in r._fields_}


@pytest.mark.parametrize("name", TABLED + sorted(model.CUSTOM))
def test_self_check(name):
    import ctypes
    from libear_amd import capi
    if name in model.CUSTOM:
        capi.define_layout(name, model.CUSTOM[name][0])
    channels = capi.layout_channels(name)
    p = capi.Panner(ctx(), name)
    try:
        r, again = p.self_check(), p.self_check()
    finally:
        p.close()
    print(name, report_fields(r))
    assert ctypes.string_at(ctypes.addressof(r), ctypes.sizeof(r)) == ctypes.string_at(ctypes.addressof(again), ctypes.sizeof(again))
    assert r.n_directions == 5200 + sum(1 for c in channels if not c[3]) and r.missed == 0
    assert r.max_power_error <= 1e-12 and 1.0 - 1e-9 <= r.min_own_gain <= 1.0 + 1e-9
    assert (r.n_regions, r.n_triplets, r.n_quads, r.n_ngons, r.largest_ngon) == model.Panner(channels).counts()
    if name in model.CUSTOM:
        _, n_facets, n_quads, n_triangles, rings, _ = model.CUSTOM[name]
        ring_facets = sum(rings)  # (every loudspeaker around a virtual one closes one facet with it and its neighbour)
        assert (r.n_quads, r.n_triplets, r.n_ngons, r.largest_ngon) == (n_quads, n_triangles - ring_facets, len(rings), max(rings))
        assert r.n_regions == n_facets - ring_facets + len(rings)


def test_self_check_of_the_stereo_downmix():
    """0+2+0 pans on 0+5+0 and mixes down: -3 dB at the back by design, so the power error reaches 0.5 there"""
    from libear_amd import capi
    p = capi.Panner(ctx(), "0+2+0")
    try:
        r, again = p.self_check(), p.self_check()
    finally:
        p.close()
    print("0+2+0", report_fields(r))
    assert report_fields(r) == report_fields(again)
    assert r.n_directions == 5202 and r.missed == 0 and 0.4 < r.max_power_error <= 0.5 + 1e-12
    assert (r.n_regions, r.n_ngons) == (12, 2)  # the regions of 0+5+0


def test_self_check_at_real_positions_and_after_a_call():
    """the loudspeakers' REAL directions are what the self-check pans, and it leaves the count of the last call alone"""
    from libear_amd import capi
    channels = model.CUSTOM["dome"][0]
    capi.define_layout("dome", channels)
    p = capi.Panner(ctx(), "dome", moved_positions(channels, 3))
    try:
        p.calculate([10.0, 20.0], [5.0, 50.0])
        r = p.self_check()
        assert r.missed == 0 and r.max_power_error <= 1e-12 and r.min_own_gain >= 1.0 - 1e-9 and p.missed() == 0
    finally:
        p.close()
