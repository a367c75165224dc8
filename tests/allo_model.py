"""A float64 numpy model of the allocentric (Cartesian) point-source panner, written from the specification in include/earhip.h
group T (the loudspeaker table, the snapping, bracket() and the z / y / x walk), not from the C++ core.  Plain loops over
positions: the tests use a few thousand of them."""
import math

import numpy as np

from layouts import LAYOUTS

S = math.sqrt(2.0) - 1.0
HALF_PI = math.pi / 2.0


def _pm(name, x, y, z):
    """a +- row of the table: the + name (left, x negative) first"""
    return {name.replace("*", "+"): (-x, y, z), name.replace("*", "-"): (x, y, z)}


TABLE = {"M+000": (0.0, 1.0, 0.0), "M+180": (0.0, -1.0, 0.0), "U+000": (0.0, 1.0, 1.0), "U+180": (0.0, -1.0, 1.0),
         "UH+180": (0.0, -1.0, 1.0), "T+000": (0.0, 0.0, 1.0), "B+000": (0.0, 1.0, -1.0)}
for _row in (("M*030", 1.0, 1.0, 0.0), ("M*SC", S, 1.0, 0.0), ("M*060", 1.0, S, 0.0), ("M*090", 1.0, 0.0, 0.0),
             ("M*110", 1.0, -1.0, 0.0), ("M*135", 1.0, -1.0, 0.0), ("U*030", 1.0, 1.0, 1.0), ("U*045", 1.0, 1.0, 1.0),
             ("U*090", 1.0, 0.0, 1.0), ("U*110", 1.0, -1.0, 1.0), ("U*135", 1.0, -1.0, 1.0), ("B*045", 1.0, 1.0, -1.0)):
    TABLE.update(_pm(*_row))
EXCEPTIONS = {("9+10+3", "M+030"): (-S, 1.0, 0.0), ("9+10+3", "M-030"): (S, 1.0, 0.0)}


def is_lfe(name):
    return name.startswith("LFE")


def table_positions(layout):
    """float64 [n_channels][3] of a BS.2051 layout, LFE rows NaN"""
    out = np.full((len(LAYOUTS[layout]), 3), np.nan)
    for c, name in enumerate(LAYOUTS[layout]):
        if not is_lfe(name):
            out[c] = EXCEPTIONS.get((layout, name), TABLE[name])
    return out


def snap(positions, lfe):
    """per axis: the loudspeakers' coordinates sorted ascending and walked; a value within 1e-6 of the first value of the
    current group takes that first value.  -> a copy, LFE rows NaN"""
    p = np.array(positions, np.float64)
    real = [c for c in range(len(p)) if not lfe[c]]
    p[[c for c in range(len(p)) if lfe[c]]] = np.nan
    for k in range(3):
        first = None
        for c in sorted(real, key=lambda c: p[c, k]):
            if first is not None and p[c, k] - first <= 1e-6:
                p[c, k] = first
            else:
                first = p[c, k]
    return p


class Model:
    def __init__(self, layout=None, positions=None, lfe=None):
        """a BS.2051 layout's table, or positions [n][3] with the LFE flags"""
        if positions is None:
            positions, lfe = table_positions(layout), [is_lfe(n) for n in LAYOUTS[layout]]
        self.lfe = list(lfe)
        self.p = snap(positions, self.lfe)
        self.n = len(self.p)
        self.real = [c for c in range(self.n) if not self.lfe[c]]

    @staticmethod
    def bracket(values, v):
        """[(value, weight)] over a non-empty set of distinct doubles"""
        below = [p for p in values if p <= v]
        above = [p for p in values if p >= v]
        if not below:
            return [(min(above), 1.0)]
        if not above:
            return [(max(below), 1.0)]
        lo, hi = max(below), min(above)
        if lo == hi:
            return [(lo, 1.0)]
        f = (v - lo) / (hi - lo)
        return [(lo, math.cos(f * HALF_PI)), (hi, math.sin(f * HALF_PI))]

    def weights(self, x, y, z, excluded=0):
        """float64 [n_channels] of one position"""
        active = [c for c in self.real if not (int(excluded) >> c) & 1] or self.real
        w = np.zeros(self.n)
        p = self.p
        for Z, wz in self.bracket({p[c, 2] for c in active}, z):
            plane = [c for c in active if p[c, 2] == Z]
            for Y, wy in self.bracket({p[c, 1] for c in plane}, y):
                row = [c for c in plane if p[c, 1] == Y]
                for X, wx in self.bracket({p[c, 0] for c in row}, x):
                    (c,) = [c for c in row if p[c, 0] == X]
                    w[c] = (wz * wy) * wx
        return w

    def calculate64(self, x, y, z, gain=None, diffuse=None, excluded=None):
        """(direct, diffuse) float64 [n][n_channels], before the rounding to float32"""
        x = np.atleast_1d(np.asarray(x, np.float64))
        n = x.size
        y, z = (np.broadcast_to(np.asarray(v, np.float64), (n,)) for v in (y, z))
        g = np.ones(n) if gain is None else np.broadcast_to(np.asarray(gain, np.float64), (n,))
        d = np.zeros(n) if diffuse is None else np.broadcast_to(np.asarray(diffuse, np.float64), (n,))
        m = np.zeros(n, np.uint32) if excluded is None else np.broadcast_to(np.asarray(excluded, np.uint32), (n,))
        w = np.stack([self.weights(x[i], y[i], z[i], m[i]) for i in range(n)]) if n else np.zeros((0, self.n))
        return w * g[:, None] * np.sqrt(1.0 - d)[:, None], w * g[:, None] * np.sqrt(d)[:, None]

    def excluded_channels(self, zones):
        """zones: dicts of min_x .. max_z -> the mask of the loudspeakers inside at least one"""
        tol, mask = 1e-6, 0
        for zn in zones:
            for c in self.real:
                if all(zn["min_" + a] - tol < self.p[c, k] < zn["max_" + a] + tol for k, a in enumerate("xyz")):
                    mask |= 1 << c
        return mask


def spacing_bar(want64):
    """one float32 spacing at max(|want|, 2^-20): the bar of the host and device forms against float32(model)"""
    w = np.maximum(np.abs(np.asarray(want64, np.float64)), 2.0 ** -20).astype(np.float32)
    return np.spacing(w).astype(np.float64)


def within_one_spacing(got32, want64):
    """(ok, worst error / bar): got against float32(want64)"""
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    err = np.abs(got32.astype(np.float64) - want32.astype(np.float64))
    bar = spacing_bar(want64)
    return bool(np.all(err <= bar)), float(np.max(err / bar)) if err.size else 0.0


# positions every batch of the tests ends with: on loudspeakers, between them, the centre, outside the box, -0.0
SPECIAL = [(0.0, 1.0, 0.0), (-0.5, 1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 3.0), (0.0, 0.0, 0.5), (0.0, 0.0, 1.0), (-1.0, 1.0, 0.0),
           (0.5, -1.0, 1.0), (-0.0, -0.0, -0.0), (1.3, -1.3, -1.3), (-1.0, -1.0, -1.0), (S, 1.0, 0.0)]

# a 32-channel layout of the caller's own: 21 loudspeakers (two rings and a top) and 11 LFE channels in between
DOME32_NAME = "allo-dome32"


def dome32():
    """-> (channels for define_layout [(name, azimuth, elevation, is_lfe)], positions float64 [32][3]): the rings stand on
    the walls of the cube (the direction scaled until it meets one), the upper ring on the ceiling's height"""
    channels, pos = [], []
    ring = [("M", 30, 0.0, 0.0), ("U", 45, 35.0, 1.0)]
    k = 0
    for prefix, step, el, z in ring:
        for a in range(0, 360, step):
            a = a if a <= 180 else a - 360
            channels.append((f"{prefix}{'+' if a >= 0 else '-'}{abs(a):03d}", float(a), el, False))
            px, py = -math.sin(math.radians(a)), math.cos(math.radians(a))
            scale = max(abs(px), abs(py))
            pos.append((px / scale, py / scale, z))
            if len(channels) % 3 == 2 and k < 11:
                k += 1
                channels.append((f"LFE{k}", 45.0, -30.0, True))
                pos.append((np.nan, np.nan, np.nan))
    channels.append(("T+000", 0.0, 90.0, False))
    pos.append((0.0, 0.0, 1.0))
    while k < 11:
        k += 1
        channels.append((f"LFE{k}", 45.0, -30.0, True))
        pos.append((np.nan, np.nan, np.nan))
    assert len(channels) == 32
    return channels, np.array(pos, np.float64)
