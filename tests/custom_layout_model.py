"""A float64 numpy restatement of the point source panner of ANY loudspeaker layout, for the layouts the oracle has no
table for (earhip_layout_define): the augmented loudspeaker set (extra loudspeakers above / below the mid layer, the
virtual ones), the brute-force convex hull with its merge of coplanar triangles, the three region handlers (triplet,
quad, virtual n-gon), the downmix of the extra loudspeakers and the final normalisation.  tests/test_custom_layout_cpu.py
first holds it to the oracle's panner on 4+5+0 and 9+10+3; only then is it the reference for the defined layouts.

Also the three layouts the tests define: 2+7+0, 6+9+0 and a dome, as lists of (name, azimuth, elevation, is_lfe)."""
import itertools

import numpy as np


def _pm(prefix, azimuths, el):
    out = []
    for a in azimuths:
        out += [(f"{prefix}+{a:03d}", float(a), float(el), False), (f"{prefix}-{a:03d}", float(-a), float(el), False)]
    return out


LFE1 = ("LFE1", 45.0, -30.0, True)
LAYOUT_2_7_0 = _pm("M", [30], 0) + [("M+000", 0.0, 0.0, False), LFE1] + _pm("M", [90, 135], 0) + _pm("U", [90], 30)
LAYOUT_6_9_0 = (_pm("M", [30], 0) + [("M+000", 0.0, 0.0, False), LFE1] + _pm("M", [60, 90, 135], 0) +
                _pm("U", [45, 90, 135], 30))


def _ring(prefix, step, el):
    out = []
    for a in range(0, 360, step):
        a = a if a <= 180 else a - 360
        out.append((f"{prefix}{'+' if a >= 0 else '-'}{abs(a):03d}", float(a), float(el), False))
    return out


LAYOUT_DOME = _ring("M", 30, 0) + _ring("U", 45, 35) + [("T+000", 0.0, 90.0, False)]

# name -> (channels, facets, quads, triangles, rings around the virtual loudspeakers (below, above), simplices)
CUSTOM = {
    "2+7+0": (LAYOUT_2_7_0, 26, 10, 16, [7, 7], 36),
    "6+9+0": (LAYOUT_6_9_0, 36, 12, 24, [9, 6], 48),
    "dome": (LAYOUT_DOME, 52, 12, 40, [12], 64),
}


def cart(az, el):
    """libear's polar convention (src/common/geom.cpp:82-87)"""
    az, el = np.radians(-np.asarray(az, np.float64)), np.radians(np.asarray(el, np.float64))
    return np.stack([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el) + 0 * az], axis=-1)


def polar(xyz):
    """unit vectors [n][3] -> (azimuth, elevation) in degrees"""
    xyz = np.asarray(xyz, np.float64)
    return -np.degrees(np.arctan2(xyz[:, 0], xyz[:, 1])), np.degrees(np.arctan2(xyz[:, 2], np.hypot(xyz[:, 0], xyz[:, 1])))


def augment(channels, positions=None):
    """-> (xyz [V][3], mix_to [V] over the loudspeakers that are not LFE (-1: virtual), indices of the virtual vertices).
    positions: (azimuths, elevations) of every channel, the real positions (None: nominal); the layer logic follows the
    nominal ones (point_source_panner.cpp:256-349, :431-476)"""
    keep = [i for i, c in enumerate(channels) if not c[3]]
    nom = [(channels[i][1], channels[i][2]) for i in keep]
    real = nom if positions is None else [(float(positions[0][i]), float(positions[1][i])) for i in keep]
    pts, mix_to = [cart(a, e) for a, e in real], list(range(len(keep)))
    for layer_nominal, lo, hi in ((-30.0, -70.0, -10.0), (30.0, 10.0, 70.0)):
        inside = [k for k, (_, e) in enumerate(nom) if lo <= e <= hi]
        az_limit = max(abs(nom[k][0]) for k in inside) + 40.0 if inside else 0.0
        layer_el = sum(real[k][1] for k in inside) / len(inside) if inside else layer_nominal
        for k in range(len(keep)):
            if -10 <= nom[k][1] <= 10 and abs(real[k][0]) >= az_limit - 1e-5:
                pts.append(cart(real[k][0], layer_el))
                mix_to.append(k)
    virt = [len(pts)]
    pts.append(np.array([0.0, 0.0, -1.0]))
    mix_to.append(-1)
    if not any(channels[i][0] in ("T+000", "UH+180") for i in keep):
        virt.append(len(pts))
        pts.append(np.array([0.0, 0.0, 1.0]))
        mix_to.append(-1)
    return np.array(pts), mix_to, virt


def convex_hull(pts, tol=1e-5):
    """facets as ascending tuples of vertex indices (libear's algorithm: src/common/convex_hull.cpp)"""
    pts = np.asarray(pts, np.float64)
    mean = pts.mean(axis=0)
    tris, normals = [], []
    for i, j, k in itertools.combinations(range(len(pts)), 3):
        nrm = np.cross(pts[j] - pts[i], pts[k] - pts[i])
        if not nrm @ nrm > tol:
            raise ValueError("collinear points in convex hull")
        nrm = nrm / np.sqrt(nrm @ nrm)
        side = nrm @ (mean - pts[i])
        if abs(side) < tol:
            continue
        d = (pts - pts[i]) @ nrm
        if (d > -tol).all() if side > 0 else (d < tol).all():
            tris.append((i, j, k))
            normals.append(nrm)
    facets, facet_normals = [], []
    for tri, nrm in zip(tris, normals):
        for f, fn in zip(facets, facet_normals):
            x = np.cross(fn, nrm)
            if abs((pts[tri[0]] - pts[min(f)]) @ fn) < tol and x @ x < tol:
                f.update(tri)
                break
        else:
            facets.append(set(tri))
            facet_normals.append(nrm)
    return [tuple(sorted(f)) for f in facets]


def vertex_order(pos):
    """order of the vertices around their centre (src/common/geom.cpp:37-70)"""
    r = pos - pos.mean(axis=0)
    a = r[0]
    b = r[1 + int(np.argmin(np.abs(r[1:] @ a)))]
    return list(np.argsort(np.arctan2(r @ a, r @ b), kind="stable"))


def _triplet(rows, p):
    """-> (taken [n], gains [n][3]) (point_source_panner.cpp:43-51)"""
    pv = p @ np.linalg.inv(rows)
    taken = (pv >= -1e-11).all(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        pv = np.clip(pv / np.linalg.norm(pv, axis=1, keepdims=True), 0.0, 1.0)
    return taken, pv


def _poly(q):
    a, b, c, d = q
    return np.array([np.cross(b - a, c - d), np.cross(a, c - d) + np.cross(b - a, d), np.cross(a, d)])


def _quad_pan(poly, p):
    """first real root in (-1e-10, 1 + 1e-10) of (poly . p), clamped; NaN: none (:157-190)"""
    a, b, c = (p @ poly[0], p @ poly[1], p @ poly[2])
    eps = 1e-10
    r = np.full((2, len(p)), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        det = b * b - 4.0 * a * c
        zero_c, lin = np.abs(c) < eps, np.abs(a) < eps
        two, one = det > eps, (det > -eps) & ~(det > eps)
        quad = ~zero_c & ~lin
        r[0] = np.where(zero_c, 0.0, np.where(lin, -c / b, np.where(two, (-b + np.sqrt(np.abs(det))) / (2.0 * a),
                                                                  np.where(one, -b / (2.0 * a), np.nan))))
        r[1] = np.where(quad & two, (-b - np.sqrt(np.abs(det))) / (2.0 * a), np.nan)
        ok = (-eps < r) & (r < 1.0 + eps)
    return np.clip(np.where(ok[0], r[0], np.where(ok[1], r[1], np.nan)), 0.0, 1.0)


class Panner:
    """the point source panner of a layout: channels as (name, azimuth, elevation, is_lfe) with NOMINAL positions,
    positions = (azimuths, elevations) of every channel where the loudspeakers really stand (None: nominal); facets: a
    facet list to use in its order instead of the model's own hull (regions that share an edge both accept a direction
    within 1e-11 of it, so the order decides which one answers there)"""

    def __init__(self, channels, positions=None, facets=None):
        self.n_real = sum(1 for c in channels if not c[3])
        self.full_index = [i for i, c in enumerate(channels) if not c[3]]
        nominal, _, _ = augment(channels)
        self.facets = convex_hull(nominal) if facets is None else [tuple(f) for f in facets]
        verts, mix_to, virt = augment(channels, positions)
        self.verts, self.mix_to, self.virt = verts, mix_to, virt
        self.regions = []  # (kind, outputs, data), the n-gons first (:497-527), then the other facets in hull order
        for vv in virt:
            ring = sorted({v for f in self.facets if vv in f for v in f} - {vv})
            assert len(ring) >= 3 and not set(ring) & set(virt)
            pos = verts[ring]
            order = vertex_order(pos)
            tris = [(order[t], order[(t + 1) % len(ring)]) for t in range(len(ring))]
            self.regions.append(("ngon", [mix_to[v] for v in ring], (pos, tris, verts[vv])))
        for f in self.facets:
            if set(f) & set(virt):
                continue
            assert len(f) in (3, 4), f
            pos = verts[list(f)]
            self.regions.append(("triplet" if len(f) == 3 else "quad", [mix_to[v] for v in f], pos))

    def counts(self):
        kinds = [r[0] for r in self.regions]
        ngons = [len(r[1]) for r in self.regions if r[0] == "ngon"]
        return len(kinds), kinds.count("triplet"), kinds.count("quad"), len(ngons), max(ngons)

    def _region(self, kind, data, p):
        if kind == "triplet":
            return _triplet(data, p)
        if kind == "ngon":
            pos, tris, centre = data
            n = len(pos)
            taken, g = np.zeros(len(p), bool), np.zeros((len(p), n))
            for a, b in tris:
                t, pv = _triplet(np.array([pos[a], pos[b], centre]), p)
                new = t & ~taken
                row = np.repeat(pv[new][:, 2:3] / np.sqrt(n), n, axis=1)  # the centre's gain, equal power (:86-101)
                row[:, a] += pv[new][:, 0]
                row[:, b] += pv[new][:, 1]
                g[new] = row / np.linalg.norm(row, axis=1, keepdims=True)
                taken |= new
            return taken, g
        order = vertex_order(data)
        q = data[order]
        x, y = _quad_pan(_poly(q), p), _quad_pan(_poly(np.roll(q, -1, axis=0)), p)
        pvs = np.zeros((len(p), 4))
        pvs[:, order[0]], pvs[:, order[1]] = (1 - x) * (1 - y), x * (1 - y)
        pvs[:, order[2]], pvs[:, order[3]] = x * y, (1 - x) * y
        with np.errstate(invalid="ignore"):
            taken = ~np.isnan(x) & ~np.isnan(y) & (np.einsum("ij,ij->i", pvs @ data, p) > 0)
            pvs = pvs / np.linalg.norm(pvs, axis=1, keepdims=True)
        return taken, pvs

    def pan(self, xyz):
        """unit vectors [n][3] -> (gains [n][loudspeakers that are not LFE], missed [n] bool)"""
        p = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        out, done = np.zeros((len(p), self.n_real)), np.zeros(len(p), bool)
        for kind, outputs, data in self.regions:
            todo = np.flatnonzero(~done)
            if not len(todo):
                break
            taken, g = self._region(kind, data, p[todo])
            rows = todo[taken]
            for k, o in enumerate(outputs):
                out[rows, o] += g[taken, k]
            done[rows] = True
        with np.errstate(invalid="ignore"):
            out[done] /= np.linalg.norm(out[done], axis=1, keepdims=True)
        return out, ~done

    def full(self, pv, n_full):
        """gains over the loudspeakers that are not LFE -> float32 rows of the full layout, LFE columns zero"""
        out = np.zeros((len(pv), n_full), np.float32)
        out[:, self.full_index] = pv
        return out
