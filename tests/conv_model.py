"""An independent numpy float64 restatement of ITU-R BS.2127 section 10 as libear implements it
(src/conversion.cpp): polar <-> Cartesian conversion of Objects positions and extents, vectorised over arrays.
It is the checker of the conversion group (earhip group K).

Status per element, as the library reports it: 0 ok, 1 invalid argument (a polar azimuth that is infinite or
beyond +-2^40: libear's angle loops never return there), 2 internal error (no sector, or the sector position p
outside [-1e-6, 1 + 1e-6]).  Outputs of failed elements are NaN.
"""
import numpy as np

OK, INVALID, INTERNAL = 0, 1, 2
EL_TOP, EL_TOP_TILDE = 30.0, 45.0
MAX_AZIMUTH = 2.0 ** 40

# mapping points of the five sectors: polar azimuth and the Cartesian point (x, y) it maps to
POLAR_POINTS = np.array([0.0, -30.0, -110.0, 110.0, 30.0])
CART_POINTS = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]])
RAD = np.pi / 180.0
DEG = 180.0 / np.pi


def _turns(x, lo):
    """x moved by whole turns to [lo, lo + 360); fmod keeps the reduction exact for any finite x"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.fmod(x, 360.0)
        r = np.where(r - 360.0 >= lo, r - 360.0, r)
        r = np.where(r - 360.0 >= lo, r - 360.0, r)
        r = np.where(r < lo, r + 360.0, r)
        r = np.where(r < lo, r + 360.0, r)
    return r


def _inside(x, start, end):
    """x within [start, end] going anticlockwise (end reduced to (start, start + 360])"""
    end = _turns(end, start)
    if end <= start:
        end += 360.0
    return _turns(x, start) <= end


def _sectors():
    out = []
    for k in range(5):
        j = (k + 1) % 5
        a, b = CART_POINTS[k], CART_POINTS[j]
        inv = np.linalg.inv(np.array([a, b]))  # [x, y] = [g_l, g_r] @ [a; b]  =>  [g_l, g_r] = [x, y] @ inv
        out.append(dict(left=POLAR_POINTS[k], right=POLAR_POINTS[j], cart_left=-np.degrees(np.arctan2(a[0], a[1])),
                        cart_right=-np.degrees(np.arctan2(b[0], b[1])), a=a, b=b, inv=inv))
    return out


SECTORS = _sectors()


def _sign(x):
    return np.where(x < 0, -1.0, np.where(x > 0, 1.0, 0.0))


def _find(az, key_right, key_left):
    """index of the first sector containing az, -1 if none"""
    idx = np.full(np.shape(az), -1)
    for k in range(4, -1, -1):
        s = SECTORS[k]
        idx = np.where(_inside(az, s[key_right], s[key_left]), k, idx)
    return idx


def _lin_from_az(left, right, az):
    mid = (left + right) / 2.0
    rng = right - mid
    g = 0.5 + 0.5 * np.tan((az - mid) * RAD) / np.tan(rng * RAD)
    return np.arctan2(g, 1.0 - g) * (2.0 / np.pi)


def _az_from_lin(left, right, p):
    mid = (left + right) / 2.0
    rng = right - mid
    gl, gr = np.cos(p * (np.pi / 2.0)), np.sin(p * (np.pi / 2.0))
    g = gr / (gl + gr)
    return mid + np.degrees(np.arctan(2.0 * (g - 0.5) * np.tan(rng * RAD)))


def point_polar_to_cart(az, el, dist):
    az, el, dist = (np.asarray(v, np.float64) for v in np.broadcast_arrays(az, el, dist))
    with np.errstate(all="ignore"):
        high = np.abs(el) > EL_TOP
        el_t_high = EL_TOP_TILDE + (90.0 - EL_TOP_TILDE) * (np.abs(el) - EL_TOP) / (90.0 - EL_TOP)
        el_t_low = EL_TOP_TILDE * el / EL_TOP
        z = np.where(high, dist * _sign(el), np.tan(el_t_low * RAD) * dist)
        r_xy = np.where(high, dist * np.tan((90.0 - el_t_high) * RAD), dist)
        invalid = np.abs(az) > MAX_AZIMUTH
        az_ok = np.where(invalid, 0.0, az)
        k = _find(az_ok, "right", "left")
        x = np.full(az.shape, np.nan)
        y = np.full(az.shape, np.nan)
        p_all = np.full(az.shape, np.nan)
        for i, s in enumerate(SECTORS):
            m = k == i
            if not m.any():
                continue
            left = _turns(s["left"], s["right"])
            p = _lin_from_az(left, s["right"], _turns(az_ok[m], s["right"]))
            p_all[m] = p
            x[m] = r_xy[m] * (s["a"][0] + (s["b"][0] - s["a"][0]) * p)
            y[m] = r_xy[m] * (s["a"][1] + (s["b"][1] - s["a"][1]) * p)
        bad_p = (k >= 0) & ~((p_all >= -1e-6) & (p_all <= 1.0 + 1e-6))
    status = np.where(invalid, INVALID, np.where((k < 0) | bad_p, INTERNAL, OK))
    failed = status != OK
    return (np.where(failed, np.nan, x), np.where(failed, np.nan, y), np.where(failed, np.nan, z)), status


def point_cart_to_polar(x, y, z):
    x, y, z = (np.asarray(v, np.float64) for v in np.broadcast_arrays(x, y, z))
    eps = 1e-10
    with np.errstate(all="ignore"):
        az_c = -np.degrees(np.arctan2(x, y))
        k = _find(az_c, "cart_right", "cart_left")
        az = np.full(x.shape, np.nan)
        r_xy = np.full(x.shape, np.nan)
        for i, s in enumerate(SECTORS):
            m = k == i
            if not m.any():
                continue
            gl = x[m] * s["inv"][0, 0] + y[m] * s["inv"][1, 0]
            gr = x[m] * s["inv"][0, 1] + y[m] * s["inv"][1, 1]
            r = gl + gr
            left = _turns(s["left"], s["right"])
            az[m] = _turns(_az_from_lin(left, s["right"], gr / r), -180.0)
            r_xy[m] = r
        el_t = np.degrees(np.arctan(z / r_xy))
        high = np.abs(el_t) > EL_TOP_TILDE
        el = np.where(high, _sign(el_t) * (EL_TOP + (90.0 - EL_TOP) * (np.abs(el_t) - EL_TOP_TILDE) / (90.0 - EL_TOP_TILDE)),
                      EL_TOP * el_t / EL_TOP_TILDE)
        d = np.where(high, np.abs(z), r_xy)
    centre = (np.abs(x) < eps) & (np.abs(y) < eps)
    pole = centre & ~(np.abs(z) < eps)
    az = np.where(centre, 0.0, az)
    el = np.where(centre, np.where(pole, _sign(z) * 90.0, 0.0), el)
    d = np.where(centre, np.where(pole, np.abs(z), 0.0), d)
    status = np.where(~centre & (k < 0), INTERNAL, OK)
    failed = status != OK
    return (np.where(failed, np.nan, az), np.where(failed, np.nan, el), np.where(failed, np.nan, d)), status


def local_coordinate_system(az, el):
    """[..., 3 rows, 3] : the unit vectors at (az - 90, 0), (az, el), (az, el + 90)"""
    def cart(a, e):
        return np.stack([np.sin(-a * RAD) * np.cos(e * RAD), np.cos(-a * RAD) * np.cos(e * RAD), np.sin(e * RAD)], -1)
    return np.stack([cart(az - 90.0, np.zeros_like(el)), cart(az, el), cart(az, el + 90.0)], -2)


def _maxnan(a, b):
    """std::max(a, b): a unless a < b"""
    return np.where(a < b, b, a)


def whd2xyz(w, h, d):
    with np.errstate(all="ignore"):
        sx = np.where(w < 180.0, np.sin(w / 2.0 * RAD), 1.0)
        sz = np.where(h < 180.0, np.sin(h / 2.0 * RAD), 1.0)
        yw = (1.0 - np.cos(w / 2.0 * RAD)) / 2.0
        yh = (1.0 - np.cos(h / 2.0 * RAD)) / 2.0
    return sx, _maxnan(_maxnan(yw, yh), d), sz


def xyz2whd(sx, sy, sz):
    with np.errstate(all="ignore"):
        from_sy = 2.0 * np.degrees(np.arccos(1.0 - 2.0 * sy))
        from_sx = 2.0 * np.degrees(np.arcsin(sx))
        from_sz = 2.0 * np.degrees(np.arcsin(sz))
        w = from_sx + sx * _maxnan(from_sy - from_sx, 0.0)
        h = from_sz + sz * _maxnan(from_sy - from_sz, 0.0)
        _, ey, _ = whd2xyz(w, h, np.zeros_like(w))
        d = _maxnan(0.0, sy - ey)
    return w, h, d


def _norms(m):
    """column norms, the squares summed first to last"""
    return np.sqrt(m[..., 0, :] ** 2 + m[..., 1, :] ** 2 + m[..., 2, :] ** 2)


def extent_polar_to_cart(az, el, dist, w, h, d):
    (x, y, z), status = point_polar_to_cart(az, el, dist)
    az, el, w, h, d = (np.asarray(v, np.float64) for v in np.broadcast_arrays(az, el, w, h, d))
    failed = status != OK
    with np.errstate(all="ignore"):
        lcs = local_coordinate_system(np.where(failed, 0.0, az), el)
        front = np.stack(whd2xyz(w, h, d), -1)
        size = _norms(lcs * front[..., :, None])
    ext = (size[..., 0], size[..., 2], size[..., 1])
    return (x, y, z), tuple(np.where(failed, np.nan, e) for e in ext), status


def extent_cart_to_polar(x, y, z, w, h, d):
    (az, el, dist), status = point_cart_to_polar(x, y, z)
    w, h, d = (np.asarray(v, np.float64) for v in np.broadcast_arrays(w, h, d))
    with np.errstate(all="ignore"):
        lcs = local_coordinate_system(az, el)
        e = np.stack([w, d, h], -1)  # x, y, z sizes
        # the norm of each basis vector scaled per Cartesian axis
        s = np.sqrt((lcs[..., :, 0] * e[..., None, 0]) ** 2 + (lcs[..., :, 1] * e[..., None, 1]) ** 2
                    + (lcs[..., :, 2] * e[..., None, 2]) ** 2)
    ext = xyz2whd(s[..., 0], s[..., 1], s[..., 2])
    failed = status != OK
    return (az, el, dist), tuple(np.where(failed, np.nan, v) for v in ext), status
