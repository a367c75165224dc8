"""An independent float64 numpy model of include/earhip.h group R (screenRef scaling and screenEdgeLock, ITU-R BS.2127-0
sections 7.3.3 and 7.3.4): a screen's edges as the group comment writes them, the scale by np.interp over the two breakpoint
lists, the lock.  A screen is a dict: {"aspect", "az", "el", "dist", "width"} (polar) or {"aspect", "x", "y", "z", "width_x"}."""
import numpy as np

DEFAULT = dict(aspect=1.78, az=0.0, el=0.0, dist=1.0, width=58.0)
SCREEN_30 = dict(aspect=1.78, az=0.0, el=0.0, dist=1.0, width=30.0)
POLAR_15 = dict(aspect=1.5, az=-20.0, el=10.0, dist=2.0, width=40.0)
CART = dict(aspect=1.78, x=0.0, y=1.0, z=0.0, width_x=1.0)
# three more that keep their edges ordered: off-centre, high, narrow
OTHERS = (dict(aspect=2.39, az=35.0, el=-12.0, dist=3.0, width=70.0), dict(aspect=1.33, x=-0.4, y=0.8, z=0.3, width_x=0.9),
          dict(aspect=1.0, az=-60.0, el=25.0, dist=1.0, width=12.0))
ALL = (DEFAULT, SCREEN_30, POLAR_15, CART) + OTHERS


def cart(az, el, d):
    az, el = np.radians(az), np.radians(el)
    return np.array([np.sin(-az) * np.cos(el) * d, np.cos(-az) * np.cos(el) * d, np.sin(el) * d])


def azim(v):
    return -np.degrees(np.arctan2(v[0], v[1]))


def elev(v):
    return np.degrees(np.arctan2(v[2], np.hypot(v[0], v[1])))


def edges(s):
    """(left, right, bottom, top) in degrees"""
    if "x" in s:
        c = np.array([s["x"], s["y"], s["z"]])
        w = s["width_x"] / 2.0
        h = w / s["aspect"]
        xv, zv = np.array([w, 0.0, 0.0]), np.array([0.0, 0.0, h])
    else:
        c = cart(s["az"], s["el"], s["dist"])
        w = s["dist"] * np.tan(np.radians(s["width"] / 2.0))
        h = w / s["aspect"]
        xv, zv = w * cart(s["az"] - 90.0, 0.0, 1.0), h * cart(s["az"], s["el"] + 90.0, 1.0)
    return float(azim(c - xv)), float(azim(c + xv)), float(elev(c - zv)), float(elev(c + zv))


def apply(az, el, reproduction, reference=None, screen_ref=None, lock_h=None, lock_v=None):
    """arrays [n] -> (azimuth, elevation); reproduction None: the identity"""
    az, el = np.array(az, np.float64), np.array(el, np.float64)
    n = az.size
    if reproduction is None:
        return az, el
    ref = np.ones(n, bool) if screen_ref is None else np.asarray(screen_ref) != 0
    lh = np.zeros(n, int) if lock_h is None else np.asarray(lock_h)
    lv = np.zeros(n, int) if lock_v is None else np.asarray(lock_v)
    rl, rr, rb, rt = edges(DEFAULT if reference is None else reference)
    pl, pr, pb, pt = edges(reproduction)
    a = np.fmod(az, 360.0)
    a = np.where(a > 180.0, a - 360.0, np.where(a < -180.0, a + 360.0, a))
    with np.errstate(invalid="ignore"):
        az = np.where(ref, np.interp(a, [-180.0, rr, rl, 180.0], [-180.0, pr, pl, 180.0]), az)
        el = np.where(ref, np.interp(el, [-90.0, rb, rt, 90.0], [-90.0, pb, pt, 90.0]), el)
    az = np.where(lh == 1, pl, np.where(lh == 2, pr, az))
    el = np.where(lv == 1, pb, np.where(lv == 2, pt, el))
    return az, el


def mixed_batch(n, seed, invalid=False):
    """n seeded elements that mix flags and locks, the seam, the poles, zero and azimuths beyond a turn; invalid: every 37th
    flagged element is one the stage refuses.  -> az, el, screen_ref, lock_h, lock_v (float64, float64, uint8 x 3), bad (bool)"""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-180.0, 180.0, n)
    el = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n)))
    special_az = np.array([180.0, -180.0, 0.0, -0.0, 29.0, -29.0, 389.0, -540.0, 720.0, 1e9 + 0.5, 179.99999999999997])
    special_el = np.array([90.0, -90.0, 0.0, -0.0, 17.29708889245067, -17.29708889245067, 45.0])
    pick = rng.uniform(0, 1, n) < 0.15
    az[pick] = rng.choice(special_az, int(pick.sum()))
    pick = rng.uniform(0, 1, n) < 0.15
    el[pick] = rng.choice(special_el, int(pick.sum()))
    ref = (rng.uniform(0, 1, n) < 0.6).astype(np.uint8)
    lh = rng.choice([0, 0, 0, 1, 2], n).astype(np.uint8)
    lv = rng.choice([0, 0, 0, 1, 2], n).astype(np.uint8)
    untouched = (ref == 0) & (lh == 0) & (lv == 0)
    # what an untouched element holds is nobody's business
    nan = untouched & (rng.uniform(0, 1, n) < 0.2)
    az[nan] = np.nan
    el[untouched & (rng.uniform(0, 1, n) < 0.2)] = 1234.5
    bad = np.zeros(n, bool)
    if invalid:
        flagged = np.flatnonzero(~untouched)[::37]
        bad[flagged] = True
        for k, i in enumerate(flagged):
            kind = k % 6
            if kind == 0:
                az[i] = np.nan
            elif kind == 1:
                az[i] = np.inf
            elif kind == 2:
                az[i] = 2.0 ** 41
            elif kind == 3:
                el[i] = 90.00000000000001
            elif kind == 4:
                el[i] = -np.inf
            else:
                lh[i] = 3
    return az, el, ref, lh, lv, bad
