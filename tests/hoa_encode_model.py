"""A float64 numpy model of the Ambisonic encoder, written from the text of include/earhip.h group Q alone: the Legendre
recurrence, the norms, T_m, the exact fmod of the azimuth.  Shared by the CPU and GPU tests of the encoder."""
import math

import numpy as np

FUMA = {(0, 0): 1 / math.sqrt(2), (1, 0): 1.0, (1, 1): 1.0, (2, 0): 1.0, (2, 1): 2 / math.sqrt(3), (2, 2): 2 / math.sqrt(3),
        (3, 0): 1.0, (3, 1): math.sqrt(45 / 32), (3, 2): 3 / math.sqrt(5), (3, 3): math.sqrt(8 / 5)}
FUMA_WXYZ = ([0, 1, 1, 1], [0, 1, -1, 0])


def acn(order):
    idx = [(n, m) for n in range(order + 1) for m in range(-n, n + 1)]
    return [n for n, _ in idx], [m for _, m in idx]


def norm(name, n, a):
    sn3d = math.sqrt(math.factorial(n - a) / math.factorial(n + a))
    if name == "SN3D":
        return sn3d
    if name == "N3D":
        return math.sqrt(2 * n + 1) * sn3d
    assert name == "FuMa" and n <= 3
    return FUMA[(n, a)] * sn3d


def legendre(n, a, x):
    """P_n^a(x) without the Condon-Shortley phase, by the header's upward recurrence; x an array"""
    x = np.asarray(x, np.float64)
    s = np.sqrt((1.0 - x) * (1.0 + x))
    p0 = np.ones_like(x)
    for i in range(1, a + 1):
        p0 = p0 * ((2.0 * i - 1.0) * s)
    if n == a:
        return p0
    p1 = x * (2.0 * a + 1.0) * p0
    for l in range(a + 2, n + 1):
        p0, p1 = p1, (x * (2.0 * l - 1.0) * p1 - (l + a - 1.0) * p0) / (l - a)
    return p1


def harmonic_rad(n, m, r, x, name="N3D"):
    """K P T at azimuth r (radians) and x = sin(elevation); arrays"""
    r = np.asarray(r, np.float64)
    t = math.sqrt(2.0) * np.cos(m * r) if m > 0 else (-math.sqrt(2.0) * np.sin(m * r) if m < 0 else np.ones_like(r))
    return norm(name, n, abs(m)) * legendre(n, abs(m), x) * t


def encode64(orders, degrees, az, el, gain=None, name="SN3D"):
    """float64 [n][n_coef]: gain * K * P * T, left to right"""
    az = np.atleast_1d(np.asarray(az, np.float64))
    el = np.broadcast_to(np.asarray(el, np.float64), az.shape)
    g = np.ones_like(az) if gain is None else np.broadcast_to(np.asarray(gain, np.float64), az.shape)
    r = np.fmod(az, 360.0) * (math.pi / 180.0)
    x = np.sin(el * (math.pi / 180.0))
    out = np.empty((az.size, len(orders)), np.float64)
    for c, (n, m) in enumerate(zip(orders, degrees)):
        a = abs(m)
        t = math.sqrt(2.0) * np.cos(m * r) if m > 0 else (-math.sqrt(2.0) * np.sin(m * r) if m < 0 else np.ones_like(r))
        out[:, c] = g * norm(name, n, a) * legendre(n, a, x) * t
    return out


def encode(orders, degrees, az, el, gain=None, name="SN3D"):
    return encode64(orders, degrees, az, el, gain, name).astype(np.float32)


def spacing_bar(want64):
    """one float32 spacing at max(|want|, 2^-20): the bar of the host and device forms against float32(reference)"""
    w = np.maximum(np.abs(np.asarray(want64, np.float64)), 2.0 ** -20).astype(np.float32)
    return np.spacing(w).astype(np.float64)


def within_one_spacing(got32, want64):
    """(ok, worst error / bar): got against float32(want64)"""
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    err = np.abs(got32.astype(np.float64) - want32.astype(np.float64))
    bar = spacing_bar(want64)
    return bool(np.all(err <= bar)), float(np.max(err / bar))


def cart(az, el):
    """ADM polar degrees -> unit vectors (x right, y front, z up), [n][3]"""
    a, e = np.radians(np.asarray(az, np.float64)), np.radians(np.asarray(el, np.float64))
    return np.stack([-np.sin(a) * np.cos(e), np.cos(a) * np.cos(e), np.sin(e)], axis=-1)


def polar(v):
    """unit vectors [n][3] -> (az, el) in degrees"""
    v = np.asarray(v, np.float64)
    return -np.degrees(np.arctan2(v[:, 0], v[:, 1])), np.degrees(np.arcsin(np.clip(v[:, 2], -1.0, 1.0)))


def random_rotation(rng):
    """a proper rotation, 3 x 3, from a seeded generator"""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def yaw(deg):
    """anticlockwise about z (up): azimuth + deg"""
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
