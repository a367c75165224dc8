"""An independent numpy restatement of libear's GainCalculatorDirectSpeakers::calculate
(src/direct_speakers/gain_calculator_direct_speakers.cpp:244-320), the checker of capi.DirectSpeakers.

Metadata is the dict form capi.DirectSpeakers takes.  The point source panner of step 6 is passed in as
`psp(az, el) -> gains [n][n_channels]` (the pinned oracle panner in the tests), so that everything else can
run without a device.  Rows that need the panner are collected and panned in one call, as the library does.
"""
import re

import numpy as np

import _oracle

TOL = 1e-5
URN0 = "urn:itu:bs:2051:0:speaker:"
DEFAULT_SUBSTITUTIONS = {"LFE": "LFE1", "LFEL": "LFE1", "LFER": "LFE2"}
FREQ_SPEAKERLABEL_LFE_MISMATCH, FREQ_NOT_LFE = 1, 2
_URN = re.compile(r"urn:itu:bs:2051:[0-9]+:speaker:([^\r\n]*)")
_COMMON_PACK = re.compile(r"AP_0001[0-9a-fA-F]{4}")


class AdmError(Exception):
    pass


class NotImplementedCase(Exception):
    pass


def inside_angle_range(x, start, end, tol=0.0):
    """src/common/geom.cpp:7-28"""
    while end - 360.0 > start:
        end -= 360.0
    while end < start:
        end += 360.0
    start_tol = start - tol
    while x - 360.0 >= start_tol:
        x -= 360.0
    while x < start_tol:
        x += 360.0
    return x <= end + tol


class Model:
    """channels: [(name, nominal azimuth, nominal elevation, is_lfe)] of the full layout; real: (azimuths,
    elevations) of the loudspeakers' real positions, None: nominal"""

    def __init__(self, channels, substitutions=None, real=None):
        self.names = [c[0] for c in channels]
        self.az = np.array([c[1] for c in channels], np.float64)
        self.el = np.array([c[2] for c in channels], np.float64)
        self.lfe = np.array([c[3] for c in channels], bool)
        raz, rel = (self.az, self.el) if real is None else (np.asarray(real[0], np.float64), np.asarray(real[1], np.float64))
        self.real_xyz = _oracle.cart(raz, rel)
        self.subst = dict(substitutions or {})
        self.subst.update(DEFAULT_SUBSTITUTIONS)  # (std::map::insert: a default is never overridden)

    def nominal_label(self, label):
        m = _URN.fullmatch(label)
        ret = m.group(1) if m else label
        return self.subst.get(label, ret)

    def _bounds(self, m, lfe):
        az, el, dist = m.get("azimuth", 0.0), m.get("elevation", 0.0), m.get("distance", 1.0)

        def get(k, default):
            return default if m.get(k) is None else m[k]
        az0, az1 = get("azimuthMin", az), get("azimuthMax", az)
        el0, el1 = get("elevationMin", el), get("elevationMax", el)
        d0, d1 = get("distanceMin", dist), get("distanceMax", dist)
        p = _oracle.cart(az, el, dist)
        found = []
        for c in range(len(self.names)):
            if self.lfe[c] != lfe:
                continue
            if ((inside_angle_range(self.az[c], az0, az1, TOL) or abs(self.el[c]) >= 90.0 - TOL)
                    and el0 - TOL < self.el[c] < el1 + TOL and d0 - TOL < 1.0 < d1 + TOL):
                found.append((float(np.linalg.norm(self.real_xyz[c] - p)), c))
        if len(found) == 1:
            return found[0][1]
        found.sort()
        if len(found) > 1 and abs(found[0][0] - found[1][0]) > TOL:
            return found[0][1]
        return None

    def one(self, m):
        """-> (gains [n_channels] or None when the panner is needed, [warning codes]); raises AdmError /
        NotImplementedCase as the library refuses"""
        labels = list(m.get("speakerLabels", ()))
        if m.get("audioPackFormatID") is not None and not labels:
            raise AdmError("audioPackFormatID without speakerLabels")
        if m.get("cartesian"):
            raise NotImplementedCase("Cartesian position")
        warnings = []
        lp, hp = m.get("lowPass"), m.get("highPass")
        lfe_freq = lp is not None and lp <= 200 and hp is None
        if not lfe_freq and (lp is not None or hp is not None):
            warnings.append(FREQ_NOT_LFE)
        lfe_name = any(self.nominal_label(lab) in ("LFE1", "LFE2") for lab in labels)
        if lfe_freq != lfe_name and labels:
            warnings.append(FREQ_SPEAKERLABEL_LFE_MISMATCH)
        lfe = lfe_freq or lfe_name
        pack = m.get("audioPackFormatID")
        if pack is not None and _COMMON_PACK.fullmatch(pack):
            raise NotImplementedCase(pack)
        g = np.zeros(len(self.names), np.float32)
        for lab in labels:
            nominal = self.nominal_label(lab)
            if nominal in self.names and self.lfe[self.names.index(nominal)] == lfe:
                g[self.names.index(nominal)] = 1.0
                return g, warnings
        sel = m.get("screenEdgeLock") or {}
        if sel.get("horizontal") is not None or sel.get("vertical") is not None:
            raise NotImplementedCase("screenEdgeLock")
        c = self._bounds(m, lfe)
        if c is not None:
            g[c] = 1.0
            return g, warnings
        if lfe:
            if "LFE1" in self.names:
                g[self.names.index("LFE1")] = 1.0
            return g, warnings
        return None, warnings

    def calculate(self, metadata, psp):
        """-> (gains float32 [n][n_channels], warnings int32 [n][2])"""
        n = len(metadata)
        gains = np.zeros((n, len(self.names)), np.float32)
        warnings = np.zeros((n, 2), np.int32)
        rows = []
        for i, m in enumerate(metadata):
            g, w = self.one(m)
            warnings[i, :len(w)] = w
            if g is None:
                rows.append(i)
            else:
                gains[i] = g
        if rows:
            az = np.array([metadata[i].get("azimuth", 0.0) for i in rows], np.float64)
            el = np.array([metadata[i].get("elevation", 0.0) for i in rows], np.float64)
            gains[rows] = psp(az, el)
        return gains, warnings


def oracle_psp(layout, real=None):
    """the pinned oracle panner (oracle/panner_oracle.hpp) as step 6 wants it: direct gains, LFE columns zero"""
    o = _oracle.GainCalculatorObjects(layout, real)
    return lambda az, el: o.calculate(az, el)[0]


def random_metadata(ch, n, seed, bounds=0.7):
    """n metadata dicts around the channels ch of a layout ([(name, azimuth, elevation, is_lfe)]): labels (URNs,
    substitutions, LFE names, missing ones), frequencies, positions near the loudspeakers with and without bounds"""
    rng = np.random.default_rng(seed)
    pool = [c[0] for c in ch] + ["B+000", "M+135", "U+180", "LFE", "LFEL", "LFER", "LFE2", "foo"]
    out = []
    for _ in range(n):
        md = {}
        if rng.random() < 0.4:
            k = int(rng.integers(1, 4))
            md["speakerLabels"] = [(URN0 if rng.random() < 0.5 else "") + pool[int(rng.integers(len(pool)))]
                                   for _ in range(k)]
        if rng.random() < 0.2:
            md["lowPass"] = float(rng.choice([80.0, 120.0, 200.0, 250.0, 1000.0]))
        if rng.random() < 0.05:
            md["highPass"] = 40.0
        c = ch[int(rng.integers(len(ch)))]
        md["azimuth"] = c[1] + float(rng.uniform(-25, 25))
        md["elevation"] = float(np.clip(c[2] + rng.uniform(-25, 25), -90, 90))
        if rng.random() < bounds:
            w_az, w_el = rng.uniform(0, 40, 2)
            md["azimuthMin"], md["azimuthMax"] = md["azimuth"] - w_az, md["azimuth"] + rng.uniform(0, 40)
            md["elevationMin"], md["elevationMax"] = md["elevation"] - w_el, md["elevation"] + rng.uniform(0, 40)
            if rng.random() < 0.3:
                md["distanceMin"] = 0.5
        out.append(md)
    return out
