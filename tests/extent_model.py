"""A plain float64 restatement of libear's PolarExtent::handle / calc_pv_spread (src/object_based/polar_extent.cpp:257-302) over
ANY point source panner, for the layouts the oracle has no table for: the grid from the oracle (PolarExtent.grid()), the point
gains from tests/custom_layout_model.py at the grid points, the weights from the oracle's double weighting function
(oracle_extent_weight, which=1), float64 sums.  tests/test_extent_cases_cpu.py first holds it to the oracle's double core
(handle(which=1)) on 4+5+0 at 1e-9; only then is it the reference for a defined layout."""
import numpy as np

import _oracle

FADE = 10.0


class PolarExtent:
    def __init__(self, pan):
        """pan: unit vectors [n][3] -> gains [n][loudspeakers that are not LFE] (custom_layout_model.Panner.pan's first result)"""
        self.pan = pan
        self.oracle = _oracle.PolarExtent("0+5+0")  # (its grid and its weighting function: neither depends on the layout)
        self.grid = self.oracle.grid()
        self.grid_gains = pan(self.grid)

    def spread(self, position, width, height):
        """calc_pv_spread (:257-288)"""
        amount_spread = float(np.interp(max(width, height), [0.0, FADE], [0.0, 1.0]))
        amount_point = 1.0 - amount_spread
        pv = np.zeros(self.grid_gains.shape[1])
        if amount_point > 1e-10:
            pv += amount_point * self.pan(position[None, :] / np.linalg.norm(position))[0] ** 2
        if amount_spread > 1e-10:
            width, height = max(width, FADE / 2.0), max(height, FADE / 2.0)
            w = np.array([self.oracle.weight(position, width, height, q, which=1) for q in self.grid])
            total = w @ self.grid_gains
            pv += amount_spread * (total / np.linalg.norm(total)) ** 2
        return np.sqrt(pv)

    def handle(self, xyz, width, height, depth):
        """positions [n][3] (none at the origin), extents in degrees -> pv [n][loudspeakers that are not LFE] (:290-302)"""
        out = []
        for p, w, h, dp in zip(np.asarray(xyz, np.float64).reshape(-1, 3), width, height, depth):
            distance = float(np.linalg.norm(p))
            if dp != 0.0:
                near, far = max(distance - dp / 2.0, 0.0), max(distance + dp / 2.0, 0.0)
                a = self.spread(p, _oracle.extent_mod(w, near), _oracle.extent_mod(h, near))
                b = self.spread(p, _oracle.extent_mod(w, far), _oracle.extent_mod(h, far))
                out.append(np.sqrt((a * a + b * b) / 2.0))
            else:
                out.append(self.spread(p, _oracle.extent_mod(w, distance), _oracle.extent_mod(h, distance)))
        return np.array(out)
