"""Terrains of the device plant step (`cimpc_plant_step_terrain`, include/cimpc.h).

The reference's environments (src/simulation/environments/*.jl) as `cimpc_terrain` values: a kind plus fp64 parameters,
with host-side `surface` / `gradient` that evaluate exactly what the device evaluates.

  flat_2D_lc, flat_3D_lc          0                                              FLAT
  slope1_2D_lc                    0.5 x                                          PIECEWISE (one piece)
  slope_smooth_2D_lc              (m/t) log(1 + e^{t (x - 0.5)}), m = tan 10°, t = 25   SOFTPLUS (overflow-safe)
  sine1/2/3_2D_lc                 0.05 (cos πx - 1), 0.10 sin 2πx, 0.03 (cos πx - 1)    SINE
  piecewise1/2_2D_lc              generate_piecewise_terrain(tan(±10°)): lines joined by cubic blends   PIECEWISE
  stairs3_2D_lc                   steps at 0.125 / 0.375 / 0.625 / 0.875             PIECEWISE (zero gradient)
  sine1/2_3D_lc                   sin x + sin y, 0.075 sin 2πx                   SINE_SUM_3D
  sine3_3D_lc                     0.075 sin 2πx sin 2πy                          SINE_PRODUCT_3D
  quadratic_bowl_3D_lc            x² + y²                                        BOWL_3D

The planar models stand on the `_2D_` terrains, particle and hopper_3D on the `_3D_` ones (`terrain_valid_for`, csrc/plant_model.h).
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from ._lib import Terrain as CTerrain

FLAT, PIECEWISE, SOFTPLUS, SINE, SINE_SUM_3D, SINE_PRODUCT_3D, BOWL_3D = range(7)
KINDS_3D = (SINE_SUM_3D, SINE_PRODUCT_3D, BOWL_3D)


@dataclasses.dataclass
class Terrain:
    """kind, analytic parameters p (4), and for PIECEWISE the pieces: (start, offset, (c0, c1, c2, c3)) with piece i valid for
    x >= start (the first piece from -inf), value sum_k c_k (x - offset)^k."""
    name: str
    kind: int
    p: tuple = (0.0, 0.0, 0.0, 0.0)
    pieces: tuple = ()
    spatial: bool = False              # surf(x, y) (flat_3D_lc and the 3-D kinds) rather than surf(x)

    @property
    def is_3d(self) -> bool:
        return self.spatial or self.kind in KINDS_3D

    def to_c(self) -> CTerrain:
        t = CTerrain()
        t.kind = self.kind
        t.n_pieces = len(self.pieces)
        for i, v in enumerate(self.p):
            t.p[i] = v
        for i, (start, off, c) in enumerate(self.pieces):
            t.brk[i] = 0.0 if i == 0 else start
            t.off[i] = off
            for k in range(4):
                t.coef[i][k] = c[k]
        return t

    def _piece(self, x):
        starts = np.array([s for s, _, _ in self.pieces[1:]])
        return np.searchsorted(starts, x, side="right")        # number of starts <= x

    def surface(self, x, y=0.0):
        """surf(x) (planar) or surf(x, y) (3-D), as the device evaluates it; x, y scalars or arrays."""
        x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
        p = self.p
        if self.kind == FLAT:
            return np.zeros(np.broadcast(x, y).shape)
        if self.kind == PIECEWISE:
            i = self._piece(x)
            off = np.array([o for _, o, _ in self.pieces])[i]
            c = np.array([cc for _, _, cc in self.pieces])[i]
            t = x - off
            return ((c[..., 3] * t + c[..., 2]) * t + c[..., 1]) * t + c[..., 0]
        if self.kind == SOFTPLUS:
            u = p[1] * (x - p[2])
            return (p[0] / p[1]) * (np.maximum(u, 0.0) + np.log1p(np.exp(-np.abs(u))))
        if self.kind == SINE:
            return (p[0] * np.cos(p[2] * x) + p[1] * np.sin(p[2] * x)) + p[3]
        if self.kind == SINE_SUM_3D:
            return p[0] * np.sin(p[1] * x) + p[2] * np.sin(p[3] * y)
        if self.kind == SINE_PRODUCT_3D:
            return p[0] * (np.sin(p[1] * x) * np.sin(p[1] * y))
        if self.kind == BOWL_3D:
            return p[0] * (x * x + y * y)
        raise ValueError(f"unknown terrain kind {self.kind}")

    def gradient(self, x, y=0.0):
        """surf_grad: d surf / dx (planar) or (d/dx, d/dy) stacked on the last axis (3-D)."""
        x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
        p = self.p
        zero = np.zeros(np.broadcast(x, y).shape)
        if self.kind == FLAT:
            gx, gy = zero, zero
        elif self.kind == PIECEWISE:
            i = self._piece(x)
            off = np.array([o for _, o, _ in self.pieces])[i]
            c = np.array([cc for _, _, cc in self.pieces])[i]
            t = x - off
            gx, gy = (3.0 * c[..., 3] * t + 2.0 * c[..., 2]) * t + c[..., 1], zero
        elif self.kind == SOFTPLUS:
            u = p[1] * (x - p[2])
            e = np.exp(-np.abs(u))
            gx, gy = np.where(u > 0.0, p[0] / (1.0 + e), p[0] * e / (1.0 + e)), zero
        elif self.kind == SINE:
            gx, gy = p[2] * (p[1] * np.cos(p[2] * x) - p[0] * np.sin(p[2] * x)), zero
        elif self.kind == SINE_SUM_3D:
            gx, gy = p[0] * p[1] * np.cos(p[1] * x) + zero, p[2] * p[3] * np.cos(p[3] * y) + zero
        elif self.kind == SINE_PRODUCT_3D:
            gx, gy = p[0] * p[1] * (np.cos(p[1] * x) * np.sin(p[1] * y)), p[0] * p[1] * (np.sin(p[1] * x) * np.cos(p[1] * y))
        elif self.kind == BOWL_3D:
            gx, gy = 2.0 * p[0] * x + zero, 2.0 * p[0] * y + zero
        else:
            raise ValueError(f"unknown terrain kind {self.kind}")
        return np.stack([gx, gy], axis=-1) if self.is_3d else gx


def _poly(a, z):            # piecewise.jl: poly(a, z) = a[4] + a[3] z + a[2] z^2 + a[1] z^3
    return a[3] + a[2] * z + a[1] * z ** 2 + a[0] * z ** 3


def _d_poly(a, z):
    return a[2] + 2.0 * a[1] * z + 3.0 * a[0] * z ** 2


def piecewise_blends(m_ss: float):
    """The two cubic blends of `generate_piecewise_terrain` (piecewise.jl:29-74): 4 x 4 solves matching value and slope at the
    knots (0.4, 0.6) and (1.4, 1.6).  Returns (a1, a2) in the reference's order (a[0] = cubic coefficient)."""
    def solve(x1, y1, m1, x2, y2, m2):
        A = np.array([[x1 ** 3, x1 ** 2, x1, 1.0], [x2 ** 3, x2 ** 2, x2, 1.0],
                      [3.0 * x1 ** 2, 2.0 * x1, 1.0, 0.0], [3.0 * x2 ** 2, 2.0 * x2, 1.0, 0.0]])
        a = np.linalg.solve(A, np.array([y1, y2, m1, m2]))
        assert abs(_poly(a, x1) - y1) < 1e-8 and abs(_poly(a, x2) - y2) < 1e-8      # the reference's @asserts
        return a
    a1 = solve(0.4, 0.0 * 0.4, 0.0, 0.6, m_ss * 0.1, m_ss)
    a2 = solve(1.4, m_ss * 1.4, m_ss, 1.6, m_ss * 1.5 + (-0.25 * m_ss) * 0.1, -0.25 * m_ss)
    return a1, a2


def piecewise(name: str, m_ss: float) -> Terrain:
    """generate_piecewise_terrain(m_ss, repeat = false): 0 | blend a1 | m x - m/2 | blend a2 in (x - 0.5) | -m/4 (x - 2) + 3m/2,
    with breaks at 0.4, 0.6, 1.9, 2.1."""
    a1, a2 = piecewise_blends(m_ss)
    c = lambda a: (a[3], a[2], a[1], a[0])
    return Terrain(name, PIECEWISE, pieces=((None, 0.0, (0.0, 0.0, 0.0, 0.0)), (0.4, 0.0, c(a1)),
                                            (0.6, 0.0, (-0.5 * m_ss, m_ss, 0.0, 0.0)), (1.9, 0.5, c(a2)),
                                            (2.1, 2.0, (1.5 * m_ss, -0.25 * m_ss, 0.0, 0.0))))


def _stairs3():
    steps = ((0.125, 0.25), (0.375, 0.50), (0.625, 0.75), (0.875, 0.0))
    return Terrain("stairs3_2D_lc", PIECEWISE, pieces=((None, 0.0, (0.0, 0.0, 0.0, 0.0)),)
                   + tuple((s, 0.0, (a, 0.0, 0.0, 0.0)) for s, a in steps))


_M10 = math.tan(math.radians(10.0))


def _table():
    return {
        "flat_2D_lc": Terrain("flat_2D_lc", FLAT),
        "flat_3D_lc": Terrain("flat_3D_lc", FLAT, spatial=True),
        "slope1_2D_lc": Terrain("slope1_2D_lc", PIECEWISE, pieces=((None, 0.0, (0.0, 0.5, 0.0, 0.0)),)),
        "slope_smooth_2D_lc": Terrain("slope_smooth_2D_lc", SOFTPLUS, p=(_M10, 25.0, 0.5, 0.0)),
        "sine1_2D_lc": Terrain("sine1_2D_lc", SINE, p=(0.05, 0.0, math.pi, -0.05)),
        "sine2_2D_lc": Terrain("sine2_2D_lc", SINE, p=(0.0, 0.10, 2.0 * math.pi, 0.0)),
        "sine3_2D_lc": Terrain("sine3_2D_lc", SINE, p=(0.03, 0.0, math.pi, -0.03)),
        "piecewise1_2D_lc": piecewise("piecewise1_2D_lc", math.tan(math.radians(10.0))),
        "piecewise2_2D_lc": piecewise("piecewise2_2D_lc", math.tan(math.radians(-10.0))),
        "stairs3_2D_lc": _stairs3(),
        "sine1_3D_lc": Terrain("sine1_3D_lc", SINE_SUM_3D, p=(1.0, 1.0, 1.0, 1.0)),
        "sine2_3D_lc": Terrain("sine2_3D_lc", SINE_SUM_3D, p=(0.075, 2.0 * math.pi, 0.0, 0.0)),
        "sine3_3D_lc": Terrain("sine3_3D_lc", SINE_PRODUCT_3D, p=(0.075, 2.0 * math.pi, 0.0, 0.0)),
        "quadratic_bowl_3D_lc": Terrain("quadratic_bowl_3D_lc", BOWL_3D, p=(1.0, 0.0, 0.0, 0.0)),
    }


NAMES = tuple(_table())


def get(name: str) -> Terrain:
    """The terrain of a reference environment name (src/simulation/environments/*.jl)."""
    t = _table()
    if name not in t:
        raise KeyError(f"unknown terrain {name!r}; known: {', '.join(NAMES)}")
    return t[name]
