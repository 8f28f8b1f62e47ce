"""NumPy restatement of the terrain plant residual (TEST INFRASTRUCTURE ONLY): the reference's environments written from
their formulas (src/simulation/environments/*.jl), `rotation` (src/simulator/environment.jl:58-92, the 2-D one through its
atan form), and the residual of simulation.jl:133-158 with the models' terrain overrides, built on oracle/plant.py's classes.
Everything is complex-safe (branches on x.real), so `jacobian_z` by complex step stays exact and `oracle.plant.plant_step`
runs on these plants unchanged."""
from __future__ import annotations

import math

import numpy as np

from oracle import plant as pl
from oracle.dims import Dims


# ---- surfaces: name -> (surf, surf_grad, 3-D?) ------------------------------------------------------------------------
def _blends(m):
    def solve(x1, y1, m1, x2, y2, m2):
        A = np.array([[x1 ** 3, x1 ** 2, x1, 1.0], [x2 ** 3, x2 ** 2, x2, 1.0],
                      [3.0 * x1 ** 2, 2.0 * x1, 1.0, 0.0], [3.0 * x2 ** 2, 2.0 * x2, 1.0, 0.0]])
        return np.linalg.solve(A, np.array([y1, y2, m1, m2]))
    return solve(0.4, 0.0, 0.0, 0.6, m * 0.1, m), solve(1.4, m * 1.4, m, 1.6, m * 1.5 + (-0.25 * m) * 0.1, -0.25 * m)


poly = lambda a, z: a[3] + a[2] * z + a[1] * z ** 2 + a[0] * z ** 3
d_poly = lambda a, z: a[2] + 2.0 * a[1] * z + 3.0 * a[0] * z ** 2


def _piecewise(m):
    a1, a2 = _blends(m)
    def s(x):
        xr = np.real(x)
        return np.where(xr < 0.4, 0.0 * x, np.where(xr < 0.6, poly(a1, x), np.where(xr < 1.9, m * x - 0.5 * m,
                        np.where(xr < 2.1, poly(a2, x - 0.5), -0.250 * m * (x - 2.0) + 1.5 * m))))
    def g(x):
        xr = np.real(x)
        return np.where(xr < 0.4, 0.0 * x, np.where(xr < 0.6, d_poly(a1, x), np.where(xr < 1.9, m + 0.0 * x,
                        np.where(xr < 2.1, d_poly(a2, x - 0.5), -0.250 * m + 0.0 * x))))
    return s, g


def _stairs3(x):
    xr = np.real(x)
    return np.where(xr < 0.125, 0.0, np.where(xr < 0.375, 0.25, np.where(xr < 0.625, 0.5, np.where(xr < 0.875, 0.75, 0.0)))) + 0.0 * x


M10, T_SS = math.tan(math.radians(10.0)), 25.0
SURFACES = {
    "flat_2D_lc": (lambda x: 0.0 * x, lambda x: 0.0 * x, False),
    "flat_3D_lc": (lambda x, y: 0.0 * x, lambda x, y: (0.0 * x, 0.0 * y), True),
    "slope1_2D_lc": (lambda x: 0.5 * x, lambda x: 0.5 + 0.0 * x, False),
    "slope_smooth_2D_lc": (lambda x: M10 / T_SS * np.log(1.0 + np.exp(T_SS * (x - 0.5))),
                           lambda x: M10 * np.exp(T_SS * (x - 0.5)) / (1.0 + np.exp(T_SS * (x - 0.5))), False),
    "sine1_2D_lc": (lambda x: 0.05 * (np.cos(np.pi * x) - 1.0), lambda x: -0.05 * np.pi * np.sin(np.pi * x), False),
    "sine2_2D_lc": (lambda x: 0.10 * np.sin(2 * np.pi * x), lambda x: 0.10 * 2 * np.pi * np.cos(2 * np.pi * x), False),
    "sine3_2D_lc": (lambda x: 0.03 * (np.cos(np.pi * x) - 1.0), lambda x: -0.03 * np.pi * np.sin(np.pi * x), False),
    "piecewise1_2D_lc": _piecewise(math.tan(math.radians(10.0))) + (False,),
    "piecewise2_2D_lc": _piecewise(math.tan(math.radians(-10.0))) + (False,),
    "stairs3_2D_lc": (_stairs3, lambda x: 0.0 * x, False),
    "sine1_3D_lc": (lambda x, y: np.sin(x) + np.sin(y), lambda x, y: (np.cos(x), np.cos(y)), True),
    "sine2_3D_lc": (lambda x, y: 0.075 * np.sin(2 * np.pi * x), lambda x, y: (0.075 * 2 * np.pi * np.cos(2 * np.pi * x), 0.0 * y), True),
    "sine3_3D_lc": (lambda x, y: 0.075 * np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y),
                    lambda x, y: (0.075 * 2 * np.pi * np.cos(2 * np.pi * x) * np.sin(2 * np.pi * y),
                                  0.075 * 2 * np.pi * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)), True),
    "quadratic_bowl_3D_lc": (lambda x, y: x ** 2 + y ** 2, lambda x, y: (2.0 * x, 2.0 * y), True),
}


def rotation_2d(g):
    """environment.jl:79-92: ns = (-g, 1)/|.|, ang = atan(1, 0) - atan(ns_z, ns_x), R = [cos -sin; sin cos] (complex-safe: the
    closed form of the atan, which the reference's own formula equals; checked against the atan form on reals in the tests)."""
    c = 1.0 / np.sqrt(1.0 + g * g)
    s = -g * c
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def rotation_2d_atan(g):
    ns = np.array([-g, 1.0]) / math.sqrt(1.0 + g * g)
    ang = math.atan2(1.0, 0.0) - math.atan2(ns[1], ns[0])
    return np.array([[math.cos(ang), -math.sin(ang)], [math.sin(ang), math.cos(ang)]])


def _skew(v):
    z = 0.0 * v[..., 0]
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def rotation_3d(gx, gy):
    """environment.jl:58-77: rot(ns, e_z) = I + [v]x + [v]x^2 / (1 + c), v = ns x e_z, c = ns . e_z."""
    n = np.stack([-gx, -gy, 1.0 + 0.0 * gx], -1)
    ns = n / np.sqrt(np.sum(n * n, axis=-1, keepdims=True))
    ez = np.array([0.0, 0.0, 1.0])
    v = np.cross(ns, np.broadcast_to(ez, ns.shape))
    c = ns[..., 2]
    S = _skew(v)
    return np.eye(3) + S + (S @ S) / (1.0 + c)[..., None, None]


def _unpack(P, z, th):
    nq, nu, nw, nc, nb = P.nq, P.nu, P.nw, P.nc, P.nb
    ot = np.cumsum([0, nq, nq, nu, nw, 1, 1])
    o = np.cumsum([0, nq, nc, nb, nc, nc, nb, nc])
    return [th[..., ot[i]:ot[i + 1]] for i in range(6)], [z[..., o[i]:o[i + 1]] for i in range(7)]


def _tail(gam, b, psi, s1, eta, s2, mu, phi, vstack, nf, kappa):
    Eb = b.reshape(b.shape[:-1] + (-1, nf)).sum(axis=-1)
    return [s1 - phi, eta - vstack - np.repeat(psi, nf, axis=-1), s2 - (mu * gam - Eb), gam * s1 - kappa, b * eta - kappa, psi * s2 - kappa]


class _Planar:
    """Foot-wise terrain residual for the planar models: p_i, J_i (2 x nq) at q2 from the base class."""

    def __init__(self, name, *a, **k):
        super().__init__(*a, **k)
        self.terrain = name
        self.surf, self.grad, is3 = SURFACES[name]
        assert not is3

    def residual(self, z, th, kappa):
        (q0, q1, u1, w1, mu, h), (q2, gam, b, psi, s1, eta, s2) = _unpack(self, z, th)
        dyn0 = self.free_dynamics(q0, q1, u1, w1, q2, h)
        p, J = self.contacts(q2)                                              # (..., nc, 2), (..., nc, 2, nq)
        R = rotation_2d(self.grad(p[..., 0]))                             # per foot, at its own x
        lt = b[..., 0::2] - b[..., 1::2]
        lam = np.einsum("...cji,...cj->...ci", R, np.stack([lt, gam], -1))            # R^T [m b; γ]
        dyn = dyn0 + np.einsum("...cin,...ci->...n", J, lam)
        v = np.einsum("...cin,...n->...ci", J, (q2 - q1) / h)
        vt = np.einsum("...cij,...cj->...ci", R, v)[..., 0]
        vstack = np.stack([vt, -vt], -1).reshape(vt.shape[:-1] + (-1,))
        phi = p[..., 1] - self.surf(p[..., 0])
        return np.concatenate([dyn] + _tail(gam, b, psi, s1, eta, s2, mu, phi, vstack, 2, kappa), axis=-1)


class ChainTerrainPlant(_Planar):
    def free_dynamics(self, q0, q1, u1, w1, q2, h):
        qm1, vm1, qm2, vm2 = 0.5 * (q0 + q1), (q1 - q0) / h, 0.5 * (q1 + q2), (q2 - q1) / h
        a1, b1 = self.lagrangian_derivatives(qm1, vm1)
        a2, b2 = self.lagrangian_derivatives(qm2, vm2)
        Au = np.zeros_like(q2)
        Au[..., 0:2] = w1
        return 0.5 * h * a1 + b1 + 0.5 * h * a2 - b2 + u1 @ self.B + Au - h * self.joint_friction * vm2

    def contacts(self, q2):
        P = self.foot_positions(q2)
        J = self.foot_jacobian(q2)
        nc = self.nc
        return P.reshape(P.shape[:-1] + (nc, 2)), J.reshape(J.shape[:-2] + (nc, 2, self.nq))


class QuadrupedTerrainPlant(ChainTerrainPlant, pl.QuadrupedPlant):
    pass


class FlamingoTerrainPlant(ChainTerrainPlant, pl.FlamingoPlant):
    pass


class HopperTerrainPlant(_Planar, pl.HopperPlant):
    def free_dynamics(self, q0, q1, u1, w1, q2, h):
        qm1, vm1, qm2, vm2 = 0.5 * (q0 + q1), (q1 - q0) / h, 0.5 * (q1 + q2), (q2 - q1) / h
        a1, b1 = self.lagrangian_derivatives(qm1, vm1)
        a2, b2 = self.lagrangian_derivatives(qm2, vm2)
        sm, cm = np.sin(qm2[..., 2]), np.cos(qm2[..., 2])
        Bu = np.stack([-sm * u1[..., 1], cm * u1[..., 1], u1[..., 0], u1[..., 1]], axis=-1)
        Aw = np.concatenate([w1, np.zeros_like(w1)], axis=-1)
        return 0.5 * h * a1 + b1 + 0.5 * h * a2 - b2 + Bu + Aw

    def contacts(self, q2):
        st, ct, r = np.sin(q2[..., 2]), np.cos(q2[..., 2]), q2[..., 3]
        one, zero = np.ones_like(st), np.zeros_like(st)
        p = np.stack([q2[..., 0] + r * st, q2[..., 1] - r * ct], -1)[..., None, :]
        J = np.stack([np.stack([one, zero, r * ct, st], -1), np.stack([zero, one, r * st, -ct], -1)], -2)[..., None, :, :]
        return p, J


class Particle2DPlant:
    """particle_2D (src/dynamics/particle_2D/model.jl): q = (x, z), m = 1, g = 9.81, μ_world = 1, B = A = J = I."""
    nq, nu, nw, nc, nb = 2, 2, 2, 1, 2
    m, g, mu_world = 1.0, 9.81, 1.0
    jacobian_z = pl.PlanarChainPlant.jacobian_z

    def __init__(self):
        self.dims = Dims(nq=2, nu=2, nw=2, nc=1, nb=2)

    def free_dynamics(self, q0, q1, u1, w1, q2, h):
        grav = np.zeros_like(q2); grav[..., 1] = -self.m * self.g
        return 0.5 * h * grav + self.m * (q1 - q0) / h + 0.5 * h * grav - self.m * (q2 - q1) / h + u1 + w1

    def contacts(self, q2):
        J = np.broadcast_to(np.eye(2), q2.shape[:-1] + (1, 2, 2)).astype(q2.dtype)
        return q2[..., None, :], J


class Particle2DTerrainPlant(_Planar, Particle2DPlant):
    pass


class ParticleTerrainPlant(pl.ParticlePlant):
    """particle/model.jl:58-109 on a 3-D surface: ϕ = z - surf(x, y), λ = R^T [m b; γ], v_T = (R v)[1:2]."""

    def __init__(self, name):
        super().__init__()
        self.terrain = name
        self.surf, self.grad, is3 = SURFACES[name]
        assert is3

    def residual(self, z, th, kappa):
        q0, q1, u1, w1, mu, h = th[..., 0:3], th[..., 3:6], th[..., 6:9], th[..., 9:12], th[..., 12:13], th[..., 13:14]
        q2, gam, b, psi, s1, eta, s2 = z[..., 0:3], z[..., 3:4], z[..., 4:8], z[..., 8:9], z[..., 9:10], z[..., 10:14], z[..., 14:15]
        vm1, vm2 = (q1 - q0) / h, (q2 - q1) / h
        grav = np.zeros_like(q2); grav[..., 2] = -self.m * self.g
        gx, gy = self.grad(q2[..., 0], q2[..., 1])
        R = rotation_3d(gx + 0.0 * q2[..., 0], gy + 0.0 * q2[..., 0])
        f = np.stack([b[..., 0] - b[..., 2], b[..., 1] - b[..., 3], gam[..., 0]], axis=-1)
        lam = np.einsum("...ji,...j->...i", R, f)
        dyn = 0.5 * h * grav + self.m * vm1 + 0.5 * h * grav - self.m * vm2 + u1 + w1 + lam
        vs = np.einsum("...ij,...j->...i", R, vm2)
        vstack = np.stack([vs[..., 0], vs[..., 1], -vs[..., 0], -vs[..., 1]], axis=-1)
        phi = q2[..., 2:3] - self.surf(q2[..., 0], q2[..., 1])[..., None]
        return np.concatenate([dyn] + _tail(gam, b, psi, s1, eta, s2, mu, phi, vstack, 4, kappa), axis=-1)


def plant(model: str, terrain: str):
    """The CPU restatement of `plant.plant_step(model, ..., terrain=terrain)`."""
    if model == "particle":
        return ParticleTerrainPlant(terrain)
    cls = {"quadruped": QuadrupedTerrainPlant, "flamingo": FlamingoTerrainPlant, "hopper_2D": HopperTerrainPlant,
           "particle_2D": Particle2DTerrainPlant}[model]
    return cls(terrain)
