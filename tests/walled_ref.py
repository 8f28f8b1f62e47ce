"""NumPy restatement of pushbot (src/dynamics/pushbot/model.jl) and walledcartpole (src/dynamics/walledcartpole/model.jl) for the plant
tests: the residual of plant_residual_walls (contactimplicitmpc/jl_amd/csrc/plant_model.h) written from the model files in matrix form
(J_func as r1 G, r2 G; M and C in closed form from the Lagrangians), on complex input, so the oracle's complex-step Jacobian is exact to
round-off and `oracle.plant.plant_step` drives it.  Both models stand on flat_2D_lc (surface rotation = identity), so the generic
contact_forces and velocity_stack (src/simulation/contact_methods.jl:27-48) are the force [m b; γ] and the stack (v_T, -v_T).
tests/test_walled_models.py holds the closed forms against the automatic derivatives of lcp_models' Lagrangians."""
import functools

import numpy as np

from oracle import plant as pl
from oracle.dims import Dims
import terrain_ref as tr

R1 = np.array([[0.0, -1.0], [1.0, 0.0]])        # r1 of both J_func; r2 = -r1


class _WalledPlant:
    nc, nb = 2, 4
    g = 9.81
    jacobian_z = pl.PlanarChainPlant.jacobian_z

    def __init__(self):
        self.dims = Dims(nq=self.nq, nu=self.nu, nw=self.nw, nc=2, nb=4)
        self.joint_friction = np.asarray(self.joint_friction, dtype=float)

    def lagrangian_derivatives(self, q, v):          # D1L = -C(q, v), D2L = M(q) v (dynamics/model.jl:11-15)
        return -self.C(q, v), np.einsum("...ij,...j->...i", self.M(q), v)

    def residual(self, z, th, kappa):
        (q0, q1, u1, w1, mu, h), (q2, gam, b, psi, s1, eta, s2) = tr._unpack(self, z, th)
        qm1, vm1, qm2, vm2 = 0.5 * (q0 + q1), (q1 - q0) / h, 0.5 * (q1 + q2), (q2 - q1) / h
        a1, b1 = self.lagrangian_derivatives(qm1, vm1)
        a2, b2 = self.lagrangian_derivatives(qm2, vm2)
        J = self.J(q2)                                                                # (..., 4, nq): (tangent; normal) per contact
        lam = np.stack([b[..., 0] - b[..., 1], gam[..., 0], b[..., 2] - b[..., 3], gam[..., 1]], axis=-1)
        dyn = (0.5 * h * a1 + b1 + 0.5 * h * a2 - b2 + u1 @ self.B + w1 + np.einsum("...in,...i->...n", J, lam)
               - h * self.joint_friction * vm2)                                       # A = I
        vt = np.einsum("...in,...n->...i", J, vm2)[..., 0::2]
        vstack = np.stack([vt[..., 0], -vt[..., 0], vt[..., 1], -vt[..., 1]], axis=-1)
        return np.concatenate([dyn] + tr._tail(gam, b, psi, s1, eta, s2, mu, self.phi(q2), vstack, 2, kappa), axis=-1)


class PushBotPlant(_WalledPlant):
    """q = (θ, d); the arm's tip p = (-l sinθ + d cosθ, l cosθ + d sinθ) between walls at x = -+0.5 (model.jl:26-41, 87-104)."""
    nq, nu, nw = 2, 2, 2
    mu_world = 0.5
    mb, ma, l = 1.0, 0.01, 1.0
    joint_friction = (10.0, 10.0)
    B = np.array([[l, 1.0], [1.0, 1.0 / l]])        # B_func (:106-109)

    def point_x(self, q):
        return -self.l * np.sin(q[..., 0]) + q[..., 1] * np.cos(q[..., 0])

    def point_jacobian(self, q):                     # _jacobian, mode = :d (:46-48)
        s, c, d = np.sin(q[..., 0]), np.cos(q[..., 0]), q[..., 1]
        return np.stack([np.stack([-self.l * c - d * s, c], -1), np.stack([-self.l * s + d * c, s], -1)], -2)

    def M(self, q):                                  # mb Jcᵀ Jc + ma Jdᵀ Jd (:80-85), multiplied out
        d, l = q[..., 1], self.l
        o = np.ones_like(d)
        return np.stack([np.stack([self.mb * l * l + self.ma * (l * l + d * d), -self.ma * l * o], -1),
                         np.stack([-self.ma * l * o, self.ma * o], -1)], -2)

    def C(self, q, v):                               # (∂²L/∂q̇∂q) q̇ - ∂L/∂q of the Lagrangian (:66-78)
        s, c, d, l, g = np.sin(q[..., 0]), np.cos(q[..., 0]), q[..., 1], self.l, self.g
        return np.stack([2.0 * self.ma * d * v[..., 1] * v[..., 0] - self.mb * g * l * s - self.ma * g * (l * s - d * c),
                         -self.ma * d * v[..., 0] ** 2 + self.ma * g * s], -1)

    def phi(self, q):
        x = self.point_x(q)
        return np.stack([x + 0.5, 0.5 - x], -1)

    def J(self, q):
        Jd = self.point_jacobian(q)
        return np.concatenate([R1 @ Jd, -R1 @ Jd], axis=-2)


class WalledCartpolePlant(_WalledPlant):
    """q = (θ, x, xw1, xw2); the tip (x - l sinθ, l cosθ) between walls at -w + xw1 and w + xw2 (model.jl:42-68, 101-117)."""
    nq, nu, nw = 4, 1, 4
    mu_world = 0.1
    mb, mt, mw, l, lc, w, k = 0.978, 0.411, 0.1, 0.6, 0.4267, 0.35, 50.0
    joint_friction = (0.0, 1.0, 3.0, 3.0)
    B = np.array([[0.0, 1.0, 0.0, 0.0]])

    def tip_x(self, q):
        return q[..., 1] - self.l * np.sin(q[..., 0])

    def tip_jacobian(self, q):                       # _jacobian, mode = :tip (:58-60)
        s, c = np.sin(q[..., 0]), np.cos(q[..., 0])
        o, n = np.ones_like(s), np.zeros_like(s)
        return np.stack([np.stack([-self.l * c, o, n, n], -1), np.stack([-self.l * s, n, n, n], -1)], -2)

    def M(self, q):                                  # ∂²L/∂q̇² of the Lagrangian (:75-99)
        c = np.cos(q[..., 0])
        o, n = np.ones_like(c), np.zeros_like(c)
        a = -self.mt * self.lc * c
        return np.stack([np.stack([self.mt * self.lc ** 2 * o, a, n, n], -1), np.stack([a, (self.mt + self.mb) * o, n, n], -1),
                         np.stack([n, n, self.mw * o, n], -1), np.stack([n, n, n, self.mw * o], -1)], -2)

    def C(self, q, v):
        s = np.sin(q[..., 0])
        return np.stack([-self.mt * self.g * self.lc * s, self.mt * self.lc * v[..., 0] ** 2 * s, 2.0 * self.k * q[..., 2],
                         2.0 * self.k * q[..., 3]], -1)

    def phi(self, q):
        x = self.tip_x(q)
        return np.stack([x - q[..., 2] + self.w, self.w + q[..., 3] - x], -1)

    def J(self, q):
        Jt = self.tip_jacobian(q)
        e = lambda i: np.array([[1.0 if j == i else 0.0 for j in range(4)], [0.0] * 4])
        return np.concatenate([R1 @ (Jt - e(2)), -R1 @ (Jt - e(3))], axis=-2)


H_STEP = 0.02                                   # the step tests' time step
PLANTS = {"pushbot": PushBotPlant, "walledcartpole": WalledCartpolePlant}


def step_inputs(model: str, seed: int = 0, B: int = 64, h: float = 0.02, disturbed: bool = False):
    """The inputs of the step tests: B states around the walls, some of them starting inside one.
    pushbot: θ ~ U(-0.4, 0.4), tip x ~ U(-0.52, 0.52), d = (x + l sinθ) / cosθ; walledcartpole: θ ~ U(-0.7, 0.7), x ~ U(-0.1, 0.1),
    xw ~ U(-0.01, 0.01); v ~ U(-1, 1), q0 = q1 - h v, u ~ U(-1, 1); disturbed: w ~ U(-5, 5) h on every coordinate, else None."""
    P = PLANTS[model]()
    rng = np.random.default_rng(seed)
    if model == "pushbot":
        th, x = rng.uniform(-0.4, 0.4, B), rng.uniform(-0.52, 0.52, B)
        q1 = np.stack([th, (x + P.l * np.sin(th)) / np.cos(th)], -1)
    else:
        q1 = np.stack([rng.uniform(-0.7, 0.7, B), rng.uniform(-0.1, 0.1, B), rng.uniform(-0.01, 0.01, B), rng.uniform(-0.01, 0.01, B)], -1)
    v = rng.uniform(-1.0, 1.0, (B, P.nq))
    u = rng.uniform(-1.0, 1.0, (B, P.nu))
    w = rng.uniform(-5.0, 5.0, (B, P.nw)) * h if disturbed else None
    return q1 - h * v, q1, u, w


def cpu_steps(model: str, q0, q1, u, w, mu, h):
    """`oracle.plant.plant_step` per state: (status, q2, γ, b, iterations) as arrays."""
    P = PLANTS[model]()
    out = [pl.plant_step(P, q0[i], q1[i], u[i], np.zeros(P.nw) if w is None else w[i], mu, h, pl.SIM_OPTS) for i in range(len(q0))]
    return (np.array([o[0] for o in out]), np.array([o[2] for o in out]), np.array([o[3] for o in out]), np.array([o[4] for o in out]),
            np.array([o[1] for o in out]))


@functools.lru_cache(maxsize=None)
def cpu_step_case(model: str, disturbed: bool):
    """The CPU side of the step tests, solved once per process: `cpu_steps` on `step_inputs(model, 0, 64, H_STEP, disturbed)` with the
    model's μ_world."""
    q0, q1, u, w = step_inputs(model, 0, 64, H_STEP, disturbed)
    return cpu_steps(model, q0, q1, u, w, PLANTS[model].mu_world, H_STEP)
