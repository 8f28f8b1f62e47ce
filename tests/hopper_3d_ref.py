"""NumPy restatement of hopper_3D (src/dynamics/hopper_3D/model.jl) for the plant tests: the residual of
plant_residual_hopper_3d (contactimplicitmpc/jl_amd/csrc/plant_model.h) written from the model file, on flat ground or on a 3-D
surface of tests/terrain_ref.py, on complex input, so the oracle's complex-step Jacobian is exact to round-off and
`oracle.plant.plant_step` drives it.  The contact Jacobian J = dk/dq (ForwardDiff in the reference, model.jl:70-73) is written
in matrix form, dR/dp_j = (8 (S E_j + E_j S) - 8 p_j S + 4 (1 - |p|²) E_j) / (1 + |p|²)² - 4 p_j (R - I) / (1 + |p|²) with
E_j = skew(e_j): another route than the header's componentwise one; tests/test_hopper_3d.py holds both against torch's jacfwd."""
import numpy as np

from oracle import plant as pl
from oracle.dims import Dims
import terrain_ref as tr

_E = np.zeros((3, 3, 3))
for _j, (_a, _b) in enumerate(((1, 2), (2, 0), (0, 1))):            # skew(e_j)
    _E[_j, _b, _a], _E[_j, _a, _b] = 1.0, -1.0


def mrp(p):
    """R = I + (8 S² + 4 (1 - |p|²) S) / (1 + |p|²)², S = skew(p); p (..., 3) -> (..., 3, 3)."""
    n = np.sum(p * p, axis=-1)[..., None, None]
    S = tr._skew(p)
    return np.eye(3) + (8.0 * (S @ S) + 4.0 * (1.0 - n) * S) / (1.0 + n) ** 2


def mrp_derivative(p):
    """dR/dp_j, (..., 3 [j], 3, 3)."""
    n = np.sum(p * p, axis=-1)[..., None, None]
    S, R = tr._skew(p), mrp(p)
    out = []
    for j in range(3):
        pj = p[..., j][..., None, None]
        out.append((8.0 * (S @ _E[j] + _E[j] @ S) - 8.0 * pj * S + 4.0 * (1.0 - n) * _E[j]) / (1.0 + n) ** 2
                   - 4.0 * pj * (R - np.eye(3)) / (1.0 + n))
    return np.stack(out, axis=-3)


class Hopper3DPlant:
    """hopper_3D on `terrain` (a 3-D name of terrain_ref.SURFACES; None = flat_3D_lc, surface rotation = identity)."""
    nq, nu, nw, nc, nb = 7, 3, 3, 1, 4
    g = 9.81
    mu_world = 1.5
    mb, ml, Jb, Jl = 3.0, 0.3, 0.75, 0.075
    transpose = False                 # True: R^T in the place of R (the convention the gait files rule out)
    jacobian_z = pl.PlanarChainPlant.jacobian_z

    def __init__(self, terrain=None):
        self.Md = np.array([self.mb + self.ml] * 3 + [self.Jb + self.Jl] * 3 + [self.ml])
        self.dims = Dims(nq=7, nu=3, nw=3, nc=1, nb=4)
        self.terrain = terrain
        if terrain is not None:
            self.surf, self.grad, is3 = tr.SURFACES[terrain]
            assert is3

    def rot(self, p):
        R = mrp(p)
        return np.swapaxes(R, -1, -2) if self.transpose else R

    def foot(self, q):                                  # kinematics, model.jl:33-37
        return q[..., 0:3] - self.rot(q[..., 3:6])[..., :, 2] * q[..., 6:7]

    def foot_jacobian(self, q):                         # (..., 3, 7)
        dR = mrp_derivative(q[..., 3:6])
        dR = np.swapaxes(dR, -1, -2) if self.transpose else dR
        da = np.swapaxes(dR[..., :, :, 2], -1, -2)      # da_i / dp_j
        a = self.rot(q[..., 3:6])[..., :, 2]
        eye = np.broadcast_to(np.eye(3), da.shape).astype(da.dtype)
        return np.concatenate([eye, -q[..., 6:7, None] * da, -a[..., None]], axis=-1)

    def residual(self, z, th, kappa):
        (q0, q1, u1, w1, mu, h), (q2, gam, b, psi, s1, eta, s2) = tr._unpack(self, z, th)
        vm1, qm2, vm2 = (q1 - q0) / h, 0.5 * (q1 + q2), (q2 - q1) / h
        grav = np.zeros_like(q2); grav[..., 2] = -self.Md[2] * self.g
        Rm = self.rot(qm2[..., 3:6])
        Bu = np.concatenate([Rm[..., :, 2] * u1[..., 2:3], Rm[..., :, 0] * u1[..., 0:1] + Rm[..., :, 1] * u1[..., 1:2], u1[..., 2:3]], axis=-1)
        Aw = np.concatenate([w1, np.zeros(w1.shape[:-1] + (4,), dtype=w1.dtype)], axis=-1)
        k, J = self.foot(q2), self.foot_jacobian(q2)
        f = np.stack([b[..., 0] - b[..., 2], b[..., 1] - b[..., 3], gam[..., 0]], axis=-1)
        v = np.einsum("...in,...n->...i", J, vm2)
        if self.terrain is None:
            phi = k[..., 2:3]
        else:
            gx, gy = self.grad(k[..., 0], k[..., 1])
            Rs = tr.rotation_3d(gx + 0.0 * k[..., 0], gy + 0.0 * k[..., 0])
            f = np.einsum("...ji,...j->...i", Rs, f)
            v = np.einsum("...ij,...j->...i", Rs, v)
            phi = k[..., 2:3] - self.surf(k[..., 0], k[..., 1])[..., None]
        dyn = 0.5 * h * grav + self.Md * vm1 + 0.5 * h * grav - self.Md * vm2 + Bu + Aw + np.einsum("...in,...i->...n", J, f)
        vstack = np.stack([v[..., 0], v[..., 1], -v[..., 0], -v[..., 1]], axis=-1)
        return np.concatenate([dyn] + tr._tail(gam, b, psi, s1, eta, s2, mu, phi, vstack, 4, kappa), axis=-1)


class Hopper3DTransposedPlant(Hopper3DPlant):
    transpose = True
