"""NumPy restatement of centroidal_quadruped_box and centroidal_quadruped_wall (src/dynamics/centroidal_quadruped_box/model.jl,
src/dynamics/centroidal_quadruped_wall/model.jl) for the plant tests: the residual of plant_residual_centroidal_env
(contactimplicitmpc/jl_amd/csrc/plant_model.h) written from the model files, on complex input, so the oracle's complex-step
Jacobian is exact to round-off.  Both reference files define only the damped model; damped=False is the variant the box gait
was produced with (tests/test_centroidal_wall_box.py)."""
import numpy as np

from oracle import plant as pl
from oracle.dims import Dims

WALL_X = 0.25


def elevation(x):
    """e(x) = 0.2 (1 + tanh(200 (x - 0.25))) / 2, centroidal_quadruped_box/model.jl:101-106."""
    return 0.2 * (1.0 + np.tanh(200.0 * (x - 0.25))) / 2.0


class _EnvPlant(pl.CentroidalPlant):
    kind = ""

    def __init__(self, damped=True):
        super().__init__(damped)
        self.dims = Dims(nq=self.nq, nu=self.nu, nw=self.nw, nc=self.nc, nb=self.nb)

    def residual(self, z, th, kappa):
        nq, nu, nc, nb = self.nq, self.nu, self.nc, self.nb
        ot = np.cumsum([0, nq, nq, nu, self.nw, 1, 1])
        q0, q1, u1, w1, mu, h = (th[..., ot[i]:ot[i + 1]] for i in range(6))
        o = np.cumsum([0, nq, nc, nb, nc, nc, nb, nc])
        q2, gam, b, psi, s1, eta, s2 = (z[..., o[i]:o[i + 1]] for i in range(7))
        vm1, qm2, vm2 = (q1 - q0) / h, 0.5 * (q1 + q2), (q2 - q1) / h
        a1, b1 = self.lagrangian_derivatives(vm1)
        a2, b2 = self.lagrangian_derivatives(vm2)
        dyn = 0.5 * h * a1 + b1 + 0.5 * h * a2 - b2 - h * self.joint_friction * vm2
        R = self.rotation(qm2[..., 3:6])
        dyn = dyn + 0                                   # copy (complex-safe)
        dyn[..., 0:3] += w1
        phi, vs = [], []
        for c in range(nc):
            f = c % 4
            p2, p1 = q2[..., 6 + 3 * f:9 + 3 * f], q1[..., 6 + 3 * f:9 + 3 * f]
            v = (p2 - p1) / h
            mb = np.stack([b[..., 4 * c] - b[..., 4 * c + 2], b[..., 4 * c + 1] - b[..., 4 * c + 3]], axis=-1)
            if c < 4:                                   # floor: [m b; γ], v_T = (v_x, v_y)
                force = np.concatenate([mb, gam[..., c:c + 1]], axis=-1)
                phi.append(p2[..., 2] - (elevation(p2[..., 0]) if self.kind == "box" else 0.0))
                vt = v[..., 0:2]
            else:                                       # wall: [-γ; m b], v_T = (v_y, v_z)
                force = np.concatenate([-gam[..., c:c + 1], mb], axis=-1)
                phi.append(WALL_X - p2[..., 0])
                vt = v[..., 1:3]
            dyn[..., 6 + 3 * f:9 + 3 * f] += force
            vs.append(np.stack([vt[..., 0], vt[..., 1], -vt[..., 0], -vt[..., 1]], axis=-1))
        for f in range(4):                              # B(qm2)^T u
            uf = u1[..., 3 * f:3 * f + 3]
            rf = qm2[..., 6 + 3 * f:9 + 3 * f] - qm2[..., 0:3]
            dyn[..., 0:3] += uf
            dyn[..., 3:6] += np.einsum("...ji,...j->...i", R, np.cross(rf, uf))
            dyn[..., 6 + 3 * f:9 + 3 * f] -= uf
        phi = np.stack(phi, axis=-1)
        Eb = np.stack([b[..., 4 * c:4 * c + 4].sum(axis=-1) for c in range(nc)], axis=-1)
        return np.concatenate([dyn, s1 - phi, eta - np.concatenate(vs, axis=-1) - np.repeat(psi, 4, axis=-1), s2 - (mu * gam - Eb),
                               gam * s1 - kappa, b * eta - kappa, psi * s2 - kappa], axis=-1)


class BoxPlant(_EnvPlant):
    """centroidal_quadruped_box: nc 4, 0.5 kg feet, ϕ_i = p_z,i - e(p_x,i), vertical normal."""
    kind, nc, nb = "box", 4, 16
    mass_foot = 0.5


class WallPlant(_EnvPlant):
    """centroidal_quadruped_wall: nc 8, contacts 5-8 the feet against x = 0.25."""
    kind, nc, nb = "wall", 8, 32


PLANTS = {"centroidal_quadruped_box": BoxPlant, "centroidal_quadruped_wall": WallPlant}
