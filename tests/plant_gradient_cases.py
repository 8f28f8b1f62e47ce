"""Inputs and references of the step-gradient tests (tests/test_plant_gradients.py without a device, tests/test_gpu_plant_gradients.py
on it, scripts/plant_gradients_ab.py): the definition of csrc/plant_sensitivity.hip restated in NumPy,

    dz = -R(z, θ; reg)⁻¹ ∂r/∂θ[:, :n_cols],   rows [q2; γ; b],

where R is ∂r/∂z with the bilinear rows' two diagonals replaced by max(y2, reg) and max(y1, reg) (linearized_solver.jl:390-391,
434-435, restated in oracle/lcp.py:166-167), solved three ways: in longdouble (tests/gains_ref.solve_ld), by `numpy.linalg.solve`,
and by a float64 restatement of the kernel's own elimination order.  The Jacobians are the torch linearization of
contactimplicitmpc/jl_amd/lcp_models.py on flat ground and the complex step of the NumPy restatements on terrain, as in
tests/plant_linearize_cases.py.  Every reference is computed once per process and read-only."""
import functools
import os

import numpy as np

import gains_ref
import plant_linearize_cases as plc

HERE = os.path.dirname(os.path.abspath(__file__))
REG = 1e-9                      # SIM_OPTS.kappa_tol * SIM_OPTS.gamma_reg
FACTOR = 100.0                  # the margin the gain kernels were given (tests/gains_edge_cases.bound), without its 1e-9 cap
REF_LIMIT = 1e-6                # a step whose float64 references are further than this from the longdouble solve fails its test


def dims(model: str):
    """(nq, nu, nc, nb, nw, nz, nθ, nr) of a plant model."""
    from contactimplicitmpc.jl_amd import plant
    _, nq, nu, nc, fd, nw = plant.model_dims(model)
    nb = fd * nc
    return nq, nu, nc, nb, nw, nq + 4 * nc + 2 * nb, 2 * nq + nu + nw + 2, nq + nc + nb


def regularized(rz, z, nq: int, ny: int, reg: float):
    """R(z, θ; reg) from ∂r/∂z: row nq + ny + t is the bilinear row y1[t] y2[t], y1 = z[nq + t], y2 = z[nq + ny + t]."""
    R = np.array(rz, dtype=float)
    for t in range(ny):
        R[nq + ny + t, nq + t] = np.maximum(z[nq + ny + t], reg)
        R[nq + ny + t, nq + ny + t] = np.maximum(z[nq + t], reg)
    return R


def solve_kernel_order(R, rhs):
    """R \\ rhs in float64 in the order of plant_sensitivity_kernel: the augmented matrix [R | rhs] eliminated row by row with the
    FIRST largest |entry| of a column as its pivot, multipliers by division, every update one product and one difference (no fused
    multiply-add), then the back substitution from the last row up, each entry losing its terms in the order k = n - 1, n - 2, ..."""
    n = len(R)
    W = np.concatenate([np.array(R, dtype=float), np.array(rhs, dtype=float).reshape(n, -1)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(W[k:, k])))
        if p != k:
            W[[k, p], k:] = W[[p, k], k:]
        pv = W[k, k]
        if not (np.isfinite(pv) and abs(pv) > 0):
            raise np.linalg.LinAlgError(f"zero or non-finite pivot at column {k}")
        l = W[k + 1:, k] / pv
        W[k + 1:, k + 1:] -= l[:, None] * W[k, k + 1:][None, :]
    X = W[:, n:]
    for k in range(n - 1, -1, -1):
        X[k] = X[k] / W[k, k]
        X[:k] -= W[:k, k][:, None] * X[k][None, :]
    return X


def rel(a, ref):
    ref = np.asarray(ref)
    return float(np.abs(np.asarray(a, dtype=gains_ref.LD) - ref).max() / np.abs(ref).max())


def references(model: str, rz, rth, z, reg: float, n_cols: int):
    """dict(ld (nr, n_cols) longdouble, d_lapack, d_order, bound, cond) of one knot from its float64 Jacobians."""
    nq, nu, nc, nb, nw, nz, nth, nr = dims(model)
    R = regularized(rz, z, nq, 2 * nc + nb, reg)
    rhs = -np.asarray(rth, dtype=float)[:, :n_cols]
    ld = gains_ref.solve_ld(R, rhs)[:nr]
    d_lapack = rel(np.linalg.solve(R, rhs)[:nr], ld)
    d_order = rel(solve_kernel_order(R, rhs)[:nr], ld)
    return dict(ld=ld, d_lapack=d_lapack, d_order=d_order, bound=FACTOR * max(d_lapack, d_order, 2.2e-16), cond=float(np.linalg.cond(R)))


def jacobians(model: str, terrain, z, th):
    """(∂r/∂z, ∂r/∂θ) in float64 of one knot (1-D z) or of N knots in one evaluation: torch on flat ground, the complex step of the
    restatement on a terrain."""
    z, th = np.array(z, dtype=float), np.array(th, dtype=float)
    if z.ndim == 1:
        rz, rth = jacobians(model, terrain, z[None], th[None])
        return rz[0], rth[0]
    if terrain is None:
        _, rz, rth = _torch_model(model).linearize_batch(z, th, 0.0)
        return np.asarray(rz), np.asarray(rth)
    lin = [plc.complex_step(_restatement(model, terrain), z[k], th[k], 0.0) for k in range(len(z))]
    return np.stack([l[1] for l in lin]), np.stack([l[2] for l in lin])


@functools.lru_cache(maxsize=None)
def _torch_model(model: str):
    from contactimplicitmpc.jl_amd import lcp_models
    return lcp_models.MODELS[model]()


@functools.lru_cache(maxsize=None)
def _restatement(model: str, terrain: str):
    return plc.restatement(model, terrain)


def knot_references(model: str, terrain, z, th, reg: float, n_cols: int):
    rz, rth = jacobians(model, terrain, z, th)
    return references(model, rz, rth, z, reg, n_cols)


# ---- synthetic knots: the inputs of tests/plant_linearize_cases.py, N = 3 ----------------------------------------------------------------
N_KNOTS = 3
FLAT_CASES = tuple((name, mid) for mid, name in sorted(plc.TORCH_MODELS.items()))      # the eleven flat models
REGS = (0.0, REG)


@functools.lru_cache(maxsize=None)
def flat_case(mid: int, reg: float):
    """(z, θ, [references per knot]) of flat model `mid`, every column of θ."""
    name = plc.TORCH_MODELS[mid]
    z, th, (_, rz, rth) = plc.torch_case(mid, N_KNOTS)
    nth = th.shape[1]
    return z, th, [references(name, rz[k], rth[k], z[k], reg, nth) for k in range(N_KNOTS)]


@functools.lru_cache(maxsize=None)
def terrain_case(model: str, mid: int, terrain: str, reg: float):
    z, th, lin = plc.terrain_case(model, mid, terrain, N_KNOTS)
    nth = th.shape[1]
    return z, th, [references(model, lin[k][1], lin[k][2], z[k], reg, nth) for k in range(N_KNOTS)]


# ---- rollouts ------------------------------------------------------------------------------------------------------------------------------
def _gait(name):
    from contactimplicitmpc.jl_amd import gait_io
    return gait_io.load_gait(os.path.join(HERE, "golden", "gaits", name))


@functools.lru_cache(maxsize=None)
def rollout_case(which: str):
    """dict(model, terrain, q1 (B, nq), v1, u (K, B, nu) nominal controls (N_sample = 1), mu (B,), h, T) of a rollout case.
    hopper_2D: three hoppers dropped from 3 cm with different friction and leg forces - four steps of flight, the impact, contact under a
    light leg force and, from step 8, under a push that takes the normal impulse above 1;
    particle: released 1 cm above the side of quadratic_bowl_3D_lc (z = x² + y², a 47° slope there), where it lands and slides; quadruped and centroidal_quadruped_wall: the
    shipped gaits' first knots under the gaits' own controls."""
    if which == "hopper_2D":
        B, T, h = 3, 14, 0.01
        q1 = np.tile(np.array([0.0, 0.5 * np.cos(0.1) + 0.03, 0.1, 0.5]), (B, 1))
        v1 = np.tile(np.array([0.3, 0.0, 0.0, 0.0]), (B, 1))
        push = np.array([[0.0, 5.0], [0.0, 4.0], [0.02, 6.0]])                       # applied as they stand (N_sample = 1): impulses per step
        u = np.stack([push * (0.01 if t < 8 else 1.0) for t in range(T)])           # a light leg force through flight and landing, then the push
        return dict(model="hopper_2D", terrain=None, q1=q1, v1=v1, u=u, mu=np.array([0.8, 0.3, 0.05]), h=h, T=T)
    if which == "particle":
        T, h = 14, 0.01
        return dict(model="particle", terrain="quadratic_bowl_3D_lc", q1=np.array([[0.5, 0.2, 0.29 + 0.01]]), v1=np.array([[0.0, 0.0, 0.0]]),
                    u=np.zeros((T, 1, 3)), mu=np.array([0.5]), h=h, T=T)
    if which == "quadruped":
        g, T = _gait("quadruped_gait2.jld2"), 6
        k = np.array([0, g.H // 2])
        u = np.stack([g.u[(k + t) % g.H] for t in range(T)])
        return dict(model="quadruped", terrain=None, q1=g.q[k + 1], v1=(g.q[k + 1] - g.q[k]) / g.h, u=u, mu=np.array([g.mu, 0.6 * g.mu]), h=g.h, T=T)
    if which == "centroidal_quadruped_wall":
        g, T = _gait("wall_stand_FL_4.jld2"), 2
        k = np.array([g.H // 2])
        u = np.stack([g.u[(k + t) % g.H] for t in range(T)])
        return dict(model="centroidal_quadruped_wall", terrain=None, q1=g.q[k + 1], v1=(g.q[k + 1] - g.q[k]) / g.h, u=u, mu=np.array([g.mu]), h=g.h, T=T)
    raise KeyError(which)


ROLLOUTS = ("hopper_2D", "particle", "quadruped", "centroidal_quadruped_wall")


def step_theta(case, q, u_applied, t: int, b: int):
    """θ = [q0; q1; u1; w1; μ; h] of step t of robot b, from a rollout's trajectory q (T + 2, B, nq) and applied controls."""
    nw = dims(case["model"])[4]
    return np.concatenate([q[t, b], q[t + 1, b], u_applied[t, b], np.zeros(nw), [case["mu"][b]], [case["h"]]])


def cpu_plant(case):
    """The CPU restatement that steps a rollout case (oracle/plant.py and the restatements under tests/)."""
    from oracle import plant as pl
    if case["model"] == "hopper_2D":
        return pl.HopperPlant()
    if case["model"] == "quadruped":
        return pl.QuadrupedPlant()
    if case["model"] == "particle":
        import terrain_ref
        return terrain_ref.plant("particle", case["terrain"])
    import centroidal_wall_box_ref
    return centroidal_wall_box_ref.PLANTS[case["model"]]()


def cpu_step_z(P, q0, q1, u, w, mu, h, opts):
    """oracle.plant.plant_step (the same statements), returning the whole converged z: (status, z, θ)."""
    from oracle import ip as oip
    d = P.dims
    iy1, iy2 = d.iy1, d.iy2
    th = np.concatenate([q0, q1, u, w, [mu], [h]])
    z = np.ones(d.nz)
    z[:d.nq] = q1

    def viol(r):
        return float(np.abs(r[:d.nq + d.ny]).max()), float(np.abs(r[d.nq + d.ny:]).max())

    r = P.residual(z, th, 0.0)
    r_vio, k_vio = viol(r)
    for _ in range(opts.max_iter):
        if r_vio < opts.r_tol and k_vio < opts.kappa_tol:
            break
        rz = P.jacobian_z(z, th)
        D = np.linalg.solve(rz, r)
        a_aff = oip.step_length(z[iy1], z[iy2], D[iy1], D[iy2], 1.0)
        mu_c, sigma = oip.centering(z[iy1], z[iy2], D[iy1], D[iy2], a_aff)
        kc = max(sigma * mu_c, opts.kappa_tol / opts.undercut)
        rc = P.residual(z, th, kc)
        rc[iy2] += D[iy1] * D[iy2]
        D = np.linalg.solve(rz, rc)
        tau = max(1.0 - opts.eps_min, 1.0 - max(r_vio, k_vio) ** 2)
        alpha = oip.step_length(z[iy1], z[iy2], D[iy1], D[iy2], tau)
        if alpha < opts.stall_alpha:
            break
        z = z - alpha * D
        for i in range(1, opts.max_ls + 1):
            r = P.residual(z, th, 0.0)
            r_c, k_c = viol(r)
            if r_c <= r_vio or k_c <= k_vio:
                break
            z = z + alpha * opts.ls_scale ** i * D
        r_vio, k_vio = r_c, k_c
    return bool(r_vio < opts.r_tol and k_vio < opts.kappa_tol), z, th


@functools.lru_cache(maxsize=None)
def cpu_rollout(which: str):
    """The rollout case stepped on the CPU: (status (T, B), z (T, B, nz), θ (T, B, nθ))."""
    from oracle import plant as pl
    c = rollout_case(which)
    P = cpu_plant(c)
    nq, nu, nc, nb, nw, nz, nth, nr = dims(c["model"])
    B, T, h = c["q1"].shape[0], c["T"], c["h"]
    st, Z, TH = np.zeros((T, B), dtype=bool), np.zeros((T, B, nz)), np.zeros((T, B, nth))
    for b in range(B):
        q0, q1 = c["q1"][b] - h * c["v1"][b], c["q1"][b].copy()
        for t in range(T):
            st[t, b], Z[t, b], TH[t, b] = cpu_step_z(P, q0, q1, c["u"][t, b if c["u"].shape[1] > 1 else 0], np.zeros(nw), c["mu"][b], h, pl.SIM_OPTS)
            q0, q1 = q1, Z[t, b, :nq].copy()
    for a in (st, Z, TH):
        a.setflags(write=False)
    return st, Z, TH


def rollout_references(case, Z, TH, reg: float, n_cols: int):
    """`references` of every step of a rollout from its z (T, B, nz) and θ (T, B, nθ): an object array (T, B) of dicts."""
    T, B = Z.shape[:2]
    rz, rth = jacobians(case["model"], case["terrain"], Z.reshape(T * B, -1), TH.reshape(T * B, -1))
    out = np.empty((T, B), dtype=object)
    for t in range(T):
        for b in range(B):
            out[t, b] = references(case["model"], rz[t * B + b], rth[t * B + b], Z[t, b], reg, n_cols)
    return out
