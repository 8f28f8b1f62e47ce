"""Seeded inputs of the per-knot interior-point seam tests (tests/test_ip_seam.py without a device, tests/test_gpu_ip_seam.py on one),
each with its longdouble answer (tests/ip_seam_ref.py) and the distance `d_ref` of the float64 restatement (oracle/lcp.py: the device's
algorithm) to that answer.  Every bound of a device figure is built from `d_ref`, so from the references alone.

Part 1, the B2 seam (`cimpc_ip_residual`, `cimpc_ip_linear_solve`): `seam_case(source, row)`.  source "synth": knot KNOT of
`common.make_case(row, 0, H_ref=3, seed=SEED)`; source "real": knot REAL_KNOT of `real_problems.real_problem(row, 1e-3)`, the knot
tests/test_gpu_round3_parity.py uses.  The operators do not depend on the mode, so one set of points and answers serves both modes.
Part 2, the sensitivities of `implicit_dynamics`: `sens_case(model, mode, H)`."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import ip as oip, lcp

import ip_seam_ref as ref
from common import make_case, oracle_sweep

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = ("pushbot", "hopper", "quadruped", "flamingo", "centroidal", "hopper3d", "walledcartpole", "particle", "particle2d")   # rows with callbacks
REAL = ("quadruped", "flamingo", "centroidal")
SEAM = [("synth", r) for r in ROWS] + [("real", r) for r in REAL]
SEED, KNOT, REAL_KNOT, REAL_KAPPA = 11, 1, 4, 1e-3
# Seed of the points, right-hand sides and displacements: one under which every case holds the conditions of tests/test_ip_seam.py.  A seed
# that misses a condition is changed, never the condition.
POINT_SEED = 20
# d_ref of a linear-solve point: the float64 restatement's distance to the longdouble answer at the point and at N_NOISE copies of it with
# every entry of (z, r) moved by one unit in the last place (each copy against the longdouble answer of ITS inputs), the largest of them.
# One float64 evaluation is a draw from the algorithm's round-off scatter, which is two to three decades wide on these systems; the
# largest of a few draws has no such lower tail, and comes from the references alone.
N_NOISE = 4
REG = 1e-5                      # the `reg` regime's regularisation
LATE_PRODUCT = 1e-8             # y1 y2 of every pair of a `late` point
REGIMES = (("near", 0.0), ("late", 0.0), ("reg", REG))


# ---- the lane-group width of a row, from model_table.h itself ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_table():
    """{row name: dict(dims=(nq, nu, nw, nc, nb), lanes, async)} as tests/native/model_table_check.cpp prints `model_lanes` and the rows
    of csrc/model_table.h (the way tests/test_model_table.py reads them), built once per session.  Without g++ there is no reading of the
    header and the cases cannot be made: that is an error, not a skip."""
    if shutil.which("g++") is None:
        raise RuntimeError("g++ is needed to read model_lanes from csrc/model_table.h (tests/native/model_table_check.cpp)")
    tmp = tempfile.mkdtemp(prefix="ip_seam_model_table_")
    try:
        exe = os.path.join(tmp, "model_table_check")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "model_table_check.cpp")])
        out = subprocess.run([exe], input="", capture_output=True, text=True, check=True).stdout.split("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rows = [line.split() for line in out if line.startswith("row ")]
    return {r[1]: dict(dims=tuple(int(v) for v in r[2:7]), lanes=int(r[7]), async_=int(r[8])) for r in rows}


def lanes_by_rule(m):
    """The rule model_table.h states for `model_lanes`, restated for tests/test_ip_seam.py to hold the header's figures against."""
    n = max(m["nq"], 2 * m["nc"] + m["nb"])
    return 16 if n <= 16 else 32 if n <= 32 else 64


def point_counts(ppw):
    """n of a call: 1, ppw - 1 (where that is at least 1), ppw, ppw + 1, 2 ppw + 1 - a lone point, a ragged and a full wavefront, a second
    workgroup with one live lane group, a third."""
    return sorted({n for n in (1, ppw - 1, ppw, ppw + 1, 2 * ppw + 1) if n >= 1})


# ---- part 1: the B2 seam ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def knot(source, row):
    """(Dims of mode 0, z0, th0, r0, rz0, rth0) of the case's knot."""
    if source == "synth":
        d, prob, _, _ = make_case(row, 0, H_ref=3, H=1, B=1, seed=SEED)
        t = KNOT
    else:
        from real_problems import real_problem
        d, _, prob, _ = real_problem(row, REAL_KAPPA)
        t = REAL_KNOT
    return d, prob["z0"][t].copy(), prob["th0"][t].copy(), prob["r0"][t].copy(), prob["rz0"][t].copy(), prob["rth0"][t].copy()


def _near(z0, rng):
    return np.abs(z0 * (1.0 + 0.05 * rng.standard_normal(z0.shape))) + 1e-3


def _late(d, z0, rng):
    """Late on the central path: per pair s = 10^U(-6, -2), one of (y1, y2) = s and the other LATE_PRODUCT / s, the side drawn per pair.
    So that every point serves the `reg` regime and shows both orientations whatever ny is (4 on the smallest rows), four draws are
    overwritten: two pairs get s outside [REG, LATE_PRODUCT / REG] (one y of each below REG), one pair gets s inside (both above),
    and two pairs get side 0 (y1 the smaller of the two) and side 1."""
    ny = d.ny
    e = rng.uniform(-6.0, -2.0, ny)
    k = rng.permutation(ny)
    e[k[0]] = rng.uniform(-6.0, -5.1)
    e[k[1]] = rng.uniform(-2.9, -2.0)
    e[k[2]] = rng.uniform(-4.9, -3.1)
    side = rng.integers(0, 2, ny)
    j = rng.permutation(ny)
    side[j[0]], side[j[1]] = 0, 1
    s = 10.0 ** e
    z = _near(z0, rng)
    lo, hi = np.minimum(s, LATE_PRODUCT / s), np.maximum(s, LATE_PRODUCT / s)
    z[d.iy1] = np.where(side == 0, lo, hi)          # side 0: y1 is the small one of the pair
    z[d.iy2] = np.where(side == 0, hi, lo)
    return z


def _d_once(tab, z, r, reg, ld):
    d = tab.dims
    lcp.rzlin(tab, z, reg)
    f64 = lcp.linear_solve_vec(tab, r[d.ix], r[d.iy1], r[d.iy2], reg)
    return ref.dist(f64, ld)


def _d_solve(tab, z, r, reg, ld, rng):
    """(d_ref, d_plain) of one point: the largest over the point and its N_NOISE last-place copies, and the point's own."""
    plain = _d_once(tab, z, r, reg, ld)
    best = plain
    for _ in range(N_NOISE):
        zp = z * (1.0 + (rng.integers(0, 2, z.shape) * 2 - 1) * 2.0 ** -52)
        rp = r * (1.0 + (rng.integers(0, 2, r.shape) * 2 - 1) * 2.0 ** -52)
        best = max(best, _d_once(tab, zp, rp, reg, ref.linear_solve_ld(tab, zp, rp, reg)))
    return best, plain


@functools.lru_cache(maxsize=None)
def seam_case(source, row):
    """dict(G, ppw, counts, n, tab, knot, solve = {regime: dict(z, r, reg, ld, d_ref, d_plain, cond)}, residual = [dict(name, z, th, kappa, alt,
    ld, d_ref)]): n = 2 ppw + 1 points per regime (a call of fewer takes the first ones); ld (n, nz) longdouble; d_ref (n,)."""
    d, z0, th0, r0, rz0, rth0 = knot(source, row)
    tab = lcp.LinTable(d, z0, th0, r0, rz0, rth0)
    G = model_table()[row]["lanes"]
    ppw = 64 // G
    n = 2 * ppw + 1
    rng = np.random.default_rng([POINT_SEED, SEAM.index((source, row))])
    pts = dict(near=np.stack([_near(z0, rng) for _ in range(n)]), late=np.stack([_late(d, z0, rng) for _ in range(n)]))
    pts["reg"] = pts["late"]
    rhs = np.stack([r0] + [rng.standard_normal(d.nz) for _ in range(n - 1)])
    solve = {}
    noise = np.random.default_rng([POINT_SEED, SEAM.index((source, row)), 1])
    for name, reg in REGIMES:
        z = pts[name]
        ld = np.stack([ref.linear_solve_ld(tab, z[k], rhs[k], reg) for k in range(n)])
        dd = np.array([_d_solve(tab, z[k], rhs[k], reg, ld[k], noise) for k in range(n)])
        solve[name] = dict(z=z, r=rhs, reg=reg, ld=ld, d_ref=dd[:, 0], d_plain=dd[:, 1],
                           cond=np.array([np.linalg.cond(ref.rz_reg(tab, z[k], reg).astype(np.float64)) for k in range(n)]))
    ths = th0[None] + 1e-2 * rng.standard_normal((n, d.nth))
    alts = 0.05 * rng.standard_normal((n, d.nc))
    residual = []
    for name, kappa, with_alt in (("near", 1e-3, True), ("near", 0.0, False), ("late", 1e-3, False), ("late", 0.0, True)):
        z = pts[name]
        alt = alts if with_alt else None
        ld = np.stack([ref.rlin_ld(tab, z[k], ths[k], kappa, None if alt is None else alt[k]) for k in range(n)])
        f64 = []
        for k in range(n):
            tab.alt = np.zeros(d.nc) if alt is None else alt[k].copy()
            f64.append(np.concatenate(lcp.rlin(tab, z[k], ths[k], kappa)))
        tab.alt = np.zeros(d.nc)
        residual.append(dict(name=f"{name}/kappa={kappa:g}/{'alt' if with_alt else 'no alt'}", z=z, th=ths, kappa=kappa, alt=alt, ld=ld,
                             d_ref=np.array([ref.dist(f64[k], ld[k]) for k in range(n)])))
    return dict(G=G, ppw=ppw, counts=point_counts(ppw), n=n, tab=tab, knot=(d, z0, th0, r0, rz0, rth0), solve=solve, residual=residual)


def one_knot_solver(source, row, mode):
    """One solver of H_ref = H = B = 1 holding the case's knot as knot 1 (tests/test_gpu_round3_parity.py: `_one_knot_solver`)."""
    from contactimplicitmpc.jl_amd import CIMPCSolver
    d, z0, th0, r0, rz0, rth0 = knot(source, row)
    s = CIMPCSolver(d.nq, d.nu, d.nw, d.nc, d.nb, 1, 1, B=1, mode=mode)
    s.set_linearization(1, z0, th0, r0, rz0, rth0)
    return s


# ---- part 2: the sensitivities of implicit_dynamics at a converged point -----------------------------------------------------------------
SENS_MODELS = ROWS + ("centroidal_wall", "anydims")      # the ten rows of model_table.h and a dimension set nothing was compiled for
SENS_H_REF = 4
# Interior-point options under which the regularisation of the sensitivity solve depends on the options alone.  kappa_reg = 0 (nothing
# validates it away): the iteration's reg = (k_vio < kappa_reg) ? k_vio gamma_reg : 0 is then 0 at every iteration (oracle/ip.py:82,
# ip_kernel_impl.h: `iterate`), and differentiate_solution! runs at max(0, kappa_tol gamma_reg) = SENS_REG exactly (oracle/ip.py:126-129,
# ip_kernel_impl.h: `reg_floor`), whatever path the iterate took.
SENS_KAPPA_TOL, SENS_GAMMA_REG, SENS_KAPPA_REG = 2e-4, 0.1, 0.0
SENS_REG = SENS_KAPPA_TOL * SENS_GAMMA_REG
SENS_CASES = [(m, mode, 3) for m in SENS_MODELS for mode in (0, 1)] + [("quadruped", 0, 5), ("hopper", 1, 5)]     # (model, mode, H); H = 5: B = 1 only
CLAMP_LIVE = ("quadruped", "centroidal", "centroidal_wall", "anydims")      # the smallest y of a converged point is below SENS_REG on these


def sens_oracle_opts():
    return oip.IPOptions(kappa_tol=SENS_KAPPA_TOL, gamma_reg=SENS_GAMMA_REG, kappa_reg=SENS_KAPPA_REG)


def sens_device_opts():
    from contactimplicitmpc.jl_amd import InteriorPointOptions
    return InteriorPointOptions(kappa_tol=SENS_KAPPA_TOL, gamma_reg=SENS_GAMMA_REG, kappa_reg=SENS_KAPPA_REG)


def sens_block(out):
    """The consumed block (nd, 2nq + nu) of one problem from its dq0, dq1, du1."""
    return np.concatenate([out["dq0"], out["dq1"], out["du1"]], axis=-1)


@functools.lru_cache(maxsize=None)
def sens_case(model, mode, H):
    """dict(d, prob, tabs, rollouts (2, or 1 for H = 5), trajs, oracle = [per rollout: the oracle's implicit_dynamics output],
    d_direct / d_adjoint = [per rollout: (H,) distances of lcp.linear_solve_mat / lcp.linear_solve_mat_x_adjoint to the longdouble
    block (rows 1:nd - the adjoint form: its x rows - against the q0, q1, u1 columns), AT THE ORACLE'S converged point],
    cond (rollouts, H))."""
    B = 2 if H == 3 else 1
    d, prob, tabs, rollouts = make_case(model, mode, H_ref=SENS_H_REF, H=H, B=B, seed=SEED, kappa=SENS_KAPPA_TOL)
    nq, nu, nd = d.nq, d.nu, d.nd
    outs = oracle_sweep(d, tabs, rollouts, sens_oracle_opts())
    d_direct, d_adjoint, cond = [], [], np.zeros((B, H))
    for b, (tr, o) in enumerate(outs):
        dd, da = np.zeros(H), np.zeros(H)
        for i in range(H):
            tab = tabs[int(rollouts[b][0][i])]
            z = o["z"][i]
            ld = sens_block(ref.sensitivities_ld(tab, z, SENS_REG, d))
            lcp.rzlin(tab, z, SENS_REG)
            dd[i] = ref.dist(-lcp.linear_solve_mat(tab, SENS_REG)[:nd, :2 * nq + nu], ld)
            da[i] = ref.dist(-lcp.linear_solve_mat_x_adjoint(tab, SENS_REG, ncols=2 * nq + nu), ld[:nq])      # stated for the x rows
            cond[b, i] = np.linalg.cond(ref.rz_reg(tab, z, SENS_REG).astype(np.float64))
        d_direct.append(dd); d_adjoint.append(da)
    return dict(d=d, prob=prob, tabs=tabs, rollouts=rollouts, trajs=[tr for tr, _ in outs], oracle=[o for _, o in outs],
                d_direct=d_direct, d_adjoint=d_adjoint, cond=cond)


def sens_bound(case, b, i):
    return ref.bound(max(case["d_direct"][b][i], case["d_adjoint"][b][i]))
