"""The feedback gains on the device (csrc/gains.hip: gains_dynamics_kernel, tvlqr_kernel, gain_latch_kernel, gain_feedback_kernel)
against the NumPy restatement of gains.jl (tests/gains_ref.py) on the shipped gaits of the 3-D cone models (tests/gains_cases.py), the
bit identities between the entries, the singular returns, and the policy that applies the gains.

Tolerance of the parity checks: max|K_dev - K_ref| <= 1e-9 max|K_ref|, the same for P1.  The restatement itself moves by at most
6.5e-12 of max|K| under last-place noise on every entry of rz0, rθ0 (centroidal trot 1.6e-12, wall stand 1.2e-13, hopper_3D 4.5e-12),
the direct and the adjoint solve order differ by 7e-13: 1e-9 is 150 x that and five orders below any real defect."""
import os

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import InteriorPointOptions, NewtonOptions, _lib, gains, gait_io, lcp_models, plant
from contactimplicitmpc.jl_amd.policy import CIMPCPolicy
import gains_cases as gc
import gains_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGULAR, STATE = -5, -3


def _rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


# ---- parity with the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_gains_match_the_numpy_restatement(name):
    c = gc.case(name)
    m = c["model"]
    K_lin, P_lin = gains.reference_gains_lin(m.nq, m.nu, c["rz0"], c["rth0"], *c["weights"], N=c["N"], return_P1=True)
    K_dev, P_dev = gains.reference_gains(m.name, c["z"], c["theta"], *c["weights"], N=c["N"], return_P1=True)
    figures = dict(K_lin=_rel(K_lin, c["K"]), P1_lin=_rel(P_lin, c["P1"]), K_dev=_rel(K_dev, c["K"]), P1_dev=_rel(P_dev, c["P1"]))
    print(f"{name}: max|dev - ref| / max|ref| = {figures}")
    assert K_lin.shape == c["K"].shape == (c["z"].shape[0], m.nu, 2 * m.nq)
    for what, v in figures.items():
        assert v <= gc.TOL, f"{name}: {what} differs by {v:.3e} of its scale"


# ---- identities between the entries --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terrain", [None, "per knot"])
def test_device_linearized_entry_is_linearize_then_lin_bit_for_bit(terrain):
    c = gc.case("hopper_3D in place, knots 1-5, N = 3")
    m, n = c["model"], c["z"].shape[0]
    ter = None if terrain is None else ["flat_3D_lc", "sine1_3D_lc", "sine2_3D_lc", "sine3_3D_lc", "quadratic_bowl_3D_lc"][:n]
    _, rz0, rth0 = plant.linearize(m.name, c["z"], c["theta"], gc.KAPPA, terrain=ter)
    K_a, P_a = gains.reference_gains_lin(m.nq, m.nu, rz0, rth0, *c["weights"], N=c["N"], return_P1=True)
    K_b, P_b = gains.reference_gains(m.name, c["z"], c["theta"], *c["weights"], N=c["N"], terrain=ter, return_P1=True)
    assert np.isfinite(K_a).all() and np.abs(K_a).max() > 0
    assert np.array_equal(K_a, K_b) and np.array_equal(P_a, P_b)
    if terrain is not None:      # the terrains did reach the kernel
        assert not np.array_equal(K_b, gains.reference_gains(m.name, c["z"], c["theta"], *c["weights"], N=c["N"]))


def _random_problems(n_prob, n, m, T, n_ab, seed, varying=False):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n_prob, n_ab, n, n)) / np.sqrt(n)
    B = rng.standard_normal((n_prob, n_ab, n, m))
    spd = lambda k, c: (lambda X: X @ np.swapaxes(X, -1, -2) + np.eye(k))(rng.standard_normal((n_prob, c, k, k)))
    Q, R = spd(n, T if varying else 1), spd(m, T - 1)
    return A, B, Q, R


def _ref_tvlqr(A, B, Q, R, T):
    K, P = gains_ref.tvlqr([A[t % len(A)] for t in range(T - 1)], [B[t % len(B)] for t in range(T - 1)],
                           [Q[t % len(Q)] for t in range(T)], [R[t % len(R)] for t in range(T - 1)])
    return np.stack(K), P[0]


def test_a_batch_of_problems_equals_single_calls_bit_for_bit():
    n, m, T, n_ab = 13, 5, 9, 3
    A, B, Q, R = _random_problems(3, n, m, T, n_ab, seed=4)
    K, P1 = gains.tvlqr(A, B, Q, R)
    assert K.shape == (3, T - 1, m, n) and P1.shape == (3, n, n)
    for p in range(3):
        Kp, Pp = gains.tvlqr(A[p], B[p], Q[p], R[p])
        assert np.array_equal(K[p], Kp) and np.array_equal(P1[p], Pp)
        Kr, Pr = _ref_tvlqr(A[p], B[p], Q[p], R[p], T)
        assert _rel(Kp, Kr) <= gc.TOL and _rel(Pp, Pr) <= gc.TOL
    assert not np.array_equal(K[0], K[1])


def test_time_varying_weights_and_the_largest_size():
    """n_q = T, n_r = T - 1; n = 48, m = 16 is the largest size the kernel takes."""
    n, m, T, n_ab = 48, 16, 6, 5
    A, B, Q, R = _random_problems(1, n, m, T, n_ab, seed=5, varying=True)
    K, P1 = gains.tvlqr(A[0], B[0], Q[0], R[0])
    Kr, Pr = _ref_tvlqr(A[0], B[0], Q[0], R[0], T)
    f = (_rel(K, Kr), _rel(P1, Pr))
    print(f"time-varying weights, n = {n}, m = {m}: max|dev - ref| / max|ref| = K {f[0]:.3e}, P1 {f[1]:.3e}")
    assert max(f) <= gc.TOL


def test_n_keep_returns_the_leading_steps():
    n, m, T, n_ab = 6, 2, 12, 4
    A, B, Q, R = _random_problems(1, n, m, T, n_ab, seed=6)
    K, P1 = gains.tvlqr(A[0], B[0], Q[0], R[0])
    Kk, Pk = gains.tvlqr(A[0], B[0], Q[0], R[0], n_keep=3)
    assert Kk.shape == (3, m, n) and np.array_equal(Kk, K[:3]) and np.array_equal(Pk, P1)


# ---- singular input is an error return -----------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(_lib._dp)


def test_singular_rz_names_the_knot_and_leaves_k_untouched():
    c = gc.case("centroidal trot, knots 1-4, N = 2")
    m = c["model"]
    rz0 = c["rz0"][:3].copy()
    rz0[1][:, 20] = 0.0          # stays exactly zero under any row elimination: every pivoting order meets a zero pivot
    with pytest.raises(np.linalg.LinAlgError):
        gains_ref.reference_gains(m.nq, m.nu, rz0, c["rth0"][:3], *c["weights"], N=2)
    lib = _lib.load()
    rzc = np.ascontiguousarray(rz0.transpose(0, 2, 1))
    rthc = np.ascontiguousarray(c["rth0"][:3].transpose(0, 2, 1))
    Qq, Qv, Ru = (np.ascontiguousarray(w.T) for w in c["weights"])
    K, P1 = np.full((3, 2 * m.nq, m.nu), 7.0), np.full((2 * m.nq, 2 * m.nq), 7.0)
    rc = lib.cimpc_reference_gains_lin(m.nq, m.nu, m.nz, m.nth, 3, 2, _p(rzc), _p(rthc), _p(Qq), _p(Qv), _p(Ru), 100.0, 100.0, _p(K), _p(P1))
    msg = lib.cimpc_last_error(None).decode()
    assert rc == SINGULAR and "knot 2 " in msg, (rc, msg)
    assert np.all(K == 7.0) and np.all(P1 == 7.0)
    with pytest.raises(_lib.CimpcError, match="knot 2 "):
        gains.reference_gains_lin(m.nq, m.nu, rz0, c["rth0"][:3], *c["weights"], N=2)
    good = gains.reference_gains_lin(m.nq, m.nu, c["rz0"][:3], c["rth0"][:3], *c["weights"], N=2)      # the library goes on working
    assert np.isfinite(good).all()


def test_singular_riccati_step_names_the_step_and_leaves_k_untouched():
    n, m, T = 5, 2, 6
    rng = np.random.default_rng(7)
    A, B, Q, R = rng.standard_normal((1, n, n)), np.zeros((1, m, n)), np.eye(n)[None].copy(), np.zeros((1, m, m))
    K, P1 = np.full((T - 1, n, m), 7.0), np.full((n, n), 7.0)
    lib = _lib.load()
    rc = lib.cimpc_tvlqr(1, n, m, T, 1, _p(A), _p(B), 1, _p(Q), 1, _p(R), T - 1, _p(K), _p(P1))
    msg = lib.cimpc_last_error(None).decode()
    assert rc == SINGULAR and f"step {T - 1} " in msg, (rc, msg)          # the first step the chain walks
    assert np.all(K == 7.0) and np.all(P1 == 7.0)


# ---- the policy ----------------------------------------------------------------------------------------------------------------
KAPPA_MPC = 2e-4
H_MPC, N_SAMPLE, B_POL = 5, 5, 3


@pytest.fixture(scope="module")
def wall_problem():
    m = lcp_models.CentroidalQuadrupedWall()
    gait = gait_io.load_gait(os.path.join(gc.GAIT_DIR, "wall_stand_FL_4.jld2"))
    return lcp_models.reference_problem(m, gait, KAPPA_MPC, tables=False)


def _wall_policy(P, **kw):
    oq, ov, ou = gc.centroidal_weights()
    tile = lambda M: np.tile(M[None], (H_MPC, 1, 1))
    return CIMPCPolicy(P, tile(oq), tile(ou), H_mpc=H_MPC, N_sample=N_SAMPLE, B=B_POL, mode=0, obj_v=tile(ov), v_target=np.zeros((H_MPC, 18)),
                       n_opts=NewtonOptions(kappa=KAPPA_MPC, r_tol=3e-5, max_iter=5),
                       ip_opts=InteriorPointOptions(kappa_tol=KAPPA_MPC, r_tol=1e-4, undercut=5.0), device_tables=True, **kw)


def _states(P, calls):
    """Perturbed simulator states: the gait's configurations interpolated at the simulator rate, each robot off by its own noise."""
    rng = np.random.default_rng(8)
    out = []
    for k in range(calls):
        i, f = divmod(k, N_SAMPLE)
        q = P.q[1 + i] + (f / N_SAMPLE) * (P.q[2 + i] - P.q[1 + i])
        out.append(q[None] + 2e-3 * rng.standard_normal((B_POL, P.model.nq)))
    return out


def test_policy_applies_the_gains_as_the_formula_says_and_is_unchanged_without_them(wall_problem):
    P = wall_problem
    calls = 3 * N_SAMPLE
    states = _states(P, calls)
    plain, off, on = _wall_policy(P), _wall_policy(P, gains=False), _wall_policy(P, gains=True)
    try:
        nq, nu = P.model.nq, P.model.nu
        assert on.K.shape == (P.H, nu, 2 * nq) and np.isfinite(on.K).all()
        with pytest.raises(_lib.CimpcError, match=rf"\({STATE}\)"):
            on.solver.gain_feedback(states[0], states[0], N_SAMPLE)          # before a latch
        with pytest.raises(_lib.CimpcError, match=rf"\({STATE}\)"):
            on.solver.gain_latch()                                            # before a solve
        with pytest.raises(_lib.CimpcError, match=rf"\({STATE}\)"):
            plain.solver.gain_latch()                                         # no gains set
        latched = []
        latch = on.solver.gain_latch
        def recording():
            ref = on.solver.reference()
            latched.append(dict(q=ref["q"][:, :2].copy(), window=ref["window"][:, 0].copy(), u1=on.solver.newton_info()[0].copy()))
            latch()
        on.solver.gain_latch = recording
        q_prev = on.q0.copy()
        worst = 0.0
        for k, q1 in enumerate(states):
            u_plain, u_off, u_on = plain(q1), off(q1), on(q1)
            assert np.array_equal(u_plain, u_off)                             # gains=False: none of the new calls, the same controls
            L = latched[-1]
            assert len(latched) == k // N_SAMPLE + 1
            q0 = q1 - N_SAMPLE * (q1 - q_prev)
            for r in range(B_POL):
                Kt = on.K[L["window"][r] - 1]
                want = (L["u1"][r] + Kt @ (np.concatenate([L["q"][r, 0], L["q"][r, 1]]) - np.concatenate([q0[r], q1[r]]))) / N_SAMPLE
                worst = max(worst, np.abs(u_on[r] - want).max() / np.abs(want).max())
            assert not np.array_equal(u_on, u_off)
            q_prev = q1
        print(f"gain feedback against the NumPy formula over {calls} calls: worst max|u - want| / max|want| = {worst:.3e}")
        assert worst <= 1e-12
        assert on.solves == off.solves == 3 and [int(L["window"][0]) for L in latched] == [1, 2, 3]
        with pytest.raises(_lib.CimpcError, match=rf"\({STATE}\)"):
            latch()                                                           # after mpc_advance: the window has moved on
        on.solver.set_gains(None)                                             # off again: nothing left to latch or feed back
        with pytest.raises(_lib.CimpcError, match=rf"\({STATE}\)"):
            on.solver.gain_feedback(states[0], states[0], N_SAMPLE)
        with pytest.raises(_lib.CimpcError, match=rf"\({STATE}\)"):
            latch()
    finally:
        for p in (plain, off, on):
            p.close()


def test_gains_need_a_velocity_objective(wall_problem):
    oq, ov, ou = gc.centroidal_weights()
    tile = lambda M: np.tile(M[None], (H_MPC, 1, 1))
    with pytest.raises(ValueError, match="obj_v"):
        CIMPCPolicy(wall_problem, tile(oq), tile(ou), H_mpc=H_MPC, N_sample=N_SAMPLE, mode=0, device_tables=True, gains=True)


def test_wall_closed_loop_with_gains_runs_50_plant_steps():
    """scripts/closed_loop_wall.py --gains: the discrete policy with the feedback term and the device wall plant.  Every plant status
    converged and every control finite; there is no tracking threshold - nobody has measured this loop with gains, the reference
    records none."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("closed_loop_wall", os.path.join(ROOT, "scripts", "closed_loop_wall.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ok, out = mod.run(50, (0.0, -10.0), verbose=True, gains=True)
    assert ok
    assert all(o["controls_finite"] for o in out)
