"""`cimpc_plant_linearize` on the device (`plant.linearize`, plant_linearize_kernel): (r0, rz0, rθ0) of every model id against the torch
linearization of `lcp_models`, on terrain against the complex-step derivatives of the NumPy restatements, optional outputs, the role
of κ, and the real knots end to end - tables built on the device run the reference's known-answer test.  Shapes are the models' own
(28 to 167 Jacobian columns: part of one wavefront, across 64, the wall's 167 on three wavefronts) with N = 3 knots, several workgroups."""
import ctypes as C
import os

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, gait_io, lcp_models, plant
import plant_linearize_cases as cases

pytestmark = pytest.mark.gpu

GAIT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaits")
PLANT_NAME = {0: "quadruped", 1: "flamingo", 2: "hopper_2D", 3: "centroidal_quadruped", 4: "centroidal_quadruped_undamped", 5: "particle",
              7: "centroidal_quadruped_box", 8: "centroidal_quadruped_wall", 10: "hopper_3D", 12: "pushbot", 13: "walledcartpole"}


def _raw(name, z, th, kappa, want=("r0", "rz0", "rth0"), terrain=None):
    """The entry itself, with outputs left out: -> dict of the outputs asked for, in the library's (column-major) layout."""
    mid = plant.model_dims(name)[0]
    N, nz, nth = z.shape[0], z.shape[1], th.shape[1]
    out = {"r0": np.zeros((N, nz)), "rz0": np.zeros((N, nz, nz)), "rth0": np.zeros((N, nth, nz))}
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ter, nt = (None, 0) if terrain is None else plant._terrain_array(terrain, N)
    rc = _lib.load().cimpc_plant_linearize(mid, N, nt, ter, dp(np.ascontiguousarray(z)), dp(np.ascontiguousarray(th)), float(kappa),
                                           *[dp(out[k]) if k in want else None for k in ("r0", "rz0", "rth0")])
    assert rc == 0, rc
    return {k: out[k] for k in want}


# ---- 1. every id against torch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", sorted(cases.TORCH_MODELS))
def test_every_model_matches_torch(mid):
    z, th, ref = cases.torch_case(mid)
    got = plant.linearize(PLANT_NAME[mid], z, th, cases.KAPPA)
    assert [a.shape for a in got] == [a.shape for a in ref] and all(a.flags["C_CONTIGUOUS"] for a in got)
    cases.assert_linearization(got, ref, PLANT_NAME[mid])


def test_one_knot_is_unbatched_and_equal_to_its_row_of_the_batch():
    z, th, ref = cases.torch_case(0)
    got = plant.linearize("quadruped", z[0], th[0], cases.KAPPA)
    assert [a.shape for a in got] == [(43,), (43, 43), (43, 34)]
    cases.assert_linearization(got, [a[0] for a in ref], "quadruped, N = 1")
    for a, b in zip(got, plant.linearize("quadruped", z, th, cases.KAPPA)):
        assert np.array_equal(a, b[0])


# ---- 2. outputs optional --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", [8, 13])
@pytest.mark.parametrize("want", [("r0", "rz0"), ("r0", "rth0"), ("rz0", "rth0"), ("r0",), ("rz0",), ("rth0",)])
def test_a_skipped_output_leaves_the_others_unchanged(mid, want):
    z, th, _ = cases.torch_case(mid)
    full = _raw(PLANT_NAME[mid], z, th, cases.KAPPA)
    part = _raw(PLANT_NAME[mid], z, th, cases.KAPPA, want)
    for k in want:
        assert np.array_equal(part[k], full[k]), k


# ---- 3. terrain -----------------------------------------------------------------------------------------------------------------------
def test_quadruped_on_a_terrain_per_knot():
    """N = 3 with n_terrain = N: a sine, piecewise1 and flat ground in one batch, each against its restatement; the flat knot equals
    the no-terrain call bit for bit; one shared terrain equals N copies of it."""
    names = ["sine1_2D_lc", "piecewise1_2D_lc", "flat_2D_lc"]
    z, th = cases.inputs(100, 43, 34, 3)
    z[:, 0] = [0.3, 0.55, 1.7]                       # over the sine, inside piecewise1's first blend (0.4 .. 0.6), anywhere
    got = plant.linearize("quadruped", z, th, cases.KAPPA, terrain=names)
    for k in range(2):
        ref = cases.complex_step(cases.restatement("quadruped", names[k]), z[k], th[k], cases.KAPPA)
        cases.assert_linearization([a[k] for a in got], ref, f"quadruped on {names[k]}")
    flat = plant.linearize("quadruped", z, th, cases.KAPPA)
    for a, b in zip(got, flat):
        assert np.array_equal(a[2], b[2])
        assert not np.array_equal(a[0], b[0])        # ... and the rough knots are not the flat ones
    cases.assert_linearization([a[2] for a in got], lcp_models.Quadruped().linearize(z[2], th[2], cases.KAPPA), "quadruped, the flat knot")
    one = plant.linearize("quadruped", z, th, cases.KAPPA, terrain="sine1_2D_lc")
    for a, b in zip(one, plant.linearize("quadruped", z, th, cases.KAPPA, terrain=["sine1_2D_lc"] * 3)):
        assert np.array_equal(a, b)
    for a, b in zip(one, got):
        assert np.array_equal(a[0], b[0])


@pytest.mark.parametrize("model,mid,terrain", [c for c in cases.TERRAIN_CASES if c[0] != "quadruped"])
def test_terrain_families_match_the_restatements(model, mid, terrain):
    z, th, ref = cases.terrain_case(model, mid, terrain, 3)
    got = plant.linearize(model, z, th, cases.KAPPA, terrain=terrain)
    for k in range(3):
        cases.assert_linearization([a[k] for a in got], ref[k], f"{model} on {terrain}, knot {k}")


# ---- 4. κ -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", [0, 8])
def test_kappa_enters_the_bilinear_rows_of_r0_alone(mid):
    z, th, _ = cases.torch_case(mid)
    mid_, nq, nu, nc, fd, nw = plant.model_dims(PLANT_NAME[mid])
    a, b = plant.linearize(PLANT_NAME[mid], z, th, 0.0), plant.linearize(PLANT_NAME[mid], z, th, cases.KAPPA)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    lin = nq + 2 * nc + fd * nc                      # dynamics, s1 - ϕ, η - ..., s2 - ...: no κ
    assert np.array_equal(a[0][:, :lin], b[0][:, :lin])
    assert np.array_equal(b[0][:, lin:], a[0][:, lin:] - cases.KAPPA)        # γ s1 - κ, b ∘ η - κ, ψ s2 - κ: one subtraction each


# ---- 5. real knots, end to end --------------------------------------------------------------------------------------------------------
def _assert_tables(P, Q, what):
    assert np.array_equal(P.z, Q.z) and np.array_equal(P.theta, Q.theta)
    for t in range(P.H):
        cases.assert_linearization((P.r0[t], P.rz0[t], P.rth0[t]), (Q.r0[t], Q.rz0[t], Q.rth0[t]), f"{what} knot {t}")


def test_reference_known_answer_test_on_device_built_tables():
    """test/controller/implicit_dynamics.jl:7-24 as tests/test_gpu_real_problems.py runs it (quadruped gait2, κ = 1e-4, H = 30, four
    phases), with the tables of every knot built by `plant.linearizer`: within the tolerances of the torch tables, every solve
    converges and |dq2|_inf < 1e-2."""
    from common import make_solver
    from contactimplicitmpc.jl_amd import InteriorPointOptions
    from real_problems import GAITS, real_problem, real_rollout
    d, Q, _, _ = real_problem("quadruped", 1e-4)
    model = lcp_models.Quadruped()
    P = lcp_models.reference_problem(model, gait_io.load_gait(GAITS["quadruped"][1]), 1e-4, linearize=plant.linearizer("quadruped"))
    _assert_tables(P, Q, "gait2")
    prob = dict(z0=P.z, th0=P.theta, r0=P.r0, rz0=P.rz0, rth0=P.rth0, kappa=1e-4, q_ref=P.q, u_ref=P.u, w_ref=P.w, gamma_ref=P.gamma,
                b_ref=P.b, stride=lcp_models.get_stride(model, P.q), P=P)
    H = 30
    rollouts = [real_rollout(d, prob, H, phase, seed=0) for phase in (0, 30, 45, 59)]
    s = make_solver(d, prob, rollouts, H, ip_opts=InteriorPointOptions(kappa_tol=2e-4, r_tol=1e-8))
    trs = []
    for (window, ref, q0, q1) in rollouts:          # the state newton_solve! sweeps first (common.oracle_sweep)
        tr = ref.copy()
        tr.q[0], tr.q[1] = q0, q1
        tr.update_theta(d, 0)
        tr.update_theta(d, 1)
        trs.append(tr)
    out = s.implicit_dynamics(np.stack([tr.q for tr in trs]), np.stack([tr.theta for tr in trs]))
    assert out["status"].all()
    print("max |dq2|", np.abs(out["d"]).max())
    assert np.abs(out["d"]).max() < 1e-2


def test_wall_and_hopper_3d_tables_of_their_gaits():
    model = lcp_models.CentroidalQuadrupedWall()
    g = gait_io.load_gait(os.path.join(GAIT_DIR, "wall_stand_FL_4.jld2"))
    _assert_tables(lcp_models.reference_problem(model, g, 1e-3, linearize=plant.linearizer("centroidal_quadruped_wall")),
                   lcp_models.reference_problem(model, g, 1e-3), "wall_stand_FL_4")
    model = lcp_models.Hopper3D()
    t = gait_io.load_joint_traj(os.path.join(GAIT_DIR, "hopper_3D_gait_in_place.jld2"))
    _assert_tables(lcp_models.reference_problem_from_traj(model, t, 1e-4, linearize=plant.linearizer("hopper_3D")),
                   lcp_models.reference_problem_from_traj(model, t, 1e-4), "hopper_3D gait_in_place")
