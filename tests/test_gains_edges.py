"""The edge inputs of the gain kernels (tests/gains_edge_cases.py) held to their conditions without a device, by the references alone:
the float64 restatements (direct and adjoint order) stay within 1e-12 of the longdouble solve on every case, so the bound the GPU test
derives from them (tests/test_gpu_gains_edges.py) is a tight one; the matrices do make an LU with partial pivoting interchange rows -
in rz' at every knot, in R + B'PB at every Riccati step; the longdouble LU itself against LAPACK and against a system solved by hand;
and the validator's LDS limit, which comes before any device.

Measured with these seeds: restatements to longdouble <= 1.3e-14 (reference_gains_lin cases), <= 1.6e-15 (tvlqr cases, the batch of 300
included), 1.6e-15 to 7.9e-15 (real cases); row interchanges >= 0.87 nz per knot of rz', 1 to 14 per Riccati step."""
from fractions import Fraction

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib
import gains_cases as gc
import gains_edge_cases as ec
import gains_ref

CLOSE = 1e-12
INVALID = -1
REAL_SHORT = sorted(n for n, c in gc.CASES.items() if c[3] is not None and c[3] <= 5)


# ---- the longdouble LU ---------------------------------------------------------------------------------------------------------
def test_longdouble_has_a_64_bit_mantissa_here():
    assert np.finfo(gains_ref.LD).nmant >= 63, "numpy.longdouble is no wider than float64 on this machine: the references prove nothing"


def test_longdouble_lu_reproduces_lapack_on_a_40_by_40_system():
    rng = np.random.default_rng(11)
    M = (2 * np.eye(40) + rng.standard_normal((40, 40)) / np.sqrt(40))[rng.permutation(40)]
    rhs = rng.standard_normal((40, 5))
    assert gains_ref.row_interchanges(M) >= 20          # the pivoting is exercised, not walked past
    X = gains_ref.solve_ld(M, rhs)
    assert X.dtype == gains_ref.LD
    assert np.abs(X - np.linalg.solve(M, rhs)).max() <= 1e-13 * np.abs(X).max()
    assert np.abs(gains_ref.mm_ld(np.asarray(M, dtype=gains_ref.LD), X) - rhs).max() <= 1e-17 * 40 * np.abs(X).max()      # longdouble, not float64, accuracy


def test_longdouble_lu_on_a_3_by_3_system_solved_by_hand():
    """M = [1 2 3; 4 5 6; 7 8 10], b = (1, 1, 1).  By hand, pivoting as the LU does:
    column 1: the largest is 7 (row 3).  Rows: (7 8 10 | 1), (4 5 6 | 1) - 4/7 (..) = (0 3/7 2/7 | 3/7), (1 2 3 | 1) - 1/7 (..) = (0 6/7 11/7 | 6/7).
    column 2: the largest is 6/7 (the third row).  (0 3/7 2/7 | 3/7) - 1/2 (0 6/7 11/7 | 6/7) = (0 0 -1/2 | 0).
    Back: x3 = 0; x2 = (6/7) / (6/7) = 1; x1 = (1 - 8) / 7 = -1.   x = (-1, 1, 0); with b = (1, 0, 0): x = (-2/3, -2/3, 1)."""
    M = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 10.0]])
    assert gains_ref.row_interchanges(M) == 2
    x = gains_ref.solve_ld(M, np.ones(3))
    assert np.abs(x - np.array([-1.0, 1.0, 0.0])).max() <= 4 * np.finfo(gains_ref.LD).eps
    x = gains_ref.solve_ld(M, np.array([1.0, 0.0, 0.0]))
    want = np.array([gains_ref.LD(f.numerator) / gains_ref.LD(f.denominator) for f in (Fraction(-2, 3), Fraction(-2, 3), Fraction(1))])
    assert np.abs(x - want).max() <= 8 * np.finfo(gains_ref.LD).eps
    with pytest.raises(np.linalg.LinAlgError):
        gains_ref.solve_ld(np.array([[1.0, 2.0], [2.0, 4.0]]), np.ones(2))


def test_row_interchanges_counts_moved_rows():
    assert gains_ref.row_interchanges(np.diag([3.0, 2.0, 1.0])) == 0
    assert gains_ref.row_interchanges(np.array([[0.0, 1.0], [1.0, 0.0]])) == 1
    assert gains_ref.row_interchanges(np.eye(4)[[1, 2, 3, 0]]) == 3


# ---- the synthetic cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.LIN_NAMES)
def test_lin_case_restatements_are_close_to_the_longdouble_solve_and_rz_pivots(name):
    c = ec.lin_case(name)
    print(f"{name}: to longdouble (K, P1): direct {c['d_direct']}, adjoint {c['d_adjoint']}")
    assert np.isfinite(np.asarray(c["K_ld"], dtype=float)).all() and np.abs(c["K_ld"]).max() > 0
    assert max(*c["d_direct"], *c["d_adjoint"]) <= CLOSE
    assert c["K_ld"].shape == (c["H"], c["nu"], 2 * c["nq"]) and c["P1_ld"].shape == (2 * c["nq"], 2 * c["nq"])
    if c["nz"] >= 40:
        moved = [gains_ref.row_interchanges(c["rz0"][t].T) for t in range(c["H"])]
        print(f"{name}: row interchanges of rz' per knot: min {min(moved)} of {c['nz']}")
        assert min(moved) >= c["nz"] / 2


@pytest.mark.parametrize("name", ec.TVLQR_NAMES)
def test_tvlqr_case_restatement_is_close_to_the_longdouble_solve_and_the_riccati_factor_pivots(name):
    _riccati_conditions(name, ec.tvlqr_case(name))


@pytest.mark.parametrize("which", ["3", "300"])
def test_tvlqr_batch_restatement_is_close_to_the_longdouble_solve_and_the_riccati_factor_pivots(which):
    c = ec.batch_case(which)
    assert not np.array_equal(c["K_ld"][0], c["K_ld"][1])
    _riccati_conditions(f"batch of {which}", c)


def _riccati_conditions(name, c):
    print(f"{name}: float64 tvlqr to longdouble: K {c['d_f64'][:, 0].max():.3e}, P1 {c['d_f64'][:, 1].max():.3e}")
    assert np.isfinite(np.asarray(c["K_ld"], dtype=float)).all() and np.abs(c["K_ld"]).max() > 0
    assert c["d_f64"].max() <= CLOSE
    for Q in c["Q"].reshape(-1, c["n"], c["n"]):
        assert np.array_equal(Q, Q.T) and np.linalg.eigvalsh(Q).min() > 0
    if c["m"] >= 2:
        assert not any(np.array_equal(R, R.T) for R in c["R"].reshape(-1, c["m"], c["m"]))
    if c["m"] >= 4:
        moved = [gains_ref.row_interchanges(G) for G in c["G"].reshape(-1, c["m"], c["m"])]
        print(f"{name}: row interchanges of R + B'PB per step: {min(moved)} to {max(moved)}")
        assert min(moved) >= 1


def test_weights_of_the_lin_cases_are_not_symmetric():
    for name in ec.LIN_NAMES:
        c = ec.lin_case(name)
        for w in c["weights"]:
            assert w.shape[0] == 1 or not np.array_equal(w, w.T)


# ---- the real cases ------------------------------------------------------------------------------------------------------------
def test_the_box_case_is_among_the_short_real_cases():
    assert any(gc.CASES[n][0] == "centroidal_quadruped_box" for n in REAL_SHORT) and len(REAL_SHORT) >= 4


@pytest.mark.parametrize("name", REAL_SHORT)
def test_real_case_restatement_is_close_to_the_longdouble_solve(name):
    c = gc.case(name)
    m = c["model"]
    K_ld, P_ld = gains_ref.reference_gains_ld(m.nq, m.nu, c["rz0"], c["rth0"], *c["weights"], N=c["N"], return_P1=True)
    d = (ec._rel(c["K"], K_ld), ec._rel(c["P1"], P_ld))
    print(f"{name}: restatement to longdouble: K {d[0]:.3e}, P1 {d[1]:.3e}")
    assert max(d) <= CLOSE


# ---- the LDS limit comes before any device -------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(_lib._dp)


def _lin_call(nq, nz):
    """A well-posed one-knot call of that size: rz = I, rtheta = 0, unit weights."""
    nu, nth = 1, 2 * nq + 1
    rz, rth = np.eye(nz)[None].copy(), np.zeros((1, nth, nz))
    Qq, Qv, Ru = np.eye(nq), np.eye(nq), np.eye(nu)
    K = np.full((1, 2 * nq, nu), 7.0)
    lib = _lib.load()
    rc = lib.cimpc_reference_gains_lin(nq, nu, nz, nth, 1, 1, _p(rz), _p(rth), _p(Qq), _p(Qv), _p(Ru), 100.0, 100.0, _p(K), None)
    return rc, lib.cimpc_last_error(None).decode(), K


@pytest.mark.parametrize("nq,nz", ec.LDS_OVER_SHAPES)
def test_one_column_past_the_lds_limit_is_refused_without_a_device(nq, nz):
    rc, msg, K = _lin_call(nq, nz)
    assert rc == INVALID and "LDS" in msg, (rc, msg)
    assert np.all(K == 7.0)


@pytest.mark.parametrize("nq,nz", ec.LDS_MAX_SHAPES)
def test_the_largest_lds_size_passes_validation(nq, nz):
    rc, msg, _ = _lin_call(nq, nz)
    assert rc != INVALID, (rc, msg)          # no device: CIMPC_ERR_NO_DEVICE; with one the call runs
    assert {tuple(s[:3:2]) for s in ec.LIN_SHAPES} >= set(ec.LDS_MAX_SHAPES)      # and the GPU parity cases do run these sizes
