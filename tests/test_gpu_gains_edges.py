"""The gain kernels (csrc/gains.hip: gains_dynamics_kernel, tvlqr_kernel) at their edges, against the longdouble solve of
tests/gains_ref.py on the synthetic inputs of tests/gains_edge_cases.py: row interchanges at nearly every column of both LUs, nz around
the 64-lane pivot search, nq = 24, the largest LDS the validator lets through, the edges of the 2 x 3 product tiles (odd rows, columns
no multiple of 3, m > n, n = 1, m = 1), T = 2, n_ab > T - 1, per-problem strides with n_q = T and n_keep < T - 1, more workgroups than
CUs, weights that are not symmetric; the bit identities between calls; and every error return.

The bound of a parity figure max|dev - ld| / max|ld| (K and P1 each) is min(1e-9, 100 x max(d_direct, d_adjoint, 2.2e-16)), d_* being
the float64 restatements' own distances to the longdouble solve on that case (`ec.bound`): it comes from the references, never from the
device.  tests/test_gains_edges.py holds the same inputs to their conditions without a device.

Measured on an MI355X (`profiles/gains_parity_edges.json`, scripts/gains_parity.py --edges): reference_gains_lin K <= 6.9e-15, P1 <= 2.4e-15
against bounds of 2.2e-14 to 1.3e-12; tvlqr K <= 1.9e-15, P1 <= 9.2e-16 (all 300 problems of the batch included) against 2.2e-14 to
1.6e-13; the closest any figure comes to its bound is a factor of 36.  The two largest LDS sizes (163 504 B and 163 600 B of 163 840) were
granted and ran."""
import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, gains
import gains_edge_cases as ec
import gains_ref

pytestmark = pytest.mark.gpu

OK, SINGULAR = 0, -5


def _p(a):
    return a.ctypes.data_as(_lib._dp)


def _cm(a):
    return np.ascontiguousarray(np.swapaxes(np.asarray(a, dtype=np.float64), -1, -2))


def _raw_tvlqr(A, B, Q, R, T, n_keep=None):
    """cimpc_tvlqr on (n_prob, n_ab, n, n), (n_prob, n_ab, n, m), (n_prob, n_q, n, n), (n_prob, n_r, m, m) with K and P1 pre-filled with
    7.0: (rc, message, K (n_prob, n_keep, m, n), P1 (n_prob, n, n)) in numpy's order."""
    n_prob, n_ab, n, m = B.shape
    n_keep = T - 1 if n_keep is None else n_keep
    Ac, Bc, Qc, Rc = _cm(A), _cm(B), _cm(Q), _cm(R)
    K, P1 = np.full((n_prob, n_keep, n, m), 7.0), np.full((n_prob, n, n), 7.0)
    lib = _lib.load()
    rc = lib.cimpc_tvlqr(n_prob, n, m, T, n_ab, _p(Ac), _p(Bc), Q.shape[1], _p(Qc), R.shape[1], _p(Rc), n_keep, _p(K), _p(P1))
    return rc, lib.cimpc_last_error(None).decode(), np.ascontiguousarray(K.transpose(0, 1, 3, 2)), np.ascontiguousarray(P1.transpose(0, 2, 1))


def _raw_lin(c, rz0=None, rth0=None, weights=None):
    """cimpc_reference_gains_lin on the case's inputs, or on damaged copies of them, K and P1 pre-filled with 7.0."""
    nq, nu, nz, nth, N = c["nq"], c["nu"], c["nz"], c["nth"], c["N"]
    rz0 = c["rz0"] if rz0 is None else rz0
    rth0 = c["rth0"] if rth0 is None else rth0
    H = len(rz0)
    rzc, rthc = _cm(rz0), _cm(rth0)
    Qq, Qv, Ru = (_cm(w) for w in (c["weights"] if weights is None else weights))
    K, P1 = np.full((H, 2 * nq, nu), 7.0), np.full((2 * nq, 2 * nq), 7.0)
    lib = _lib.load()
    rc = lib.cimpc_reference_gains_lin(nq, nu, nz, nth, H, N, _p(rzc), _p(rthc), _p(Qq), _p(Qv), _p(Ru), 100.0, 100.0, _p(K), _p(P1))
    return rc, lib.cimpc_last_error(None).decode(), np.ascontiguousarray(K.transpose(0, 2, 1)), np.ascontiguousarray(P1.T)


def _untouched(*arrays):
    return all(np.all(a == 7.0) for a in arrays)


# ---- parity with the longdouble solve ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.LIN_NAMES)
def test_reference_gains_lin_matches_the_longdouble_solve(name):
    c = ec.lin_case(name)
    K, P1 = gains.reference_gains_lin(c["nq"], c["nu"], c["rz0"], c["rth0"], *c["weights"], N=c["N"], return_P1=True)
    assert K.shape == c["K_ld"].shape and P1.shape == c["P1_ld"].shape
    d = (ec._rel(K, c["K_ld"]), ec._rel(P1, c["P1_ld"]))
    b = tuple(ec.bound(c["d_direct"][i], c["d_adjoint"][i]) for i in range(2))
    print(f"{name}: max|dev - ld| / max|ld|: K {d[0]:.3e} (bound {b[0]:.3e}), P1 {d[1]:.3e} (bound {b[1]:.3e}); "
          f"float64 direct {c['d_direct']}, adjoint {c['d_adjoint']}")
    assert d[0] <= b[0] and d[1] <= b[1]


@pytest.mark.parametrize("name", ec.TVLQR_NAMES)
def test_tvlqr_matches_the_longdouble_solve(name):
    c = ec.tvlqr_case(name)
    rc, msg, K, P1 = _raw_tvlqr(c["A"], c["B"], c["Q"], c["R"], c["T"])
    assert rc == OK, (rc, msg)
    d = (ec._rel(K[0], c["K_ld"][0]), ec._rel(P1[0], c["P1_ld"][0]))
    b = (ec.bound(c["d_f64"][0, 0]), ec.bound(c["d_f64"][0, 1]))
    print(f"{name}: max|dev - ld| / max|ld|: K {d[0]:.3e} (bound {b[0]:.3e}), P1 {d[1]:.3e} (bound {b[1]:.3e}); float64 {tuple(c['d_f64'][0])}")
    assert d[0] <= b[0] and d[1] <= b[1]


# ---- identities ----------------------------------------------------------------------------------------------------------------
def test_batch_of_three_with_n_keep_equals_single_calls_bit_for_bit():
    """n_q = T, n_r = T - 1, n_keep = 4 < T - 1: every per-problem stride differs from the constant-weight, keep-all one."""
    c = ec.batch_case("3")
    keep = ec.BATCH_3_KEEP
    K, P1 = gains.tvlqr(c["A"], c["B"], c["Q"], c["R"], n_keep=keep)
    assert K.shape == (3, keep, c["m"], c["n"]) and P1.shape == (3, c["n"], c["n"])
    for p in range(3):
        Kp, Pp = gains.tvlqr(c["A"][p], c["B"][p], c["Q"][p], c["R"][p], n_keep=keep)
        assert np.array_equal(K[p], Kp) and np.array_equal(P1[p], Pp)
        d = (ec._rel(Kp, c["K_ld"][p, :keep]), ec._rel(Pp, c["P1_ld"][p]))
        print(f"batch of 3, problem {p}: K {d[0]:.3e}, P1 {d[1]:.3e}")
        assert d[0] <= ec.bound(c["d_f64"][p, 0]) and d[1] <= ec.bound(c["d_f64"][p, 1])
    assert not np.array_equal(K[0], K[1]) and not np.array_equal(K[1], K[2])


def test_batch_of_300_equals_single_calls_and_every_problem_meets_the_bound():
    c = ec.batch_case("300")
    K, P1 = gains.tvlqr(c["A"], c["B"], c["Q"], c["R"])
    assert K.shape == c["K_ld"].shape
    for p in (0, 1, 149, 255, 299):
        Kp, Pp = gains.tvlqr(c["A"][p], c["B"][p], c["Q"][p], c["R"][p])
        assert np.array_equal(K[p], Kp) and np.array_equal(P1[p], Pp), p
    d = np.array([(ec._rel(K[p], c["K_ld"][p]), ec._rel(P1[p], c["P1_ld"][p])) for p in range(300)])
    b = np.array([(ec.bound(x), ec.bound(y)) for x, y in c["d_f64"]])
    print(f"batch of 300: worst K {d[:, 0].max():.3e}, P1 {d[:, 1].max():.3e}; smallest margin to the bound {np.min(b / np.maximum(d, 1e-300)):.1f} x")
    assert np.all(d <= b)


@pytest.mark.parametrize("name", ["n=47 m=15 T=4 n_ab=7 Q const", "n=16 m=4 T=9 n_ab=9 n_q=T"])
def test_more_dynamics_than_steps_equals_the_truncated_call_bit_for_bit(name):
    c = ec.tvlqr_case(name)
    T = c["T"]
    assert c["n_ab"] > T - 1
    rc, msg, K, P1 = _raw_tvlqr(c["A"], c["B"], c["Q"], c["R"], T)
    rc2, msg2, K2, P2 = _raw_tvlqr(c["A"][:, :T - 1], c["B"][:, :T - 1], c["Q"], c["R"], T)
    assert rc == OK and rc2 == OK, (msg, msg2)
    assert np.isfinite(K).all() and np.array_equal(K, K2) and np.array_equal(P1, P2)


def test_nan_in_an_unread_column_of_rtheta_changes_nothing():
    c = ec.lin_inputs(ec.ERRORS_SHAPE)
    first_unread = 2 * c["nq"] + c["nu"]
    assert c["nth"] > first_unread
    rc, msg, K, P1 = _raw_lin(c)
    assert rc == OK and np.isfinite(K).all() and np.isfinite(P1).all(), (rc, msg)
    rth0 = c["rth0"].copy()
    rth0[:, :, first_unread] = np.nan
    rth0[2, 11, c["nth"] - 1] = np.nan
    rc2, msg2, K2, P2 = _raw_lin(c, rth0=rth0)
    assert rc2 == OK, (rc2, msg2)
    assert np.array_equal(K, K2) and np.array_equal(P1, P2)


def test_a_transposed_state_weight_changes_the_gains():
    """The weights of these cases are not symmetric, so the case can see a transpose: the device follows obj_q' to the longdouble answer
    for obj_q', which is far from the answer for obj_q."""
    c = ec.lin_case("nq=7 nu=3 nz=65 nth=21 H=2 N=2")
    oq, ov, ou = c["weights"]
    K_t = gains.reference_gains_lin(c["nq"], c["nu"], c["rz0"], c["rth0"], oq.T, ov, ou, N=c["N"])
    K_t_ld = gains_ref.reference_gains_ld(c["nq"], c["nu"], c["rz0"], c["rth0"], oq.T, ov, ou, N=c["N"])
    b = ec.bound(c["d_direct"][0], c["d_adjoint"][0])
    moved = ec._rel(K_t, c["K_ld"])
    print(f"transposed obj_q: K moves by {moved:.3e} of its scale; to its own longdouble answer {ec._rel(K_t, K_t_ld):.3e} (bound {b:.3e})")
    assert ec._rel(K_t, K_t_ld) <= b
    assert moved > 1e-4 > 1e3 * b


# ---- error returns -------------------------------------------------------------------------------------------------------------
def _good_lin_call_still_works():
    c = ec.lin_case("nq=2 nu=1 nz=2 nth=5 H=2 N=3")
    K = gains.reference_gains_lin(c["nq"], c["nu"], c["rz0"], c["rth0"], *c["weights"], N=c["N"])
    assert ec._rel(K, c["K_ld"]) <= ec.bound(c["d_direct"][0], c["d_adjoint"][0])


def _good_tvlqr_call_still_works():
    c = ec.tvlqr_case("n=1 m=1 T=7 n_ab=3 Q const")
    rc, msg, K, P1 = _raw_tvlqr(c["A"], c["B"], c["Q"], c["R"], c["T"])
    assert rc == OK and ec._rel(K[0], c["K_ld"][0]) <= ec.bound(c["d_f64"][0, 0]), (rc, msg)


def _zero_column(rz0, knot, col):
    rz0[knot - 1][:, col] = 0.0          # a zero row of rz': it stays exactly zero under every row operation, so some pivot is zero


def _inf_entry(rz0, knot):
    rz0[knot - 1][5, 11] = np.inf        # an Inf pivot: the largest of its column, or it has made the column non-finite before


def _nan_entry(rz0, knot):
    rz0[knot - 1][40, 64] = np.nan


@pytest.mark.parametrize("damage,knot", [
    (lambda rz: (_zero_column(rz, 2, 20), _zero_column(rz, 4, 3)), 2),
    (lambda rz: (_zero_column(rz, 5, 64),), 5),
    (lambda rz: (_inf_entry(rz, 3),), 3),
    (lambda rz: (_nan_entry(rz, 1),), 1),
], ids=["zero columns at knots 2 and 4", "zero column at the last knot", "+Inf at knot 3", "NaN at knot 1"])
@pytest.mark.parametrize("order", ["as drawn", "reversed in memory"])
def test_singular_rz_names_the_smallest_knot_and_leaves_the_outputs_untouched(damage, knot, order):
    """`reversed in memory`: the five knots' matrices in the opposite order, damaged at the same knot NUMBERS - whichever of two singular
    knots' workgroups reaches the status word first, the smaller number stays (atomicMin)."""
    c = ec.lin_inputs(ec.ERRORS_SHAPE)
    rz0, rth0 = (c["rz0"][::-1].copy(), c["rth0"][::-1].copy()) if order != "as drawn" else (c["rz0"].copy(), c["rth0"].copy())
    damage(rz0)
    rc, msg, K, P1 = _raw_lin(c, rz0=rz0, rth0=rth0)
    assert rc == SINGULAR and f"knot {knot} " in msg, (rc, msg)
    assert _untouched(K, P1)
    _good_lin_call_still_works()


def test_nan_in_a_read_column_of_rtheta_alone_is_singular_at_its_knot():
    """rz is sound at every knot, so no pivot test sees it: the `finite` flag on D does."""
    c = ec.lin_inputs(ec.ERRORS_SHAPE)
    rth0 = c["rth0"].copy()
    rth0[2, 33, 2 * c["nq"] + c["nu"] - 1] = np.nan          # the last column that is read
    rc, msg, K, P1 = _raw_lin(c, rth0=rth0)
    assert rc == SINGULAR and "knot 3 " in msg, (rc, msg)
    assert _untouched(K, P1)
    _good_lin_call_still_works()


def test_zero_control_weight_and_no_control_is_a_singular_riccati_step_through_reference_gains_lin():
    c = ec.lin_inputs(ec.ERRORS_SHAPE)
    nq, nu, H, N = c["nq"], c["nu"], c["H"], c["N"]
    rth0 = c["rth0"].copy()
    rth0[:, :, 2 * nq:2 * nq + nu] = 0.0                     # B_t = 0
    oq, ov, _ = c["weights"]
    rc, msg, K, P1 = _raw_lin(c, rth0=rth0, weights=(oq, ov, np.zeros((nu, nu))))
    assert rc == SINGULAR and f"Riccati step {N * H} (1-based) of {N * H}" in msg, (rc, msg)      # the first step the chain walks
    assert _untouched(K, P1)
    _good_lin_call_still_works()


def test_one_singular_problem_in_a_batch_is_named_and_no_block_is_written():
    c = ec.batch_case("3")
    T = c["T"]
    B, R = c["B"].copy(), c["R"].copy()
    B[1], R[1] = 0.0, 0.0
    rc, msg, K, P1 = _raw_tvlqr(c["A"], B, c["Q"], R, T)
    assert rc == SINGULAR and "problem 1" in msg and f"step {T - 1} " in msg, (rc, msg)
    assert K.shape[0] == 3 and _untouched(K, P1)
    _good_tvlqr_call_still_works()


def _chain_with_a_step_per_matrix(varying_q):
    c = ec.tvlqr_case("n=16 m=4 T=9 n_ab=9 " + ("n_q=T" if varying_q else "Q const"))
    T = c["T"]
    return c, T, c["A"][:, :T - 1].copy(), c["B"][:, :T - 1].copy(), c["Q"].copy()      # n_ab = T - 1: A[0] is read at the last step walked only


def test_nan_in_the_last_dynamics_the_chain_reads_is_singular_at_step_1():
    """A_t enters B'PA and A - BK, never R + B'PB: a NaN in A[0] with n_ab = T - 1 meets no pivot test.  K[0] and P1 are NaN; the parent
    of this check returned CIMPC_OK with them."""
    c, T, A, B, Q = _chain_with_a_step_per_matrix(False)
    assert _raw_tvlqr(A, B, Q, c["R"], T)[0] == OK
    A[0, 0, 3, 5] = np.nan
    rc, msg, K, P1 = _raw_tvlqr(A, B, Q, c["R"], T)
    assert rc == SINGULAR and "step 1 " in msg, (rc, msg)
    assert _untouched(K, P1)
    _good_tvlqr_call_still_works()


def test_nan_in_the_first_state_weight_is_singular_at_step_1():
    """Q[0] with n_q = T enters P1 alone."""
    c, T, A, B, Q = _chain_with_a_step_per_matrix(True)
    assert Q.shape[1] == T and _raw_tvlqr(A, B, Q, c["R"], T)[0] == OK
    Q[0, 0, 2, 7] = np.nan
    rc, msg, K, P1 = _raw_tvlqr(A, B, Q, c["R"], T)
    assert rc == SINGULAR and "step 1 " in msg, (rc, msg)
    assert _untouched(K, P1)
    _good_tvlqr_call_still_works()


def test_non_finite_dynamics_mid_chain_name_the_first_step_in_walk_order():
    """+Inf in A[4] and NaN in A[2] (n_ab = T - 1): steps 5 and 3 (1-based); the chain walks T - 1, ..., 1 and stops at 5."""
    c, T, A, B, Q = _chain_with_a_step_per_matrix(False)
    A[0, 4, 0, 0] = np.inf
    A[0, 2, 1, 1] = np.nan
    rc, msg, K, P1 = _raw_tvlqr(A, B, Q, c["R"], T)
    assert rc == SINGULAR and "step 5 " in msg, (rc, msg)
    assert _untouched(K, P1)
    _good_tvlqr_call_still_works()
