"""The feedback gains without a device: the NumPy restatement of gains.jl (tests/gains_ref.py) against known answers, the argument
validation of the three stateless entries (it comes before any device call: the library loads and answers without a GPU), and the six
new exports as declared in include/cimpc.h, bound in _lib.py and called from julia/CIMPCHip.jl."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib
import gains_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID = -1
NEW = {"cimpc_tvlqr": 14, "cimpc_reference_gains_lin": 15, "cimpc_reference_gains": 14, "cimpc_set_gains": 2, "cimpc_gain_latch": 1,
       "cimpc_gain_feedback": 5}
JL_FUNCTION = {"cimpc_tvlqr": "tvlqr", "cimpc_reference_gains_lin": "reference_gains_lin", "cimpc_reference_gains": "reference_gains",
               "cimpc_set_gains": "set_gains!", "cimpc_gain_latch": "gain_latch!", "cimpc_gain_feedback": "gain_feedback!"}
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "cimpc_handle": C.c_void_p,
         "const cimpc_terrain*": C.POINTER(_lib.Terrain)}


# ---- the restatement against known answers -------------------------------------------------------------------------------------
def test_scalar_time_invariant_system_converges_to_the_dare_root():
    a, b, q, r = 1.1, 0.7, 2.0, 0.5
    # P = q + a^2 P - a^2 b^2 P^2 / (r + b^2 P)  <=>  b^2 P^2 + (r - q b^2 - a^2 r) P - q r = 0
    c1 = r - q * b * b - a * a * r
    P_inf = (-c1 + np.sqrt(c1 * c1 + 4 * b * b * q * r)) / (2 * b * b)
    K_inf = a * b * P_inf / (r + b * b * P_inf)
    T = 200
    M = lambda v: np.array([[v]])
    K, P = gains_ref.tvlqr([M(a)] * (T - 1), [M(b)] * (T - 1), [M(q)] * T, [M(r)] * (T - 1))
    assert abs(P[0][0, 0] - P_inf) <= 1e-13 * P_inf and abs(K[0][0, 0] - K_inf) <= 1e-13 * K_inf
    assert P[T - 1][0, 0] == q                                                  # P[T] = Q[T]
    assert abs(K[T - 2][0, 0] - a * b * q / (r + b * b * q)) < 1e-15             # the last gain sees Q alone


def test_terminal_cost_is_the_last_weight_also_with_time_varying_weights():
    rng = np.random.default_rng(0)
    n, m, T = 4, 2, 5
    A = [rng.standard_normal((n, n)) for _ in range(T - 1)]
    B = [rng.standard_normal((n, m)) for _ in range(T - 1)]
    Q = [np.diag(rng.uniform(1, 2, n)) for _ in range(T)]
    R = [np.diag(rng.uniform(1, 2, m)) for _ in range(T - 1)]
    K, P = gains_ref.tvlqr(A, B, Q, R)
    assert len(K) == T - 1 and len(P) == T and K[0].shape == (m, n)
    np.testing.assert_array_equal(P[T - 1], Q[T - 1])


def test_block_structure_of_the_knot_dynamics_and_weights():
    rng = np.random.default_rng(1)
    nq, nu, nz, nth = 3, 2, 9, 11
    rz, rth = rng.standard_normal((nz, nz)) + 4 * np.eye(nz), rng.standard_normal((nz, nth))
    A, B = gains_ref.dynamics(nq, nu, rz, rth)
    assert A.shape == (2 * nq, 2 * nq) and B.shape == (2 * nq, nu)
    np.testing.assert_array_equal(A[:nq], np.hstack([np.zeros((nq, nq)), np.eye(nq)]))
    np.testing.assert_array_equal(B[:nq], 0.0)
    D = -np.linalg.inv(rz) @ rth
    np.testing.assert_allclose(np.hstack([A[nq:], B[nq:]]), D[:nq, :2 * nq + nu], rtol=0, atol=1e-13)
    oq, ov, ou = np.diag([1.0, 2.0, 3.0]), np.diag([0.1, 0.2, 0.3]), np.diag([5.0, 7.0])
    Q, R = gains_ref.weights(oq, ov, ou, U_scaling=10.0, V_scaling=100.0)
    np.testing.assert_array_equal(Q[:nq, :nq], oq + 100.0 * ov)
    np.testing.assert_array_equal(Q[nq:, nq:], Q[:nq, :nq])
    np.testing.assert_array_equal(Q[:nq, nq:], -100.0 * ov)
    np.testing.assert_array_equal(Q[nq:, :nq], -100.0 * ov)
    np.testing.assert_array_equal(R, 10.0 * ou)


def test_two_knot_chain_written_out_by_hand():
    """N = 1, H = 2: P3 = Q; K2, P2 from knot 2; K1 from knot 1 and P2 - the gains come back in knot order."""
    rng = np.random.default_rng(2)
    nq, nu, nz, nth = 2, 1, 6, 8
    rz = rng.standard_normal((2, nz, nz)) + 4 * np.eye(nz)
    rth = rng.standard_normal((2, nz, nth))
    oq, ov, ou = np.diag([1.0, 2.0]), np.diag([0.3, 0.1]), np.array([[0.5]])
    K, P1 = gains_ref.reference_gains(nq, nu, rz, rth, oq, ov, ou, N=1, U_scaling=3.0, V_scaling=7.0, return_P1=True)
    Q = np.block([[oq + 7 * ov, -7 * ov], [-7 * ov, oq + 7 * ov]])
    R = 3.0 * ou
    def AB(t):
        D = np.linalg.solve(-rz[t], rth[t])[:nq]
        return np.vstack([np.hstack([np.zeros((2, 2)), np.eye(2)]), D[:, :4]]), np.vstack([np.zeros((2, 1)), D[:, 4:5]])
    A1, B1 = AB(0)
    A2, B2 = AB(1)
    K2 = np.linalg.solve(R + B2.T @ Q @ B2, B2.T @ Q @ A2)
    P2 = Q + K2.T @ R @ K2 + (A2 - B2 @ K2).T @ Q @ (A2 - B2 @ K2)
    K1 = np.linalg.solve(R + B1.T @ P2 @ B1, B1.T @ P2 @ A1)
    P1h = Q + K1.T @ R @ K1 + (A1 - B1 @ K1).T @ P2 @ (A1 - B1 @ K1)
    np.testing.assert_allclose(K, np.stack([K1, K2]), rtol=1e-13, atol=0)
    np.testing.assert_allclose(P1, P1h, rtol=1e-13, atol=0)


def test_repeats_make_the_chain_periodic_and_converge():
    """N copies of the same knots: K[1:H] of N = 6 and N = 7 agree once the Riccati recursion has settled, and differ from N = 1."""
    rng = np.random.default_rng(3)
    nq, nu, nz, nth, H = 2, 2, 6, 9, 3
    rz = rng.standard_normal((H, nz, nz)) + 5 * np.eye(nz)
    rth = rng.standard_normal((H, nz, nth))
    w = (np.eye(nq), 0.01 * np.eye(nq), 0.1 * np.eye(nu))
    K1, K6, K7 = (gains_ref.reference_gains(nq, nu, rz, rth, *w, N=N, U_scaling=1.0, V_scaling=1.0) for N in (1, 6, 7))
    assert np.abs(K6 - K7).max() < 1e-6 * np.abs(K7).max() < np.abs(K1 - K7).max()


# ---- validation comes before any device ----------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(_lib._dp)


def test_tvlqr_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    n, m, T = 4, 2, 6
    A, B, Q, R = np.zeros((1, n, n)), np.zeros((1, n, m)), np.zeros((1, n, n)), np.zeros((1, m, m))
    K, P1 = np.full((T - 1, n, m), 7.0), np.full((n, n), 7.0)
    good = dict(n_prob=1, n=n, m=m, T=T, n_ab=1, A=_p(A), B=_p(B), n_q=1, Q=_p(Q), n_r=1, R=_p(R), n_keep=T - 1, K=_p(K), P1=_p(P1))
    order = ["n_prob", "n", "m", "T", "n_ab", "A", "B", "n_q", "Q", "n_r", "R", "n_keep", "K", "P1"]
    bad = [dict(A=None), dict(B=None), dict(Q=None), dict(R=None), dict(K=None), dict(n_prob=0), dict(n=0), dict(m=0), dict(T=1), dict(T=0),
           dict(n_ab=0), dict(n_q=2), dict(n_q=0), dict(n_r=2), dict(n_r=T), dict(n_keep=0), dict(n_keep=T), dict(n=49), dict(m=17)]
    for over in bad:
        a = {**good, **over}
        assert lib.cimpc_tvlqr(*[a[k] for k in order]) == INVALID, over
        assert lib.cimpc_last_error(None)
    assert np.all(K == 7.0) and np.all(P1 == 7.0)


def test_reference_gains_lin_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    nq, nu, nz, nth, H = 3, 2, 9, 11, 2
    rz, rth = np.zeros((H, nz, nz)), np.zeros((H, nth, nz))
    Qq, Qv, Ru = np.eye(nq), np.eye(nq), np.eye(nu)
    K = np.full((H, 2 * nq, nu), 7.0)
    good = dict(nq=nq, nu=nu, nz=nz, nth=nth, H=H, N=2, rz0=_p(rz), rth0=_p(rth), Qq=_p(Qq), Qv=_p(Qv), Ru=_p(Ru), Us=100.0, Vs=100.0, K=_p(K), P1=None)
    order = ["nq", "nu", "nz", "nth", "H", "N", "rz0", "rth0", "Qq", "Qv", "Ru", "Us", "Vs", "K", "P1"]
    bad = [dict(rz0=None), dict(rth0=None), dict(Qq=None), dict(Qv=None), dict(Ru=None), dict(K=None), dict(nq=0), dict(nu=0), dict(nz=0), dict(nth=0),
           dict(H=0), dict(N=0), dict(N=-1), dict(Us=0.0), dict(Us=-1.0), dict(Us=float("inf")), dict(Us=float("nan")), dict(Vs=0.0),
           dict(Vs=float("nan")), dict(nth=2 * nq + nu - 1), dict(nz=nq - 1), dict(nq=25), dict(nu=17, nth=2 * nq + 17)]
    for over in bad:
        a = {**good, **over}
        assert lib.cimpc_reference_gains_lin(*[a[k] for k in order]) == INVALID, over
    assert np.all(K == 7.0)


def test_reference_gains_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    mid, nq, nu, nz, nth, H = 10, 7, 3, 19, 22, 2          # hopper_3D
    z, th = np.zeros((H, nz)), np.ones((H, nth))
    Qq, Qv, Ru = np.eye(nq), np.eye(nq), np.eye(nu)
    K = np.full((H, 2 * nq, nu), 7.0)
    ter = (_lib.Terrain * 1)()
    good = dict(model=mid, H=H, N=2, n_ter=0, ter=None, z=_p(z), th=_p(th), Qq=_p(Qq), Qv=_p(Qv), Ru=_p(Ru), Us=100.0, Vs=100.0, K=_p(K), P1=None)
    order = ["model", "H", "N", "n_ter", "ter", "z", "th", "Qq", "Qv", "Ru", "Us", "Vs", "K", "P1"]
    th_bad_h = th.copy(); th_bad_h[1, -1] = 0.0
    bad = [dict(model=99), dict(model=9), dict(H=0), dict(N=0), dict(z=None), dict(th=None), dict(Qq=None), dict(Qv=None), dict(Ru=None), dict(K=None),
           dict(Us=0.0), dict(Vs=float("inf")), dict(n_ter=1), dict(ter=ter), dict(n_ter=3, ter=ter), dict(th=_p(th_bad_h)),
           dict(model=6)]                                   # particle_2D needs a terrain
    for over in bad:
        a = {**good, **over}
        assert lib.cimpc_reference_gains(*[a[k] for k in order]) == INVALID, over
    assert np.all(K == 7.0)


def test_handle_entries_refuse_a_null_handle():
    lib = _lib.load()
    a = np.zeros(8)
    assert lib.cimpc_set_gains(None, _p(a)) == INVALID
    assert lib.cimpc_gain_latch(None) == INVALID
    assert lib.cimpc_gain_feedback(None, _p(a), _p(a), 1.0, _p(a)) == INVALID


def test_python_wrappers_check_shapes_first():
    from contactimplicitmpc.jl_amd import gains
    with pytest.raises(ValueError):
        gains.tvlqr(np.zeros((1, 2, 2)), np.zeros((1, 2, 1)), np.zeros((1, 2, 2)), np.zeros((1, 1, 1)))      # nothing carries the horizon
    with pytest.raises(ValueError):
        gains.reference_gains("hopper_3D", np.zeros((2, 19)), np.ones((3, 22)), np.eye(7), np.eye(7), np.eye(3))
    with pytest.raises(KeyError):
        gains.reference_gains("no_such_model", np.zeros((2, 19)), np.ones((2, 22)), np.eye(7), np.eye(7), np.eye(3))


# ---- the exports ---------------------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NEW))
def test_export_is_declared_and_bound(name):
    params = _prototype(name)
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(params) == NEW[name]
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), name)
    assert _lib.load().cimpc_version() >= 108


@pytest.mark.parametrize("name", sorted(NEW))
def test_julia_call_matches_the_prototype(name):
    compat = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Terrain}": {"const cimpc_terrain*"},
              "Ptr{Cvoid}": {"cimpc_handle"}}
    fn_name = JL_FUNCTION[name]
    i = JL.find("function " + fn_name + "(")
    i = JL.index("\n" + fn_name + "(") if i < 0 else i              # a one-line definition
    fn = JL[i:]
    m = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint", fn, flags=re.S)
    m2 = re.search(r"ccall\(\(:" + name + r",\s*LIB\),\s*Cint,\s*\(([^()]*)\)", fn)
    assert m or m2, f"{fn_name} does not call {name}"
    if m and (not m2 or m.start() < m2.start()):
        types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    else:
        types = [a.strip() for a in m2.group(1).split(",") if a.strip()]
    params = _prototype(name)
    assert len(types) == len(params), f"{name}: {len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in compat[jt], f"{name} argument {k}: Julia {jt} against C `{ct}`"


def test_header_says_where_the_feedback_is_placed_and_which_models_are_singular():
    hdr = open(os.path.join(ROOT, "include", "cimpc.h")).read()
    assert "THE PLACEMENT IS THIS BUILD'S" in hdr and "continuous_policy_v3.jl:74-85" in hdr
    assert "planar models at their shipped gaits are singular" in hdr


def test_julia_set_gains_packs_the_vector_of_matrices_reference_gains_returns():
    """Julia cannot run here, so statically: `reference_gains` returns a vector of H matrices, `set_gains!` takes a vector of matrices,
    checks its length against H_ref and each size against (nu, 2nq), and hands the library ONE contiguous nu x 2nq x H_ref array built
    by `cat(K...; dims = 3)` - not `pack`, whose only method takes a vector of vectors."""
    rg = JL[JL.index("function reference_gains("):]
    rg = rg[:rg.index("\nend\n")]
    assert "return [K[:, :, t] for t = 1:H]" in rg
    fn = JL[JL.index("function set_gains!("):]
    fn = fn[:fn.index("\nend\n")]
    assert "K::Union{Nothing,AbstractVector{<:AbstractMatrix}}" in fn
    assert "length(K) == d.H_ref" in fn and "size(k) == (d.nu, 2 * d.nq)" in fn
    assert "cat(K...; dims = 3)" in fn and "pack(" not in fn
    calls = re.findall(r"ccall\(\(:cimpc_set_gains, LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}\), hs\.h, (\w+)\)", fn)
    assert calls == ["C_NULL", "Kc"]
    m = re.search(r"pack\(v::AbstractVector\{<:AbstractVector\}", JL)
    assert m and len(re.findall(r"\npack\(", JL)) == 1          # still the only method: a vector of matrices would not dispatch to it


def test_reference_gains_says_which_condition_of_the_linearization_it_missed():
    lib = _lib.load()
    nq, nu, nz, nth, H = 7, 3, 19, 22, 2                   # hopper_3D
    z, th = np.zeros((H, nz)), np.ones((H, nth))
    th_bad_h = th.copy(); th_bad_h[1, -1] = 0.0
    Qq, Qv, Ru, K = np.eye(nq), np.eye(nq), np.eye(nu), np.zeros((H, 2 * nq, nu))
    ter = (_lib.Terrain * 3)()
    call = lambda model, n_ter, t, theta: lib.cimpc_reference_gains(model, H, 2, n_ter, t, _p(z), _p(theta), _p(Qq), _p(Qv), _p(Ru), 100.0, 100.0, _p(K), None)
    for args, word in (((99, 0, None, th), "unknown plant model 99"), ((10, 3, ter, th), "neither 1 nor H"), ((10, 1, None, th), "do not go together"),
                       ((6, 0, None, th), "needs a terrain"), ((10, 0, None, th_bad_h), "h (the last entry")):
        assert call(*args) == INVALID
        assert word in lib.cimpc_last_error(None).decode(), (args[:2], lib.cimpc_last_error(None).decode())
