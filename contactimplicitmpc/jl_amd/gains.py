"""Time-varying LQR feedback gains along the reference on the device (`csrc/gains.hip`): `tvlqr` and `reference_gains` of the
reference's src/controller/gains.jl:1-51 behind a numpy interface.

All arrays here are numpy's row-major `M[i, j]`; the library's matrices are column-major, so every matrix crosses the boundary
transposed.  There is no CPU fallback: the NumPy restatement the tests compare with lives in tests/gains_ref.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _check(lib, rc, what):
    if rc != 0:
        raise _lib.CimpcError(f"{what} failed ({rc}): {lib.cimpc_last_error(None).decode()}")


def _cm(a, shape):
    """(..., r, c) row-major -> contiguous stack of column-major r x c matrices."""
    a = np.asarray(a, dtype=np.float64).reshape(shape)
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


def tvlqr(A, B, Q, R, n_keep=None):
    """`tvlqr(A, B, Q, R)` (gains.jl:1-15) for one problem or a batch of equal-sized ones.
    A (n_ab, n, n) or (n_prob, n_ab, n, n); B (.., n_ab, n, m); step t (0-based) of the T - 1 steps uses A[t % n_ab], B[t % n_ab].
    Q (T, n, n) or (1, n, n) with T given by R; R (T - 1, m, m), or (1, m, m) when Q carries T.  One of Q, R must carry the horizon.
    Returns (K, P1): K (.., n_keep, m, n), the first n_keep (default T - 1) gains, and P1 (.., n, n) = P[1]."""
    A, B, Q, R = (np.asarray(x, dtype=np.float64) for x in (A, B, Q, R))
    batched = A.ndim == 4
    if not batched:
        A, B, Q, R = A[None], B[None], Q[None], R[None]
    n_prob, n_ab, n, _ = A.shape
    m = B.shape[-1]
    n_q, n_r = Q.shape[1], R.shape[1]
    if n_q > 1:
        T = n_q
    elif n_r > 1:
        T = n_r + 1
    else:
        raise ValueError("Q (T matrices) or R (T - 1 matrices) must carry the horizon; for constant weights repeat one of them")
    n_keep = T - 1 if n_keep is None else int(n_keep)
    lib = _lib.load()
    Ac, Bc, Qc, Rc = _cm(A, (n_prob, n_ab, n, n)), _cm(B, (n_prob, n_ab, n, m)), _cm(Q, (n_prob, n_q, n, n)), _cm(R, (n_prob, n_r, m, m))
    K = np.zeros((n_prob, max(n_keep, 0), n, m))          # column-major m x n
    P1 = np.zeros((n_prob, n, n))
    _check(lib, lib.cimpc_tvlqr(n_prob, n, m, T, n_ab, _dp(Ac), _dp(Bc), n_q, _dp(Qc), n_r, _dp(Rc), n_keep, _dp(K), _dp(P1)), "cimpc_tvlqr")
    K, P1 = np.ascontiguousarray(K.transpose(0, 1, 3, 2)), np.ascontiguousarray(P1.transpose(0, 2, 1))
    return (K, P1) if batched else (K[0], P1[0])


def _weights(nq, nu, obj_q, obj_v, obj_u):
    f = lambda a, k: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(k, k).T)
    return f(obj_q, nq), f(obj_v, nq), f(obj_u, nu)


def reference_gains_lin(nq, nu, rz0, rth0, obj_q, obj_v, obj_u, N=10, U_scaling=100.0, V_scaling=100.0, return_P1=False):
    """`reference_gains` (gains.jl:17-51) from a linearization made elsewhere: rz0 (H, nz, nz), rth0 (H, nz, nθ) with
    rz0[t][i, j] = ∂r_i/∂z_j (what `ContactModel.linearize_batch` and `plant.linearize` return); obj_q, obj_v (nq, nq), obj_u (nu, nu)
    = obj.q[1], obj.v[1], obj.u[1].  Returns K (H, nu, 2nq), with P1 (2nq, 2nq) behind it if asked for."""
    rz0, rth0 = np.asarray(rz0, dtype=np.float64), np.asarray(rth0, dtype=np.float64)
    H, nz, nth = rth0.shape
    Qq, Qv, Ru = _weights(nq, nu, obj_q, obj_v, obj_u)
    lib = _lib.load()
    K = np.zeros((H, 2 * nq, nu))
    P1 = np.zeros((2 * nq, 2 * nq)) if return_P1 else None
    _check(lib, lib.cimpc_reference_gains_lin(int(nq), int(nu), nz, nth, H, int(N), _dp(_cm(rz0, (H, nz, nz))), _dp(_cm(rth0, (H, nz, nth))),
                                              _dp(Qq), _dp(Qv), _dp(Ru), float(U_scaling), float(V_scaling), _dp(K), _dp(P1)),
           "cimpc_reference_gains_lin")
    K = np.ascontiguousarray(K.transpose(0, 2, 1))
    return (K, np.ascontiguousarray(P1.T)) if return_P1 else K


def reference_gains(model_name, z, theta, obj_q, obj_v, obj_u, N=10, U_scaling=100.0, V_scaling=100.0, terrain=None, return_P1=False):
    """`reference_gains(s, traj, obj; N, U_scaling, V_scaling)` from (z, θ) alone: the device plant model `model_name` linearized at
    every knot, dz/dθ, the Riccati chain - all on the device.  z (H, nz), theta (H, nθ) as `plant.linearize` takes them; terrain as
    there.  Returns K (H, nu, 2nq), with P1 behind it if asked for."""
    from . import plant
    if terrain is None and model_name in plant.TERRAIN_MODELS:
        terrain = "flat_2D_lc"
    mid, nq, nu, nc, fd, nw = plant.model_dims(model_name)
    nz, nth = nq + 4 * nc + 2 * fd * nc, 2 * nq + nu + nw + 2
    za = np.ascontiguousarray(np.asarray(z, dtype=np.float64).reshape(-1, nz))
    ta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(-1, nth))
    H = za.shape[0]
    if H < 1 or ta.shape[0] != H:
        raise ValueError(f"z must be (H, {nz}) and theta (H, {nth}) with the same H >= 1")
    Qq, Qv, Ru = _weights(nq, nu, obj_q, obj_v, obj_u)
    ter, nt = (None, 0) if terrain is None else plant._terrain_array(terrain, H)
    lib = _lib.load()
    K = np.zeros((H, 2 * nq, nu))
    P1 = np.zeros((2 * nq, 2 * nq)) if return_P1 else None
    _check(lib, lib.cimpc_reference_gains(mid, H, int(N), nt, ter, _dp(za), _dp(ta), _dp(Qq), _dp(Qv), _dp(Ru), float(U_scaling),
                                          float(V_scaling), _dp(K), _dp(P1)), "cimpc_reference_gains")
    K = np.ascontiguousarray(K.transpose(0, 2, 1))
    return (K, np.ascontiguousarray(P1.T)) if return_P1 else K


def gait_feedback(q_ref, K, N_sample: int = 1, n_sample=None):
    """A gait and its `reference_gains` output as the `plant.Feedback` of a closed-loop rollout at N_sample simulator steps per knot:
    q_ref (H + 2, nq) the gait's configurations (`gait_io.Gait.q`), K (H, nu, 2nq); x_ref[k] = [q_ref[k]; q_ref[k + 1]], the target of the
    policy's feedback line at knot k (H-periodic: q_ref[H], q_ref[H + 1] close the cycle), every row held for N_sample steps and the last
    from there on.  A rollout longer than H N_sample steps takes a K and x_ref tiled by the caller."""
    from . import plant
    q_ref, K = np.asarray(q_ref, dtype=np.float64), np.asarray(K, dtype=np.float64)
    H = K.shape[0]
    if K.ndim != 3 or q_ref.ndim != 2 or q_ref.shape[0] != H + 2 or K.shape[2] != 2 * q_ref.shape[1]:
        raise ValueError("q_ref must be (H + 2, nq) beside K (H, nu, 2nq)")
    x_ref = np.concatenate([q_ref[:H], q_ref[1:H + 1]], axis=1)
    return plant.Feedback(K=K, x_ref=x_ref, hold=int(N_sample), n_sample=n_sample)
