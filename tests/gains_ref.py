"""NumPy restatement of the reference's src/controller/gains.jl (51 lines): `tvlqr` and `reference_gains`, with
`numpy.linalg.solve` (LAPACK gesv: LU with partial pivoting, what Julia's `\\` does on a square matrix) in both places.  The device
kernels of csrc/gains.hip are held to it (tests/test_gpu_gains.py); tests/test_gains.py holds IT to known answers.

Arrays are numpy's row-major M[i, j]; rz0[t][i, j] = dr_i/dz_j, rth0[t][i, j] = dr_i/dtheta_j as `ContactModel.linearize_batch` returns
them.  z = [q2; gamma; b; ...] and theta = [q0; q1; u1; w1; mu; h]: idx_z.q = 0 .. nq-1, idx_theta.q1 / .q2 / .u = the leading nq, nq, nu
columns (src/simulation/index.jl; the reference names theta's two configurations q1, q2).
"""
import numpy as np


def tvlqr(A, B, Q, R):
    """gains.jl:1-15.  A, B: lists of T-1 matrices; Q: T; R: T-1.  Returns (K, P): T-1 gains, T cost-to-go matrices."""
    T = len(Q)                                                                    # :2
    P = [np.zeros_like(A[0]) for _ in range(T)]                                   # :4
    K = [np.zeros_like(B[0].T) for _ in range(T - 1)]                             # :5
    P[T - 1] = Q[T - 1]                                                           # :6
    for t in range(T - 2, -1, -1):                                                # :8
        K[t] = np.linalg.solve(R[t] + B[t].T @ P[t + 1] @ B[t], B[t].T @ P[t + 1] @ A[t])          # :9
        Acl = A[t] - B[t] @ K[t]
        P[t] = Q[t] + K[t].T @ R[t] @ K[t] + Acl.T @ P[t + 1] @ Acl               # :10-11 (P is not symmetrized)
    return K, P                                                                   # :14


def dynamics(nq, nu, rz, rth):
    """One knot's A_t, B_t (gains.jl:31-42): dz/dtheta = -rz \\ rtheta, its q rows against the q1, q2, u columns."""
    dzdth = np.linalg.solve(-rz, rth)                                             # :31
    D1, D2, Du = dzdth[:nq, :nq], dzdth[:nq, nq:2 * nq], dzdth[:nq, 2 * nq:2 * nq + nu]      # :35-36, :39
    A = np.block([[np.zeros((nq, nq)), np.eye(nq)], [D1, D2]])                    # :33-34, :41
    B = np.vstack([np.zeros((nq, nu)), Du])                                       # :38, :42
    return A, B


def weights(obj_q, obj_v, obj_u, U_scaling=100.0, V_scaling=100.0):
    """gains.jl:43-47: the state weight couples the two configurations through the velocity weight."""
    Q = np.block([[obj_q + V_scaling * obj_v, -V_scaling * obj_v], [-V_scaling * obj_v, obj_q + V_scaling * obj_v]])
    return Q, U_scaling * obj_u


def reference_gains(nq, nu, rz0, rth0, obj_q, obj_v, obj_u, N=10, U_scaling=100.0, V_scaling=100.0, return_P1=False):
    """gains.jl:17-51 from the linearization of the H knots: they are repeated N times as they stand (:22-23: no stride shift, so the
    chain is H-periodic), K[1:H] comes back (:50)."""
    H = len(rz0)
    AB = [dynamics(nq, nu, rz0[t], rth0[t]) for t in range(H)]
    A = [AB[t % H][0] for t in range(N * H)]
    B = [AB[t % H][1] for t in range(N * H)]
    Q, R = weights(np.asarray(obj_q, dtype=float), np.asarray(obj_v, dtype=float), np.asarray(obj_u, dtype=float), U_scaling, V_scaling)
    K, P = tvlqr(A, B, [Q] * (N * H + 1), [R] * (N * H))                          # :49
    K = np.stack(K[:H])
    return (K, P[0]) if return_P1 else K
