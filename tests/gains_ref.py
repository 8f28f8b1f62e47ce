"""NumPy restatement of the reference's src/controller/gains.jl (51 lines): `tvlqr` and `reference_gains`, with
`numpy.linalg.solve` (LAPACK gesv: LU with partial pivoting, what Julia's `\\` does on a square matrix) in both places.  The device
kernels of csrc/gains.hip are held to it (tests/test_gpu_gains.py); tests/test_gains.py holds IT to known answers.

Arrays are numpy's row-major M[i, j]; rz0[t][i, j] = dr_i/dz_j, rth0[t][i, j] = dr_i/dtheta_j as `ContactModel.linearize_batch` returns
them.  z = [q2; gamma; b; ...] and theta = [q0; q1; u1; w1; mu; h]: idx_z.q = 0 .. nq-1, idx_theta.q1 / .q2 / .u = the leading nq, nq, nu
columns (src/simulation/index.jl; the reference names theta's two configurations q1, q2).
"""
import numpy as np

LD = np.longdouble      # 64-bit mantissa on x86-64 (eps 1.1e-19): the extended-precision solves the float64 restatements are held to


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


def reference_gains_adjoint(nq, nu, rz0, rth0, obj_q, obj_v, obj_u, N=10, U_scaling=100.0, V_scaling=100.0, return_P1=False):
    """`reference_gains` in float64 in the ORDER of gains_dynamics_kernel: only the q rows of dz/dtheta are consumed, so nq right-hand
    sides go through rz' (Y = rz^-T I[:, :nq]) and D = -(Y' rtheta[:, :2nq+nu]) follows; then the same `tvlqr`."""
    H = len(rz0)
    AB = []
    for t in range(H):
        nz = rz0[t].shape[0]
        Y = np.linalg.solve(rz0[t].T, np.eye(nz)[:, :nq])
        D = -(Y.T @ rth0[t][:, :2 * nq + nu])
        AB.append((np.block([[np.zeros((nq, nq)), np.eye(nq)], [D[:, :nq], D[:, nq:2 * nq]]]), np.vstack([np.zeros((nq, nu)), D[:, 2 * nq:]])))
    A = [AB[t % H][0] for t in range(N * H)]
    B = [AB[t % H][1] for t in range(N * H)]
    Q, R = weights(np.asarray(obj_q, dtype=float), np.asarray(obj_v, dtype=float), np.asarray(obj_u, dtype=float), U_scaling, V_scaling)
    K, P = tvlqr(A, B, [Q] * (N * H + 1), [R] * (N * H))
    K = np.stack(K[:H])
    return (K, P[0]) if return_P1 else K


def row_interchanges(M):
    """The number of rows LAPACK's LU with partial pivoting (getrf) moves on M: the steps k whose pivot row is not k."""
    from scipy.linalg import lu_factor
    _, piv = lu_factor(np.asarray(M, dtype=float), check_finite=False)
    return int(np.count_nonzero(piv != np.arange(len(piv))))


# ---- the same recursions in numpy.longdouble ---------------------------------------------------------------------------------------
# No LAPACK and no BLAS exist for this type: the LU is written out below, and numpy's matmul on longdouble operands is its own plain
# loop, one running sum per entry (`mm_ld` refuses any other type, so that no product slips through dgemm).
def mm_ld(X, Y):
    assert X.dtype == LD and Y.dtype == LD
    return np.matmul(X, Y)


def solve_ld(M, rhs):
    """M \\ rhs in longdouble: LU with partial pivoting taking the FIRST largest |entry| of the column, then the two triangular
    solves.  A zero or non-finite pivot raises LinAlgError, as `numpy.linalg.solve` does on an exactly singular matrix."""
    W = np.array(M, dtype=LD)
    X = np.array(rhs, dtype=LD)
    vec = X.ndim == 1
    X = X.reshape(len(W), -1)
    n = len(W)
    for k in range(n):
        p = k + int(np.argmax(np.abs(W[k:, k])))          # argmax: the first of equals
        if p != k:
            W[[k, p]] = W[[p, k]]
            X[[k, p]] = X[[p, k]]
        pv = W[k, k]
        if not (np.isfinite(pv) and abs(pv) > 0):
            raise np.linalg.LinAlgError(f"zero or non-finite pivot at column {k}")
        l = W[k + 1:, k] / pv
        W[k + 1:, k + 1:] -= l[:, None] * W[k, k + 1:][None, :]
        X[k + 1:] -= l[:, None] * X[k][None, :]
    for k in range(n - 1, -1, -1):
        X[k] = (X[k] - mm_ld(W[k, k + 1:], X[k + 1:])) / W[k, k]
    return X[:, 0] if vec else X


def tvlqr_ld(A, B, Q, R):
    """`tvlqr` in longdouble; takes float64 or longdouble matrices, returns longdouble (K, P)."""
    A, B, Q, R = ([np.asarray(M, dtype=LD) for M in L] for L in (A, B, Q, R))
    T = len(Q)
    P = [None] * T
    K = [None] * (T - 1)
    P[T - 1] = Q[T - 1]
    for t in range(T - 2, -1, -1):
        BtP = mm_ld(B[t].T, P[t + 1])
        K[t] = solve_ld(R[t] + mm_ld(BtP, B[t]), mm_ld(BtP, A[t]))
        Acl = A[t] - mm_ld(B[t], K[t])
        P[t] = Q[t] + mm_ld(K[t].T, mm_ld(R[t], K[t])) + mm_ld(Acl.T, mm_ld(P[t + 1], Acl))
    return K, P


def dynamics_ld(nq, nu, rz, rth):
    dzdth = solve_ld(-np.asarray(rz, dtype=LD), np.asarray(rth, dtype=LD)[:, :2 * nq + nu])      # the columns that are read
    Z, I = np.zeros((nq, nq), dtype=LD), np.eye(nq, dtype=LD)
    A = np.block([[Z, I], [dzdth[:nq, :nq], dzdth[:nq, nq:2 * nq]]])
    B = np.vstack([np.zeros((nq, nu), dtype=LD), dzdth[:nq, 2 * nq:]])
    return A, B


def reference_gains_ld(nq, nu, rz0, rth0, obj_q, obj_v, obj_u, N=10, U_scaling=100.0, V_scaling=100.0, return_P1=False):
    """`reference_gains` in longdouble from float64 inputs."""
    H = len(rz0)
    AB = [dynamics_ld(nq, nu, rz0[t], rth0[t]) for t in range(H)]
    A = [AB[t % H][0] for t in range(N * H)]
    B = [AB[t % H][1] for t in range(N * H)]
    Q, R = weights(np.asarray(obj_q, dtype=LD), np.asarray(obj_v, dtype=LD), np.asarray(obj_u, dtype=LD), LD(U_scaling), LD(V_scaling))
    K, P = tvlqr_ld(A, B, [Q] * (N * H + 1), [R] * (N * H))
    K = np.stack(K[:H])
    return (K, P[0]) if return_P1 else K
