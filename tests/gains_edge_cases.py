"""Synthetic inputs that take the gain kernels (csrc/gains.hip) to the edges their real-model cases (tests/gains_cases.py) do not reach,
with the answers of three references each: the longdouble solve, and the float64 restatement in the direct and in the kernel's adjoint
order (tests/gains_ref.py).  Shared by tests/test_gains_edges.py (which holds the INPUTS to their conditions without a device),
tests/test_gpu_gains_edges.py and scripts/gains_parity.py --edges.  Everything is seeded, computed once and read-only.

`reference_gains_lin` inputs: rz[t] = (2I + G/sqrt(nz))[:, perm] with G standard normal and a random column permutation - cond 4-6, and
the LU of rz' (what gains_dynamics_kernel factors) interchanges rows at nearly every column; rtheta[t] standard normal; the weights
obj_q = 2I + G/sqrt(nq), obj_v, obj_u the same form scaled by 1e-2 are NOT symmetric, so a transposed weight changes the answer.

`tvlqr` inputs: A = G/sqrt(n), B = 0.3 G/sqrt(n), Q = I + XX'/n (SPD), R_t = 20 (2I + G/sqrt(m))[perm] with its ROWS permuted (and not
by the identity when m >= 2): R + B'PB is then not symmetric and its largest entries are off the diagonal, so the LU of tvlqr_kernel
swaps rows - which no SPD weight makes it do."""
import functools

import numpy as np

import gains_ref

# (nq, nu, nz, ntheta, H, N)
LIN_SHAPES = [
    (1, 1, 1, 3, 1, 1),            # the smallest call there is: nz = nq = 1, one knot, one step
    (2, 1, 2, 5, 2, 3),
    (7, 3, 63, 19, 2, 2),          # one short of the 64-lane pivot search: an empty lane in the first column
    (7, 3, 64, 17, 2, 2),          # ntheta = 2nq + nu exactly
    (7, 3, 65, 21, 2, 2),          # one past it
    (5, 16, 40, 30, 2, 2),         # m > n; nz < 64
    (24, 16, 24, 64, 2, 2),        # nz = nq; nq = 24 is the most the back substitution's 32 column lanes take
    (24, 16, 128, 64, 2, 2),
    (24, 16, 131, 66, 2, 2),       # 163 504 B of LDS: the most the validator lets through at nq = 24
    (1, 1, 142, 5, 2, 2),          # 163 600 B: the most it lets through at all (the cap is 163 840 B)
    (23, 15, 97, 61, 3, 1),        # odd everything
    (3, 2, 9, 10, 300, 1),         # more knots (workgroups) than CUs, a chain of 300 steps
]
LIN_NAMES = ["nq=%d nu=%d nz=%d nth=%d H=%d N=%d" % s for s in LIN_SHAPES]
LDS_MAX_SHAPES = [(24, 131), (1, 142)]      # (nq, nz): the largest that fit; one more column of rz is refused
LDS_OVER_SHAPES = [(24, 132), (1, 143)]

# (n, m, T, n_ab), each with constant Q and with n_q = T
TVLQR_SHAPES = [(1, 1, 2, 1), (1, 1, 7, 3), (2, 16, 5, 2), (48, 1, 5, 3), (47, 15, 4, 7), (48, 16, 3, 1), (17, 7, 6, 2), (16, 4, 9, 9), (13, 5, 9, 3)]
TVLQR_NAMES = ["n=%d m=%d T=%d n_ab=%d %s" % (s + (q,)) for s in TVLQR_SHAPES for q in ("Q const", "n_q=T")]
BATCH_3 = (3, 13, 5, 9, 3)         # (n_prob, n, m, T, n_ab) with n_q = T, n_r = T - 1, called with n_keep = 4
BATCH_3_KEEP = 4
BATCH_300 = (300, 6, 2, 5, 2)      # more problems than CUs
ERRORS_SHAPE = (7, 3, 65, 21, 5, 2)      # the input the error-return tests damage: 5 knots, two wavefronts of pivot rows, unread rtheta columns


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _seed(*key):
    return np.random.default_rng([20240611, *key])


def _shifted(rng, k, scale=1.0):
    return scale * (2.0 * np.eye(k) + rng.standard_normal((k, k)) / np.sqrt(k))


@functools.lru_cache(maxsize=None)
def lin_inputs(shape):
    """dict(nq, nu, nz, nth, H, N, rz0 (H, nz, nz), rth0 (H, nz, nth), weights) for a (nq, nu, nz, nth, H, N)."""
    nq, nu, nz, nth, H, N = shape
    rng = _seed(1, *shape)
    rz0 = np.stack([_shifted(rng, nz)[:, rng.permutation(nz)] for _ in range(H)])
    rth0 = rng.standard_normal((H, nz, nth))
    w = (_shifted(rng, nq), _shifted(rng, nq, 1e-2), _shifted(rng, nu, 1e-2))
    for a in w:
        a.setflags(write=False)
    return _freeze(dict(nq=nq, nu=nu, nz=nz, nth=nth, H=H, N=N, rz0=rz0, rth0=rth0, weights=w))


def _rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def lin_case(name):
    """The inputs of `lin_inputs` with K_ld, P1_ld (the longdouble solve) and the float64 restatements' own distances to it, max|x - ld| /
    max|ld|: d_direct, d_adjoint (K, P1 each)."""
    c = dict(lin_inputs(LIN_SHAPES[LIN_NAMES.index(name)]))
    args = (c["nq"], c["nu"], c["rz0"], c["rth0"], *c["weights"])
    K_ld, P_ld = gains_ref.reference_gains_ld(*args, N=c["N"], return_P1=True)
    K_d, P_d = gains_ref.reference_gains(*args, N=c["N"], return_P1=True)
    K_a, P_a = gains_ref.reference_gains_adjoint(*args, N=c["N"], return_P1=True)
    c.update(K_ld=K_ld, P1_ld=P_ld, d_direct=(_rel(K_d, K_ld), _rel(P_d, P_ld)), d_adjoint=(_rel(K_a, K_ld), _rel(P_a, P_ld)))
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def tvlqr_inputs(n_prob, n, m, T, n_ab, varying_q):
    """A (n_prob, n_ab, n, n), B (n_prob, n_ab, n, m), Q (n_prob, T or 1, n, n), R (n_prob, T - 1, m, m)."""
    rng = _seed(2, n_prob, n, m, T, n_ab, int(varying_q))
    A = rng.standard_normal((n_prob, n_ab, n, n)) / np.sqrt(n)
    B = 0.3 * rng.standard_normal((n_prob, n_ab, n, m)) / np.sqrt(n)
    X = rng.standard_normal((n_prob, T if varying_q else 1, n, n))
    Q = np.eye(n) + X @ np.swapaxes(X, -1, -2) / n
    R = np.empty((n_prob, T - 1, m, m))
    for p in range(n_prob):
        for t in range(T - 1):
            perm = rng.permutation(m)
            while m >= 2 and np.array_equal(perm, np.arange(m)):      # "permuted" means moved
                perm = rng.permutation(m)
            R[p, t] = _shifted(rng, m, 20.0)[perm]
    return _freeze(dict(n=n, m=m, T=T, n_ab=n_ab, A=A, B=B, Q=Q, R=R))


def chain(c, p):
    """Problem p's lists as gains_ref.tvlqr takes them: T - 1 of A, B, R, T of Q."""
    T, n_ab, n_q = c["T"], c["n_ab"], c["Q"].shape[1]
    return ([c["A"][p, t % n_ab] for t in range(T - 1)], [c["B"][p, t % n_ab] for t in range(T - 1)],
            [c["Q"][p, t % n_q] for t in range(T)], [c["R"][p, t] for t in range(T - 1)])


def _with_refs(c):
    """K_ld (n_prob, T - 1, m, n), P1_ld (n_prob, n, n), d_f64 (n_prob, 2): the float64 `tvlqr`'s distance to the longdouble one; and
    G (n_prob, T - 1, m, m): the matrix R_t + B'P[t+1]B each step factors, from the longdouble P."""
    c = dict(c)
    n_prob = c["A"].shape[0]
    K_ld, P_ld, d, G = [], [], [], []
    for p in range(n_prob):
        A, B, Q, R = chain(c, p)
        K, P = gains_ref.tvlqr_ld(A, B, Q, R)
        Kf, Pf = gains_ref.tvlqr(A, B, Q, R)
        K_ld.append(np.stack(K)); P_ld.append(P[0])
        d.append((_rel(np.stack(Kf), np.stack(K)), _rel(Pf[0], P[0])))
        G.append(np.stack([np.asarray(R[t] + B[t].T @ P[t + 1] @ B[t], dtype=float) for t in range(c["T"] - 1)]))
    c.update(K_ld=np.stack(K_ld), P1_ld=np.stack(P_ld), d_f64=np.array(d), G=np.stack(G))
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def tvlqr_case(name):
    i = TVLQR_NAMES.index(name)
    return _with_refs(tvlqr_inputs(1, *TVLQR_SHAPES[i // 2], bool(i % 2)))


@functools.lru_cache(maxsize=None)
def batch_case(which):
    n_prob, n, m, T, n_ab = {"3": BATCH_3, "300": BATCH_300}[which]
    return _with_refs(tvlqr_inputs(n_prob, n, m, T, n_ab, which == "3"))


def bound(*d):
    """The parity bound of a device figure from the float64 restatements' own distances to the longdouble solve: 100 x the largest of
    them (and of one float64 unit), never more than the tolerance of the real-model cases.  100 x because the kernel is a third
    summation order, with FMA; the two CPU orders differ from each other by at most 3 x on these inputs."""
    import gains_cases as gc
    return min(gc.TOL, 100.0 * max(*d, 2.2e-16))
