"""Multiple shooting without a device (csrc/plant_shooting.h): the header built with g++ and run by a team of one
against the ordered float64 restatement of tests/plant_shooting_ref.py bit for bit - the layout, the defects and their sum, the cost on the
segments' own rows, the merit - and within the bounds of the longdouble restatement; the same program under AddressSanitizer and UBSan;
`cimpc_plant_shooting_cost` through ctypes (`TrackingCost.evaluate_segments`); M = 1 against `TrackingCost.evaluate`; the host helpers
`segment_nodes` and `ShootingNominal.q_stitched`; and every refusal by name, before any device is touched.

Shapes: nq 3 nu 3 (B 2, T 8, M 1, 2, 4, 8), nq 4 nu 2 (B 3, T 12, M 1, 2, 3, 4, 12), nq 18 nu 12 (B 1, T 2, M 1, 2); M = T is among them.

Measured (this file's shapes): the host build and `cimpc_plant_shooting_cost` equal the restatement bit for bit at every shape, also under
the sanitizers; the figures of the restatement against longdouble are in tests/README_plant_shooting.md."""
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, plant
import plant_adjoint_cases as pac
import plant_riccati_cases as prc
import plant_shooting_cases as psc
import plant_shooting_ref as psr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "plant_shooting_check.cpp")
# name: (nq, nu, T, B, M, per-step weights, per-robot goals)
SHAPES = {f"nq {nq} T {T} B {B} M {M}": (nq, nu, T, B, M, per_step, per_robot)
          for (nq, nu, T, B, Ms, per_step, per_robot) in ((3, 3, 8, 2, (1, 2, 4, 8), False, False), (4, 2, 12, 3, (1, 2, 3, 4, 12), True, True),
                                                         (18, 12, 2, 1, (1, 2), False, True)) for M in Ms}
WEIGHT = 3.5


def _case(name):
    """(qs, u, M, Q, R, Qf, x_goal, u_goal); the weights are not symmetric, so that a transposed block shows."""
    nq, nu, T, B, M, per_step, per_robot = SHAPES[name]
    rng = np.random.default_rng([nq, nu, T, B, M])
    qs, u = psc.random_segments(rng, nq, nu, T, B, M)
    Q, R, Qf = prc.weights(rng, 2 * nq, nu, T, per_step)
    Q, R, Qf = Q + 0.1 * rng.standard_normal(Q.shape), R + 0.1 * rng.standard_normal(R.shape), Qf + 0.1 * rng.standard_normal(Qf.shape)
    nx = B if per_robot else 1
    return qs, u, M, Q, R, Qf, rng.standard_normal((T + 1, nx, 2 * nq)), rng.standard_normal((T, nx, nu))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    out = str(tmp_path_factory.mktemp("shooting") / "plant_shooting_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", out, SRC])
    return out


def _sanitized_build(tmp_path):
    """The check program under AddressSanitizer and UBSan.  Skips only where g++ or the sanitizers' runtimes are missing, which a trivial
    program shows; a failed build of the program itself fails the test."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    flags = ["-std=c++17", "-Wall", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    out = str(tmp_path / "plant_shooting_check_san")
    subprocess.check_call(["g++", *flags, "-o", out, SRC])
    return out


def _hex(*arrays):
    return " ".join(float(v).hex() for a in arrays for v in np.asarray(a, dtype=np.float64).reshape(-1))


def _run(exe, mode, text):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.strip("\n").split("\n")


def _run_cost(exe, qs, u, M, Q, R, Qf, xg, ug, weight=WEIGHT):
    T, B, nu = u.shape
    nq = qs.shape[2]
    col = lambda A: np.swapaxes(A, -1, -2)      # the header reads column-major blocks
    head = f"{B} {T} {M} {nq} {nu} {1 if Q.ndim == 2 else T} {1 if R.ndim == 2 else T} {xg.shape[1]} {float(weight).hex()} "
    lines = _run(exe, "cost", head + _hex(qs, u, col(Q), col(Qf), col(R), xg, ug))
    v = [np.array([float.fromhex(t) for t in line.split()]) for line in lines]
    while len(v) < 6:      # M = 1: the defects' line is empty and the split drops nothing, but guard the shape
        v.append(np.zeros(0))
    return v[0], v[1], v[2].reshape(M - 1, B, 2 * nq), v[3].reshape(T + 1, B, 2 * nq), v[4].reshape(T, B, nu), v[5]


def _bitwise(got, want, what):
    for name, g, w in zip(psr.NAMES, got, want):
        g, w = np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), f"{what}: {name} differs from the restatement"


# ---- the header against the restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_build_equals_the_ordered_restatement_and_meets_longdouble(exe, name):
    case = _case(name)
    got = _run_cost(exe, *case)
    ld, f64, bound = psr.cost_bounds(*case)
    _bitwise(got[:5], [f64[k] for k in psr.NAMES], name)
    assert got[5].tobytes() == psr.merit(f64["J"], WEIGHT, f64["D"]).tobytes(), "the merit is one rounded product and one rounded sum"
    for k, g in zip(psr.NAMES, got[:5]):
        dist = pac.distance(g, ld[k]) if g.size else 0.0
        print(f"{name}, {k}: {dist:.2e} from longdouble (bound {bound[k]:.2e})")
        assert dist <= bound[k], f"{name} {k}: {dist:.3e} > {bound[k]:.3e}"
    M = case[2]
    assert (np.abs(got[2]) > 0).all() and (got[1] > 0).all() if M > 1 else (got[1] == 0.0).all()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_layout_is_the_restatements(exe, name):
    nq, nu, T, B, M = SHAPES[name][:5]
    L = T // M
    pairs, rows = (np.array(line.split(), dtype=np.int64).reshape(-1, 2) for line in _run(exe, "layout", f"{B} {T} {M}"))
    entry = np.arange(L * M * B).reshape(L, M * B)
    np.testing.assert_array_equal(pairs[:, 0], entry.reshape(-1))
    np.testing.assert_array_equal(psr.stitch(entry, M).reshape(-1)[pairs[:, 1]], pairs[:, 0])      # entry (l, j, b) lands where stitch puts it
    assert sorted(pairs[:, 1].tolist()) == list(range(T * B))
    want = [(t // L, t % L) for t in range(T)] + [(M - 1, L)]
    assert [tuple(r) for r in rows.tolist()] == want


def test_one_segment_is_the_single_shooting_cost():
    """M = 1: no node, no defect, and J, lin_q, lin_r are `TrackingCost.evaluate`'s bits."""
    for name in sorted(SHAPES):
        qs, u, M, Q, R, Qf, xg, ug = _case(name)
        if M != 1:
            continue
        cost = plant.TrackingCost(Q, R, Qf, x_goal=xg, u_goal=ug)
        J, D, d, lq, lr = cost.evaluate_segments(qs, u, 1)
        J1, lq1, lr1 = cost.evaluate(qs, u)
        assert J.tobytes() == J1.tobytes() and lq.tobytes() == lq1.tobytes() and lr.tobytes() == lr1.tobytes()
        assert D.tolist() == [0.0] * u.shape[1] and d.shape == (0, u.shape[1], 2 * qs.shape[2])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_evaluate_segments_through_ctypes_equals_the_restatement(name):
    qs, u, M, Q, R, Qf, xg, ug = _case(name)
    got = plant.TrackingCost(Q, R, Qf, x_goal=xg, u_goal=ug).evaluate_segments(qs, u, M)
    _bitwise(got, psr.cost_f64(qs, u, M, Q, R, Qf, xg, ug), name)


def test_the_program_under_the_sanitizers(tmp_path):
    out = _sanitized_build(tmp_path)
    for name in sorted(SHAPES):
        case = _case(name)
        _bitwise(_run_cost(out, *case)[:5], psr.cost_f64(*case), name)


# ---- the host helpers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (1, 2, 3, 4, 12))
def test_nodes_of_a_trajectory_and_the_stitched_trajectory(M):
    T, B, nq = 12, 3, 4
    L = T // M
    q = np.random.default_rng(M).standard_normal((T + 2, B, nq))
    nodes = plant.segment_nodes(q, M)
    assert nodes.shape == (M, B, 2 * nq)
    for j in range(M):
        np.testing.assert_array_equal(nodes[j], np.concatenate([q[j * L], q[j * L + 1]], axis=1))
    # the segments a continuous trajectory is cut into: no defect, and stitching gives the trajectory back
    qs = np.zeros((L + 2, M * B, nq))
    for j in range(M):
        qs[:, j * B:(j + 1) * B] = q[j * L:j * L + L + 2]
    nom = plant.ShootingNominal(segments=M, qs=qs, nodes=nodes, u=None, gamma=None, b=None, status=None, iters=None, defects=None, D=None, tape=None)
    np.testing.assert_array_equal(nom.q_stitched(), q)
    np.testing.assert_array_equal(psr.defects(qs, M), 0.0)
    np.testing.assert_array_equal(psr.stage_states(qs, M), np.concatenate([q[:-1], q[1:]], axis=2))


# ---- refusals, by name, before any device is touched --------------------------------------------------------------------------------------------
def test_refusals_of_the_header_by_name(exe):
    assert _run(exe, "valid", "12 5 3") == ["T not divisible by segments"]
    assert _run(exe, "valid", "12 0 3") == ["segments below 1"]
    assert _run(exe, "valid", "12 13 3") == ["T not divisible by segments"]
    assert _run(exe, "valid", "0 1 3") == ["B or T below 1"]
    assert _run(exe, "valid", "12 12 3") == ["ok"] and _run(exe, "valid", "12 1 1") == ["ok"]
    nodes = np.zeros((2, 3, 8))
    assert _run(exe, "nodes", "2 3 4 " + _hex(nodes)) == ["ok"]
    nodes[1, 2, 5] = np.nan
    assert _run(exe, "nodes", "2 3 4 " + _hex(nodes)) == ["a non-finite entry of nodes"]
    nodes[1, 2, 5] = np.inf
    assert _run(exe, "nodes", "2 3 4 " + _hex(nodes)) == ["a non-finite entry of nodes"]


def test_refusals_of_the_python_surface_by_name():
    c = psc.problem("hopper_2D")
    nq = 4
    nodes = np.zeros((5, 3, 2 * nq))
    with pytest.raises(ValueError, match="T = 12 is not divisible by segments = 5"):
        plant.rollout_segments(c["model"], nodes, c["u"], c["h"], c["mu"], segments=5)
    with pytest.raises(ValueError, match=r"nodes must be \(segments, B, 8\)"):
        plant.rollout_segments(c["model"], nodes, c["u"], c["h"], c["mu"], segments=4)
    with pytest.raises(ValueError, match="segments must be at least 1"):
        plant.rollout_segments(c["model"], nodes[:0], c["u"], c["h"], c["mu"], segments=0)
    bad = np.zeros((4, 3, 2 * nq)); bad[2, 1, 3] = np.nan
    with pytest.raises(ValueError, match="nodes: a non-finite entry"):
        plant.rollout_segments(c["model"], bad, c["u"], c["h"], c["mu"], segments=4)
    cost = plant.TrackingCost(np.eye(2 * nq), np.eye(2))
    with pytest.raises(ValueError, match="T = 12 is not divisible by segments = 5"):
        cost.evaluate_segments(np.zeros((4, 15, nq)), c["u"], 5)
    with pytest.raises(ValueError, match="qs must be"):
        cost.evaluate_segments(np.zeros((4, 12, nq)), c["u"], 4)


def test_refusals_of_the_library_leave_their_reason_and_touch_no_device():
    """The C entries refuse with CIMPC_ERR_INVALID and name the reason in cimpc_last_error(NULL); this machine may have no device at all."""
    import ctypes as C
    lib = _lib.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    mid, nq, nu, nc, fd, nw = plant.model_dims("hopper_2D")
    B, T = 3, 12

    def call(M, nodes=None, tape=True, u=True):
        L = T // M if M >= 1 and T % M == 0 else 1
        nodes = np.zeros((max(M, 1), B, 2 * nq)) if nodes is None else nodes
        ua, mu, o = np.zeros((T, B, nu)), np.array([0.5]), _lib.IpOpts(**dataclasses.asdict(plant.SIM_OPTS))
        qs, g, b = np.zeros((L + 2, max(M, 1) * B, nq)), np.zeros((T, B, nc)), np.zeros((T, B, fd * nc))
        st, it, gst = (np.zeros((T, B), dtype=np.int32) for _ in range(3))
        d, D = np.zeros((max(M, 1), B, 2 * nq)), np.zeros(B)
        handle = C.c_void_p(1)
        rc = lib.cimpc_plant_rollout_segments(mid, B, T, M, 0, 0, None, dp(nodes), dp(ua) if u else None, None, 1, 1, 1, dp(mu), 1, 0.01, C.byref(o), None,
                                              1e-9, 2 * nq + nu, dp(qs), dp(g), dp(b), ip(st), ip(it), dp(d), dp(D), None, None, None, ip(gst),
                                              C.byref(handle) if tape else None)
        assert rc == -1, rc
        assert not tape or handle.value is None, "a refused call leaves a null tape"
        return lib.cimpc_last_error(None).decode()

    assert call(5) == "cimpc_plant_rollout_segments: T not divisible by segments"
    assert call(0) == "cimpc_plant_rollout_segments: segments below 1"
    assert call(4, tape=False) == "cimpc_plant_rollout_segments: null tape"
    assert call(4, u=False) == "cimpc_plant_rollout_segments: null u"
    bad = np.zeros((4, B, 2 * nq)); bad[3, 2, 7] = np.nan
    assert call(4, nodes=bad) == "cimpc_plant_rollout_segments: a non-finite entry of nodes"
    cost = plant.TrackingCost(np.eye(2 * nq), np.eye(nu))
    cc, keep = cost._struct(nq, nu, B, T)
    out = [np.zeros(B), np.zeros(B)]
    rc = lib.cimpc_plant_shooting_cost(nq, nu, B, T, 5, C.byref(cc), dp(np.zeros((4, 15, nq))), dp(np.zeros((T, B, nu))), dp(out[0]), dp(out[1]), None, None, None)
    assert rc == -1 and lib.cimpc_last_error(None).decode() == "cimpc_plant_shooting_cost: T not divisible by segments"


# ---- the backward pass with defects (csrc/plant_riccati.h: THE DEFECT HOOK) ---------------------------------------------------------------------
# name: (nq, nu, nr, n_cols, T, B, segments, per-step weights)
LQ_SHAPES = {f"nq {nq} T {T} B {B} M {M}": (nq, nu, nr, n_cols, T, B, M, per_step)
             for (nq, nu, nr, n_cols, T, B, Ms, per_step) in ((3, 3, 8, 11, 8, 2, (1, 2, 4, 8), False), (4, 2, 7, 10, 12, 3, (1, 2, 3, 4, 12), True),
                                                             (18, 12, 58, 53, 2, 1, (2,), False)) for M in Ms}
PATTERNS = ("all zero", "one nonzero defect", "every node, both halves")
MARGIN = 10.0      # over the restatement's distance at COPIES last-place copies of the inputs; the largest ratio seen is in tests/README_plant_shooting.md
COPIES = 16


def _lq_case(name, pattern, cut=False):
    """(D, status, (nq, nu, Q, R, Qf), q, r, rho (B,), defects (M - 1, B, n), L): seeded blocks whose columns outnumber the corner's."""
    nq, nu, nr, n_cols, T, B, M, per_step = LQ_SHAPES[name]
    n = 2 * nq
    rng = np.random.default_rng([nq, nu, T, B, M, PATTERNS.index(pattern)])
    D = rng.standard_normal((T, B, nr, n_cols)) / np.sqrt(n_cols)
    status = np.ones((T, B), dtype=np.int32)
    if cut and T > 2:
        D[T // 2, 0], status[T // 2, 0] = 0.0, 0
    Q, R, Qf = prc.weights(rng, n, nu, T, per_step)
    q, r = rng.standard_normal((T + 1, B, n)), rng.standard_normal((T, B, nu))
    d = np.zeros((M - 1, B, n))
    if pattern == "one nonzero defect" and M > 1:
        d[(M - 1) // 2, B - 1, nq + 1] = 1e-2
    if pattern == "every node, both halves":
        d = 1e-2 * rng.standard_normal(d.shape)
    return D, status, (nq, nu, Q, R, Qf), q, r, rng.uniform(0.0, 1e-3, B), d, T // M


def _run_lqr(exe, D, status, nq, nu, Q, R, Qf, q, r, rho, defects, L, shoot=True, lo=None, hi=None, u_nom=None):
    T, B, nr, n_cols = D.shape
    n, m = 2 * nq, nu
    cm = lambda A: np.swapaxes(np.asarray(A), -1, -2)      # the library's matrices are column-major
    n_lim = 0 if lo is None else lo.shape[0]
    head = f"{B} {T} {nq} {nu} {nr} {n_cols} {1 if Q.ndim == 2 else T} {1 if R.ndim == 2 else T} {T} {len(rho)} {n_lim} {L} {int(shoot)} "
    arrays = [cm(D), cm(Q), cm(Qf), cm(R), q, r, rho] + ([] if lo is None else [lo, hi, u_nom]) + ([defects] if shoot else [])
    lines = _run(exe, "lqr", head + " ".join(str(int(s)) for s in status.ravel()) + " " + _hex(*arrays))
    v = [np.array([float.fromhex(t) for t in line.split()]) for line in lines[:5]]
    ints = [np.array(line.split(), dtype=np.int32) for line in lines[5:8]]
    return dict(K=cm(v[0].reshape(T, B, n, m)), k=v[1].reshape(T, B, m), P0=cm(v[2].reshape(B, n, n)), p0=v[3].reshape(B, n), dV=v[4].reshape(B, 2),
                status=ints[0], n_cut=ints[1], clamped=ints[2].reshape(T, B))


def _lq_same(got, want, what, keys=prc.OUTPUTS):
    for k in keys:
        g, w = np.ascontiguousarray(got[k], dtype=np.float64), np.ascontiguousarray(want[k], dtype=np.float64)
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {k} differs"
    assert got["status"].tolist() == want["status"].tolist() and got["n_cut"].tolist() == want["n_cut"].tolist(), what


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", sorted(LQ_SHAPES))
def test_the_chain_with_the_hook_equals_the_ordered_restatement(exe, name, pattern):
    D, status, (nq, nu, Q, R, Qf), q, r, rho, d, L = _lq_case(name, pattern, cut=True)
    got = _run_lqr(exe, D, status, nq, nu, Q, R, Qf, q, r, rho, d, L)
    _lq_same(got, psr.lq_shoot_f64(D, status, nq, nu, Q, R, Qf, q, r, rho, d, L), f"{name}, {pattern}")
    assert got["status"].tolist() == [0] * D.shape[1] and not got["clamped"].any()
    plain = _run_lqr(exe, D, status, nq, nu, Q, R, Qf, q, r, rho, d, L, shoot=False)      # the limited chain as it was
    for b in range(D.shape[1]):      # robot by robot: lq_f64 takes one rho
        one = prc.lq_f64(D[:, b:b + 1], status[:, b:b + 1], nq, nu, Q, R, Qf, q=q[:, b:b + 1], r=r[:, b:b + 1], rho=rho[b])
        for k in prc.OUTPUTS:
            assert np.ascontiguousarray(plain[k].take([b], axis=0 if k in ("P0", "p0", "dV") else 1)).tobytes() == np.ascontiguousarray(one[k]).tobytes(), (name, k)
    if pattern == "all zero":
        _lq_same(got, plain, f"{name}: zero defects give the chain without the hook", keys=("K", "k", "P0", "dV"))
        assert np.array_equal(got["p0"], plain["p0"])      # as numbers: p + 0.0 may turn a -0.0 into 0.0
    elif D.shape[0] // L > 1:
        assert not np.array_equal(got["k"], plain["k"]), "a defect moves the feedforward"
        _lq_same(got, plain, f"{name}: the gains do not see the defects", keys=("K", "P0"))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", sorted(LQ_SHAPES))
def test_the_hook_solves_the_affine_lq_problem(name, pattern):
    """The gains of the restatement at rho 0, run through the linear forward pass, are the longdouble KKT solution of the affine LQ problem: the
    bound is MARGIN x the restatement's own distance from it at last-place copies of the inputs, never below MARGIN x 2.2e-16 x the
    problem's size.  This binds the RESTATEMENT (`lq_shoot_f64`), not the header, and passes whatever the header says: it shows that the
    rule the restatement states is the right one.  The header is bound to the restatement bit for bit by the test above, the kernel to the
    header on the device."""
    D, status, (nq, nu, Q, R, Qf), q, r, _, d, L = _lq_case(name, pattern)
    T, B = D.shape[:2]
    Qs, Rs, Qfs = (0.5 * (A + np.swapaxes(A, -1, -2)) for A in (Q, R, Qf))      # the KKT system takes the symmetric part; the chain the weights as given
    g = psr.lq_shoot_f64(D, status, nq, nu, Qs, Rs, Qfs, q, r, 0.0, d, L)
    assert g["status"].tolist() == [0] * B
    rng = np.random.default_rng(7)
    worst = 0.0
    for b in range(B):
        du_ref, dx_ref, _ = psr.lq_optimum_defects_ld(D, b, nq, nu, Qs, Rs, Qfs, q, r, d, L)
        du, dx = psr.forward_linear(D, b, nq, nu, g["K"], g["k"], d, L)
        dist = max(pac.distance(du, du_ref), pac.distance(dx[1:], dx_ref[1:]))
        own = 0.0
        for _ in range(COPIES):
            Dp, qp, rp, dp = (psr.last_place(rng, a) for a in (D, q, r, d))
            gp = psr.lq_shoot_f64(Dp, status, nq, nu, Qs, Rs, Qfs, qp, rp, 0.0, dp, L)
            dup, dxp = psr.forward_linear(Dp, b, nq, nu, gp["K"], gp["k"], dp, L)
            own = max(own, pac.distance(dup, du_ref), pac.distance(dxp[1:], dx_ref[1:]))
        bound = MARGIN * max(own, 2.2e-16 * T * 2 * nq)
        print(f"{name}, {pattern}, robot {b}: {dist:.2e} from the KKT solution, {own:.2e} at last-place copies, ratio {dist / max(own, 1e-300):.2f}, bound {bound:.2e}")
        assert dist <= bound
        worst = max(worst, dist)
    assert worst < 1e-9      # and small in absolute terms: a hook at the wrong step, or with the wrong sign, is off by the defect's own size


def test_the_chain_with_the_hook_under_limits_and_the_sanitizers(tmp_path):
    """The nu = 12 shape with per-robot limits that bind, and two more: the limited chain with the hook runs clean, clamps, and keeps
    clamped controls' rows of K at zero."""
    out = _sanitized_build(tmp_path)
    for name in ("nq 18 T 2 B 1 M 2", "nq 4 T 12 B 3 M 12", "nq 3 T 8 B 2 M 4"):
        D, status, (nq, nu, Q, R, Qf), q, r, rho, d, L = _lq_case(name, "every node, both halves")
        T, B = D.shape[:2]
        free = _run_lqr(out, D, status, nq, nu, Q, R, Qf, q, r, rho, d, L)
        _lq_same(free, psr.lq_shoot_f64(D, status, nq, nu, Q, R, Qf, q, r, rho, d, L), name)
        u_nom = np.zeros((T, B, nu))
        lim = 0.5 * np.abs(free["k"]).max(axis=(0, 2))[:, None] * np.ones((B, nu))      # per robot, half its largest feedforward
        box = _run_lqr(out, D, status, nq, nu, Q, R, Qf, q, r, rho, d, L, lo=-lim, hi=lim, u_nom=u_nom)
        assert box["status"].tolist() == [0] * B and box["clamped"].any()
        assert (np.abs(box["k"]) <= lim[None] * (1 + 1e-15)).all()
        for t, b in zip(*np.nonzero(box["clamped"])):
            for i in range(nu):
                if box["clamped"][t, b] >> i & 1:
                    assert not box["K"][t, b, i].any()


def test_lqr_with_defects_refuses_by_name_without_a_device():
    import ctypes as C
    lib = _lib.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    z = np.zeros(4096)
    i = np.zeros(64, dtype=np.int32)
    rc = lib.cimpc_plant_tape_lqr_shooting(None, 1, dp(z), dp(z), 1, dp(z), dp(z), dp(z), 1, dp(z), 1, dp(z), dp(z), dp(z), dp(z), dp(z), ip(i), ip(i), 1, None,
                                           None, None, None, 3, dp(z))
    assert rc == -1 and lib.cimpc_last_error(None).decode() == "cimpc_plant_tape_lqr_shooting: a null tape, Q, Qf, R, K, status, n_cut or rho"


# ---- the exports: header, ctypes and the Julia binding agree ------------------------------------------------------------------------------------
ENTRIES = ("cimpc_plant_rollout_segments", "cimpc_plant_shooting_cost", "cimpc_plant_tape_lqr_shooting", "cimpc_plant_shooting_forward", "cimpc_plant_shooting_linesearch")
JL_C = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*"}, "Ptr{Cvoid}": {"cimpc_plant_tape"},
        "Ref{Ptr{Cvoid}}": {"cimpc_plant_tape*"}, "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"},
        "Ref{TrackingCostC}": {"const cimpc_tracking_cost*"}, "Ptr{TrackingCostC}": {"const cimpc_tracking_cost*"}}


@pytest.mark.parametrize("name", ENTRIES)
def test_the_entries_are_declared_bound_and_called_from_julia_alike(name):
    import re
    root = os.path.dirname(HERE)
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "cimpc.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    c_args = [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]
    assert len(_lib.SIGNATURES[name][1]) == len(c_args) and hasattr(_lib.load(), name)
    jl = open(os.path.join(root, "julia", "CIMPCHip.jl")).read()
    call = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint\)", jl, flags=re.S)
    assert call, f"{name} has no @ccall in julia/CIMPCHip.jl"
    j_args = [a.split("::")[1].strip() for a in call.group(1).split(",")]
    assert len(j_args) == len(c_args), (len(j_args), len(c_args))
    for k, (jt, ct) in enumerate(zip(j_args, c_args)):
        assert ct in JL_C[jt], f"{name} argument {k}: Julia {jt} against C `{ct}`"


def test_every_rollout_argument_is_refused_by_its_own_reason():
    """What `cimpc_plant_rollout_segments` shares with `cimpc_plant_rollout_tape` is refused by name too, and a NaN anywhere in the nodes -
    node 0 included - by the nodes' reason, whatever else is wrong with the call."""
    import ctypes as C
    lib = _lib.load()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    mid, nq, nu, nc, fd, nw = plant.model_dims("hopper_2D")
    B, T, M = 3, 12, 4

    def call(nodes=None, h=0.01, n_mu=1, w=None, K_w=1, n_w=1, hold_w=1, n_cols=2 * nq + nu, reg=1e-9, max_iter=100, model=mid, n_terrain=0):
        nodes = np.zeros((M, B, 2 * nq)) if nodes is None else nodes
        o = _lib.IpOpts(**dataclasses.asdict(dataclasses.replace(plant.SIM_OPTS, max_iter=max_iter)))
        ua, mu = np.zeros((T, B, nu)), np.full(B, 0.5)
        qs, g, b = np.zeros((T // M + 2, M * B, nq)), np.zeros((T, B, nc)), np.zeros((T, B, fd * nc))
        st, it, gst = (np.zeros((T, B), dtype=np.int32) for _ in range(3))
        d, D = np.zeros((M, B, 2 * nq)), np.zeros(B)
        handle = C.c_void_p(1)
        rc = lib.cimpc_plant_rollout_segments(model, B, T, M, 0, n_terrain, None, dp(nodes), dp(ua), dp(w), K_w, n_w, hold_w, dp(mu), n_mu, h, C.byref(o), None,
                                              reg, n_cols, dp(qs), dp(g), dp(b), ip(st), ip(it), dp(d), dp(D), None, None, None, ip(gst), C.byref(handle))
        assert rc == -1 and handle.value is None
        return lib.cimpc_last_error(None).decode().split(": ", 1)[1]

    first = np.zeros((M, B, 2 * nq)); first[0, 0, 0] = np.nan
    assert call(nodes=first) == "a non-finite entry of nodes"
    assert call(nodes=first, h=-1.0) == "a non-finite entry of nodes"
    assert call(h=0.0) == "h not positive"
    assert call(n_mu=2) == "n_mu neither 1 nor B"
    assert call(w=np.zeros((2, 1, nw)), K_w=2, hold_w=0) == "K_w or hold_w below 1, or n_w neither 1 nor B"
    assert call(w=np.zeros((2, 2, nw)), K_w=2, n_w=2) == "K_w or hold_w below 1, or n_w neither 1 nor B"
    assert call(n_terrain=1) == "terrain and n_terrain do not go together"
    assert call(max_iter=0) == "interior-point options out of range"
    assert call(reg=-1.0) == "reg negative or not finite"
    assert call(n_cols=2 * nq + nu - 1) == "n_cols outside 2 nq + nu .. ntheta"
    assert call(model=99) == "an unknown model"


# ---- the linear forward pass (csrc/plant_shooting.h) --------------------------------------------------------------------------------------------
def _run_forward(exe, D, nq, nu, K, k, Q, R, Qf, lq, lr, d, L):
    T, B, nr, n_cols = D.shape
    n, m = 2 * nq, nu
    cm = lambda A: np.swapaxes(np.asarray(A), -1, -2)      # the library's matrices are column-major
    head = f"{B} {T} {nq} {nu} {nr} {n_cols} {1 if Q.ndim == 2 else T} {1 if R.ndim == 2 else T} {L} "
    lines = _run(exe, "forward", head + _hex(cm(D), cm(Q), cm(Qf), cm(R), lq, lr, cm(K), k, d))
    v = [np.array([float.fromhex(t) for t in line.split()]) for line in lines]
    return v[0].reshape(T // L - 1, B, n), v[1].reshape(T, B, m), v[2].reshape(B, 2)


def _forward_case(name, pattern):
    """A backward-pass case at rho 0 with symmetric weights and its gains from the restatement (a cut step among the blocks)."""
    D, status, (nq, nu, Q, R, Qf), q, r, _, d, L = _lq_case(name, pattern, cut=True)
    Q, R, Qf = (0.5 * (A + np.swapaxes(A, -1, -2)) for A in (Q, R, Qf))
    g = psr.lq_shoot_f64(D, status, nq, nu, Q, R, Qf, q, r, 0.0, d, L)
    assert g["status"].tolist() == [0] * D.shape[1]
    return D, nq, nu, g["K"], g["k"], Q, R, Qf, q, r, d, L


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", sorted(n for n in LQ_SHAPES if not n.endswith("M 1")))
def test_the_forward_chain_equals_the_ordered_restatement(exe, name, pattern):
    case = _forward_case(name, pattern)
    got, want = _run_forward(exe, *case), psr.forward_f64(*case)
    for what, g, w in zip(("dx_nodes", "du", "dJ"), got, want):
        assert g.shape == w.shape and g.tobytes() == np.ascontiguousarray(w).tobytes(), f"{name}, {pattern}: {what} differs from the restatement"
    if pattern == "all zero":      # no defect: the model's terms are the backward pass's dV, up to rounding (they are different chains)
        D, nq, nu, K, k, Q, R, Qf, q, r, d, L = case
        dV = psr.lq_shoot_f64(D, np.ones(D.shape[:2], dtype=np.int32), nq, nu, Q, R, Qf, q, r, 0.0, d, L)["dV"]
        np.testing.assert_allclose(got[2].sum(axis=1), dV.sum(axis=1), rtol=1e-9)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", sorted(n for n in LQ_SHAPES if not n.endswith("M 1")))
def test_the_models_terms_are_the_cost_difference_in_longdouble(name, pattern):
    """dJ1 + dJ2 of the restatement = J(x + dx, u + du) - J(x, u) of the quadratic cost in longdouble, about a trajectory with seeded errors
    ex_t = x_t - x_goal_t, eu_t = u_t - u_goal_t, whose linear terms lin_q[t] = Q_t ex_t, lin_r[t] = R_t eu_t go to the backward and the forward
    pass rounded to float64.  The bound is MARGIN x the restatement's own distance at last-place copies of the inputs, never below
    MARGIN x 2.2e-16 x the number of terms.  Like the test of the hook above, this binds the restatement; the header is bound to it bit for bit."""
    D, status, (nq, nu, Q, R, Qf), _, _, _, d, L = _lq_case(name, pattern, cut=True)
    Q, R, Qf = (0.5 * (A + np.swapaxes(A, -1, -2)) for A in (Q, R, Qf))
    T, B = D.shape[:2]
    LDt = np.longdouble
    rng = np.random.default_rng(11)
    ex, eu = rng.standard_normal((T + 1, B, 2 * nq)), rng.standard_normal((T, B, nu))
    Qs = np.concatenate([np.broadcast_to(Q, (T,) + Q.shape[-2:]), Qf[None]])
    Rs = np.broadcast_to(R, (T,) + R.shape[-2:])
    lq, lr = np.einsum("tij,tbj->tbi", Qs, ex), np.einsum("tij,tbj->tbi", Rs, eu)
    g = psr.lq_shoot_f64(D, status, nq, nu, Q, R, Qf, lq, lr, 0.0, d, L)
    assert g["status"].tolist() == [0] * B
    K, k = g["K"], g["k"]
    cost = lambda a, c: LDt(0.5) * (np.einsum("ti,tij,tj->", a, Qs.astype(LDt), a) + np.einsum("ti,tij,tj->", c, Rs.astype(LDt), c))
    got = psr.forward_f64(D, nq, nu, K, k, Q, R, Qf, lq, lr, d, L)[2]
    copies = []
    for _ in range(COPIES):
        Dp, Kp, kp, lqp, lrp, dp = (psr.last_place(rng, a) for a in (D, K, k, lq, lr, d))
        copies.append(psr.forward_f64(Dp, nq, nu, Kp, kp, Q, R, Qf, lqp, lrp, dp, L)[2])
    for b in range(B):
        du, dx = psr.forward_linear(D, b, nq, nu, K, k, d, L)
        want = cost(ex[:, b].astype(LDt) + dx, eu[:, b].astype(LDt) + du) - cost(ex[:, b].astype(LDt), eu[:, b].astype(LDt))
        dist = float(abs(LDt(got[b, 0]) + LDt(got[b, 1]) - want) / abs(want))
        own = max(float(abs(LDt(c[b, 0]) + LDt(c[b, 1]) - want) / abs(want)) for c in copies)
        bound = MARGIN * max(own, 2.2e-16 * T * (2 * nq + nu))
        print(f"{name}, {pattern}, robot {b}: dJ1 + dJ2 {dist:.2e} from the longdouble difference, {own:.2e} at last-place copies, ratio {dist / max(own, 1e-300):.2f}")
        assert dist <= bound


def test_the_forward_chain_under_the_sanitizers(tmp_path):
    out = _sanitized_build(tmp_path)
    for name in ("nq 18 T 2 B 1 M 2", "nq 4 T 12 B 3 M 12", "nq 3 T 8 B 2 M 4"):
        case = _forward_case(name, "every node, both halves")
        for g, w in zip(_run_forward(out, *case), psr.forward_f64(*case)):
            assert g.tobytes() == np.ascontiguousarray(w).tobytes(), name


# ---- the line search's rules and the loop's refusals -------------------------------------------------------------------------------------------
def test_acceptance_and_choice_equal_the_restatement(exe):
    rng = np.random.default_rng(21)
    for B, na in ((1, 1), (3, 4), (2, 7)):
        alphas = np.sort(rng.uniform(0.0, 1.0, na))[::-1].copy()
        weight, armijo = rng.uniform(0.0, 5.0, B), 1e-4
        J, D = rng.uniform(1.0, 2.0, (na, B)), rng.uniform(0.0, 1e-2, (na, B))
        conv = (rng.random((na, B)) < 0.8).astype(np.int32)
        phi_nom, D_nom = rng.uniform(1.0, 2.0, B), rng.uniform(0.0, 1e-1, B)
        dJ = np.stack([-rng.uniform(0.0, 1.0, B), rng.uniform(0.0, 0.5, B)], axis=1)
        J[0, 0] = np.nan                                        # a candidate whose cost is not a number is never acceptable
        if na > 2:
            J[2, :], D[2, :] = J[1, :], D[1, :]                 # a tie: the lower index wins
        lines = _run(exe, "accept", f"{na} {B} {float(armijo).hex()} " + _hex(alphas, weight) + " " + " ".join(str(int(v)) for v in conv.ravel()) + " " +
                     _hex(J, D, phi_nom, D_nom, dJ))
        phi = np.array([float.fromhex(t) for t in lines[0].split()]).reshape(na, B)
        ok, choice = np.array(lines[1].split(), dtype=int).reshape(na, B), np.array(lines[2].split(), dtype=int)
        w_phi, w_ok, w_choice = psr.linesearch_rules(alphas, weight, conv, J, D, phi_nom, D_nom, dJ, armijo)
        assert phi.tobytes() == w_phi.tobytes() and ok.tolist() == w_ok.astype(int).tolist() and choice.tolist() == w_choice.tolist()
        assert not ok[0, 0]
        # one segment: no defect, the weight passed as 0.0 - plant_cost.h's rules to the bit
        import plant_linesearch_cases as plc
        zero = np.zeros(B)
        lines = _run(exe, "accept", f"{na} {B} {float(armijo).hex()} " + _hex(alphas, zero) + " " + " ".join(str(int(v)) for v in conv.ravel()) + " " +
                     _hex(J, np.zeros((na, B)), phi_nom, zero, dJ))
        ok1 = np.array(lines[1].split(), dtype=int).reshape(na, B)
        want = [[plc.acceptable(conv[c, b], J[c, b], phi_nom[b], armijo, alphas[c], dJ[b, 0], dJ[b, 1]) for b in range(B)] for c in range(na)]
        assert ok1.tolist() == np.array(want).astype(int).tolist()
        assert np.array(lines[2].split(), dtype=int).tolist() == [plc.choose(J[:, b], np.array(want)[:, b]) for b in range(B)]
    x, a, dx = rng.standard_normal(50), rng.uniform(0, 1, 50), rng.standard_normal(50)
    got = np.array([float.fromhex(t) for t in _run(exe, "node", "50 " + _hex(np.stack([x, a, dx], axis=1)))[0].split()])
    assert got.tobytes() == (x + a * dx).tobytes()


def test_ilqr_shooting_refuses_a_missing_weight_or_tolerance_by_name():
    c = psc.problem("hopper_2D")
    cost = plant.TrackingCost(np.eye(8), np.eye(2))
    args = (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"], cost)
    with pytest.raises(ValueError, match="^defect_weight: required with segments > 1"):
        plant.ilqr_shooting(*args, segments=3, defect_tol=1e-6)
    with pytest.raises(ValueError, match="^defect_tol: required with segments > 1"):
        plant.ilqr_shooting(*args, segments=3, defect_weight=10.0)
    with pytest.raises(ValueError, match="T = 12 is not divisible by segments = 5"):
        plant.ilqr_shooting(*args, segments=5, defect_weight=10.0, defect_tol=1e-6)
    with pytest.raises(ValueError, match="segments must be at least 1"):
        plant.ilqr_shooting(*args, segments=0)
    with pytest.raises(ValueError, match="q_guess must be"):
        plant.ilqr_shooting(*args, segments=3, defect_weight=10.0, defect_tol=1e-6, q_guess=np.zeros((13, 3, 4)))
