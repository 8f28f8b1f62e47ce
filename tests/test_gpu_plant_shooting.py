"""Multiple shooting on the device (csrc/plant_shooting.hip: `plant.rollout_segments`, `ShootingNominal`, `TrackingCost.evaluate_segments`;
DESIGN.md section 3, item 3l) against the calls it is made of, bit for bit.  Shapes: tests/plant_shooting_cases.py - the particles in flight
(B 2, T 8, M 1, 2, 4, 8), the hoppers through contact (B 3, T 12, M 1, 2, 3, 4, 12; per-robot friction, per-robot terrains, a per-robot
disturbance schedule held 5 steps, which divides no segment length), the wall quadruped (nu 12, B 1, T 2, M 1, 2).

  1. `rollout_segments` from displaced nodes = `rollout(diff_sol=True)` of the M B virtual robots built on the host: the segments' rows, the
     steps' outputs in (T, B) layout, and the tape - read through `vjp` (every entry of every block) and `lqr` (the corners) against the
     ordered restatements on the host's stitched blocks; the defects, D, J, lin_q and lin_r = the host's (`evaluate_segments`) and the restatement's
  2. the same with a cut step present: an iteration cap one below what the slowest step of the virtual robots needs leaves steps without a gradient
  3. nodes taken from a sequential rollout: every defect is 0.0 exactly, the stitched trajectory is the sequential one, and the tape answers
     `vjp` and `lqr` as `rollout_tape`'s does; J, lin_q, lin_r are `TrackingCost.evaluate`'s
  4. one segment is `rollout_tape`
  5. `lqr(defects=)`, without and under per-robot limits, = the g++ build of the chain with the hook on the device's blocks
  6. `ShootingNominal.forward` = the g++ build of the forward chain on the device's blocks and gains
  7. the line search: every candidate = its law restated on the host and the open-loop `rollout_segments` replay of what it applied; phi, ok and
     choice = the restated rules; a forced rejection leaves that robot alone
  8. `ilqr_shooting(segments=1)` = `plant.ilqr`'s host loop, through contact, under limits, through a rejection
  9. flight: one full step from displaced nodes closes the gaps and lands on the single-shooting LQ optimum
 10. contact from a state guess: phi never rises, the gaps close, the sequential replay reproduces the stitched trajectory

Measured figures: tests/README_plant_shooting.md.
"""
import dataclasses
import functools

import numpy as np
import pytest

import plant_adjoint_cases as pac
import plant_gradient_cases as pgc
import plant_riccati_cases as prc
import plant_shooting_cases as psc
import plant_shooting_ref as psr
import plant_staging_cases as pst

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), f"{what} differs"


@functools.lru_cache(maxsize=None)
def _sequential(which):
    """The sequential rollout of a case with its step gradients, once per process: (q, gamma, b, status, iters, StepGradients), read-only."""
    from contactimplicitmpc.jl_amd import plant
    c = psc.problem(which)
    ok, q, ua, gamma, b, status, iters, G = plant.rollout(c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"], diff_sol=True, **c["kw"])
    for a in (q, gamma, b, status, iters, G.dz, G.status):
        a.setflags(write=False)
    return q, gamma, b, status, iters, G


def _raw(cot):
    return dict(g_q0=cot.g_q0, g_q1=cot.g_q1, u_step=cot.u_step, w_step=cot.w_step, g_mu=cot.g_mu, g_h=cot.g_h)


def _tape_reads(tape, D, status, c, seed=0):
    """The tape against the host's blocks D (T, B, nr, n_cols) and their status: `vjp` of random cotangents = `chain_f64` (every entry of every
    block enters it), `lqr` with linear terms = `lq_f64` (the corners and the cut count), bit for bit."""
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    T, B = status.shape
    rng = np.random.default_rng([seed, T, B])
    np.testing.assert_array_equal(tape.grad_status, status)
    gq, gg, gb = pac.random_cotangents(rng, T, B, nq, nc, nb)
    cot = tape.vjp(gq, gg, gb)
    f64 = pac.chain_f64(D, gq, gg, gb, nq, nu, nw)
    assert cot.n_cut.tolist() == (status == 0).sum(axis=0).tolist()
    for k, dev in _raw(cot).items():
        assert (dev is None) == (f64[k] is None), k
        if dev is not None:
            _same(dev, np.asarray(f64[k], dtype=np.float64), f"vjp {k}")
    Q, R, Qf = prc.weights(rng, 2 * nq, nu, T)
    lq, lr = rng.standard_normal((T + 1, B, 2 * nq)), rng.standard_normal((T, B, nu))
    g = tape.lqr(Q, R, Qf, q=lq, r=lr, rho=1e-3)
    want = prc.lq_f64(D, status, nq, nu, Q, R, Qf, q=lq, r=lr, rho=1e-3)
    for k in prc.OUTPUTS:
        _same(getattr(g, k), np.asarray(want[k], dtype=np.float64), f"lqr {k}")
    assert g.status.tolist() == want["status"].tolist() and g.n_cut.tolist() == want["n_cut"].tolist()


def _segments_equal_the_virtual_robots(which, M, cut=False):
    """cut: the interior point's iteration cap is set one below what the slowest step of the virtual robots needs, so that step - or an earlier
    one of its segment that needs as many - does not converge and has no gradient."""
    from contactimplicitmpc.jl_amd import plant
    c = psc.problem(which)
    T, B, h = c["T"], c["q1"].shape[0], c["h"]
    L = T // M
    q1, v1 = psc.displaced_starts(c, _sequential(which)[0], M, seed=1)
    opts = plant.SIM_OPTS
    if cut:
        args, kw = psc.virtual_robots(c, q1, v1, M)
        slowest = int(plant.rollout(*args, **{k: v for k, v in kw.items() if k != "grad_cols"})[6].max())
        opts = dataclasses.replace(plant.SIM_OPTS, max_iter=slowest - 1)
    nodes = psc.nodes_of(q1, v1, h)
    Q, R, Qf, xg, ug = psc.cost_of(c, per_step=which == "hopper_2D")
    cost = plant.TrackingCost(Q, R, Qf, x_goal=xg, u_goal=ug)
    nom = plant.rollout_segments(c["model"], nodes, c["u"], h, c["mu"], segments=M, opts=opts, cost=cost, **c["kw"])
    args, kw = psc.virtual_robots(c, q1, v1, M)
    ok, q, ua, gamma, b, status, iters, G = plant.rollout(*args, diff_sol=True, opts=opts, **kw)
    assert q.shape == (L + 2, M * B, q1.shape[2])
    with nom.tape as tape:
        _same(nom.qs, q, "qs")
        _same(nom.nodes, np.concatenate([q[0], q[1]], axis=1).reshape(M, B, -1), "the nodes are the segments' first two rows")
        for name, got, virt in (("gamma", nom.gamma, gamma), ("b", nom.b, b), ("status", nom.status, status), ("iters", nom.iters, iters)):
            _same(got, psr.stitch(virt, M), name)
        assert tape.T == T and tape.B == B and tape.n_cols == G.dz.shape[3]
        _tape_reads(tape, psr.stitch(G.dz, M), psr.stitch(G.status, M), c)
    # the defects and the cost: the device's = the host entry's = the ordered restatement's
    host = cost.evaluate_segments(nom.qs, nom.u, M)
    f64 = psr.cost_f64(nom.qs, nom.u, M, Q, R, Qf, xg, ug)
    for name, dev, hst, ref in zip(psr.NAMES, (nom.J, nom.D, nom.defects, nom.lin_q, nom.lin_r), host, f64):
        _same(dev, hst, f"{name} (host entry)")
        _same(dev, np.asarray(ref, dtype=np.float64), f"{name} (restatement)")
    if M > 1:
        assert (np.abs(nom.defects) > 0).all(), "displaced nodes leave every defect entry nonzero"
    np.testing.assert_array_equal(nom.q_stitched()[:T], psr.stitch(q[:L], M))
    return nom, status, G


# ---- 1. the segments are the virtual robots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,M", psc.CASES)
def test_segments_equal_rollout_and_sensitivity_on_the_virtual_robots(which, M):
    nom, status, G = _segments_equal_the_virtual_robots(which, M)
    assert G.status.any(), "some step has a gradient, so that the blocks compared are not all zeros"
    if which == "flight":      # no contact: every step converges from a displaced node too
        assert status.all() and G.status.all()


# ---- 2. with a cut step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (3, 12))
def test_segments_with_a_cut_step_present(M):
    nom, status, G = _segments_equal_the_virtual_robots("hopper_2D", M, cut=True)
    assert (G.status == 0).any() and (G.status == 1).any(), "the cap cuts some steps and leaves others"


# ---- 3. nodes from a sequential rollout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,M", [cm for cm in psc.CASES if cm[1] > 1])
def test_nodes_of_a_sequential_rollout_close_every_gap(which, M):
    from contactimplicitmpc.jl_amd import plant
    c = psc.problem(which)
    T = c["T"]
    q, gamma, b, status, iters, G = _sequential(which)
    Q, R, Qf, xg, ug = psc.cost_of(c, seed=2)
    cost = plant.TrackingCost(Q, R, Qf, x_goal=xg, u_goal=ug)
    nom = plant.rollout_segments(c["model"], plant.segment_nodes(q, M), c["u"], c["h"], c["mu"], segments=M, cost=cost, **c["kw"])
    with nom.tape as tape:
        assert nom.defects.shape == (M - 1, q.shape[1], 2 * q.shape[2])
        np.testing.assert_array_equal(nom.defects, 0.0)
        np.testing.assert_array_equal(nom.D, 0.0)
        _same(nom.q_stitched(), q, "the stitched trajectory")
        for name, got, seq in (("gamma", nom.gamma, gamma), ("b", nom.b, b), ("status", nom.status, status), ("iters", nom.iters, iters)):
            _same(got, seq, name)
        _tape_reads(tape, G.dz, G.status, c, seed=3)      # the blocks of `rollout_tape`, which `rollout(diff_sol=True)` returns
    J, lq, lr = cost.evaluate(q, np.broadcast_to(c["u"], (T,) + nom.u.shape[1:]))
    _same(nom.J, J, "J"); _same(nom.lin_q, lq, "lin_q"); _same(nom.lin_r, lr, "lin_r")


# ---- 4. one segment ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(psc.SEGMENTS))
def test_one_segment_is_rollout_tape(which):
    from contactimplicitmpc.jl_amd import plant
    c = psc.problem(which)
    q, gamma, b, status, iters, G = _sequential(which)
    nom = plant.rollout_segments(c["model"], plant.segment_nodes(q, 1), c["u"], c["h"], c["mu"], segments=1, **c["kw"])
    ok, q2, ua, gamma2, b2, status2, iters2, tape2 = plant.rollout_tape(c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"], **c["kw"])
    with nom.tape as tape, tape2:
        _same(nom.qs, q2, "qs"); _same(nom.gamma, gamma2, "gamma"); _same(nom.b, b2, "b"); _same(nom.status, status2, "status"); _same(nom.iters, iters2, "iters")
        assert nom.J is None and nom.lin_q is None and nom.defects.shape[0] == 0 and nom.D.tolist() == [0.0] * q.shape[1]
        np.testing.assert_array_equal(tape.grad_status, tape2.grad_status)
        rng = np.random.default_rng(4)
        nq, nu, nc, nb = pgc.dims(c["model"])[:4]
        cots = pac.random_cotangents(rng, c["T"], q.shape[1], nq, nc, nb)
        a, bb = _raw(tape.vjp(*cots)), _raw(tape2.vjp(*cots))
        for k in a:
            assert (a[k] is None) == (bb[k] is None)
            if a[k] is not None:
                _same(a[k], bb[k], f"vjp {k}")


# ---- 5. the backward pass with defects ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_chain(tmp_path_factory):
    """tests/native/plant_shooting_check.cpp built with g++: csrc/plant_riccati.h's limited chain with the defect hook, a team of one."""
    import subprocess
    import test_plant_shooting as host
    exe = str(tmp_path_factory.mktemp("shooting") / "plant_shooting_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", exe, host.SRC])
    return exe


@pytest.mark.parametrize("which,M", [("flight", 2), ("flight", 8), ("hopper_2D", 3), ("hopper_2D", 12), ("centroidal_quadruped_wall", 2)])
def test_lqr_with_defects_is_the_host_chain_on_the_devices_blocks(host_chain, which, M):
    """On the tape of displaced nodes, under per-robot limits that bind and a rho per robot: `lqr(defects=d)` = the g++ build of the chain on the
    blocks `rollout(diff_sol=True)` gives for the virtual robots (test 1 holds the tape to them); `lqr(defects=zeros)` = `lqr` without them in
    K, k, P0, dV and clamped; without defects the call is the limited pass it was."""
    import test_plant_shooting as host
    from contactimplicitmpc.jl_amd import plant
    c = psc.problem(which)
    T, B, h = c["T"], c["q1"].shape[0], c["h"]
    L = T // M
    nq, nu = pgc.dims(c["model"])[:2]
    q1, v1 = psc.displaced_starts(c, _sequential(which)[0], M, seed=1)
    Q, R, Qf, xg, ug = psc.cost_of(c, seed=5)
    cost = plant.TrackingCost(Q, R, Qf, x_goal=xg, u_goal=ug)
    nom = plant.rollout_segments(c["model"], psc.nodes_of(q1, v1, h), c["u"], h, c["mu"], segments=M, cost=cost, **c["kw"])
    args, kw = psc.virtual_robots(c, q1, v1, M)
    G = plant.rollout(*args, diff_sol=True, **kw)[7]
    D, status = psr.stitch(G.dz, M), psr.stitch(G.status, M)
    rho = np.linspace(1e-4, 1e-3, B)
    with nom.tape as tape:
        free = tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, rho=rho, defects=nom.defects, segment_len=L)
        # per robot: the range its controls take, widened by a twentieth of its largest feedforward - so a step whose control sits at an end
        # of the range has that much room on that side and the feedforward there meets the limit
        lim = 0.05 * np.abs(free.k).max(axis=(0, 2))[:, None] * np.ones((B, nu))
        lo, hi = nom.u.min(axis=0) - lim, nom.u.max(axis=0) + lim
        limits = dict(u_lo=lo, u_hi=hi, u_nom=nom.u)
        got = tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, rho=rho, defects=nom.defects, segment_len=L, **limits)
        zero = tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, rho=rho, defects=np.zeros_like(nom.defects), segment_len=L, **limits)
        plain = tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, rho=rho, **limits)
        with pytest.raises(ValueError, match="defects must be"):
            tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, defects=nom.defects[:, :, :-1], segment_len=L)
        with pytest.raises(ValueError, match="defects and segment_len go together"):
            tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, defects=nom.defects)
        with pytest.raises(ValueError, match="a non-finite entry of defects"):
            tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, defects=np.full_like(nom.defects, np.nan), segment_len=L)
    with pytest.raises(ValueError, match="the tape is closed"):
        tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, defects=nom.defects, segment_len=L)
    for g, lims, what in ((free, {}, "no limits"), (got, dict(lo=lo, hi=hi, u_nom=nom.u), "limits")):
        want = host._run_lqr(host_chain, D, status, nq, nu, Q, R, Qf, nom.lin_q, nom.lin_r, rho, nom.defects, L, **lims)
        for k in prc.OUTPUTS:
            _same(getattr(g, k), np.ascontiguousarray(want[k], dtype=np.float64), f"{what}: {k}")
        assert g.status.tolist() == want["status"].tolist() and g.n_cut.tolist() == want["n_cut"].tolist()
        _same(g.clamped, want["clamped"], f"{what}: clamped")
    if got.status.tolist() == [0] * B:
        assert got.clamped.any(), "the limits bind"
    for k in ("K", "k", "P0", "dV", "clamped", "status", "n_cut"):
        _same(getattr(zero, k), getattr(plain, k), f"zero defects: {k}")
    np.testing.assert_array_equal(zero.p0, plain.p0)
    if status.all():      # through a cut step (B_t = 0) no defect reaches the control
        assert not np.array_equal(got.k, plain.k), "the defects move the feedforward"


# ---- 6. the linear forward pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,M", [("flight", 2), ("flight", 8), ("hopper_2D", 3), ("hopper_2D", 12), ("centroidal_quadruped_wall", 2)])
def test_the_forward_kernel_is_the_host_chain_on_the_devices_blocks_and_gains(host_chain, which, M):
    """`ShootingNominal.forward` on the tape of displaced nodes, with the gains `lqr(defects=)` gave on the device = the g++ build of
    `plant_shoot_forward_chain` on the host's blocks and those gains, in dx at the nodes, du and (dJ1, dJ2), bit for bit; with one segment
    nothing is launched and dJ is the backward pass's dV."""
    import test_plant_shooting as host
    from contactimplicitmpc.jl_amd import plant
    c = psc.problem(which)
    T, B, h = c["T"], c["q1"].shape[0], c["h"]
    L = T // M
    nq, nu = pgc.dims(c["model"])[:2]
    q1, v1 = psc.displaced_starts(c, _sequential(which)[0], M, seed=1)
    Q, R, Qf, xg, ug = psc.cost_of(c, seed=6, per_step=which == "hopper_2D")
    cost = plant.TrackingCost(Q, R, Qf, x_goal=xg, u_goal=ug)
    nom = plant.rollout_segments(c["model"], psc.nodes_of(q1, v1, h), c["u"], h, c["mu"], segments=M, cost=cost, **c["kw"])
    args, kw = psc.virtual_robots(c, q1, v1, M)
    G = plant.rollout(*args, diff_sol=True, **kw)[7]
    D = psr.stitch(G.dz, M)
    with nom.tape as tape:
        gains = tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, rho=1e-4, defects=nom.defects, segment_len=L)
        assert gains.status.tolist() == [0] * B
        dxn, du, dJ = nom.forward(gains, Q, R, Qf)
        with pytest.raises(ValueError, match="keep"):
            nom.forward(tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, defects=nom.defects, segment_len=L, keep=1), Q, R, Qf)
    with pytest.raises(ValueError, match="the tape is closed"):
        nom.forward(gains, Q, R, Qf)
    want = host._run_forward(host_chain, D, nq, nu, gains.K, gains.k, Q, R, Qf, nom.lin_q, nom.lin_r, nom.defects, L)
    for what, g, w in zip(("dx_nodes", "du", "dJ"), (dxn, du, dJ), want):
        _same(g, np.ascontiguousarray(w, dtype=np.float64), what)
    assert np.abs(dxn).max() > 0 and np.isfinite(dJ).all()
    one = plant.rollout_segments(c["model"], plant.segment_nodes(_sequential(which)[0], 1), c["u"], h, c["mu"], segments=1, cost=cost, **c["kw"])
    with one.tape as tape:
        g1 = tape.lqr(Q, R, Qf, q=one.lin_q, r=one.lin_r, rho=1e-4)
        dxn1, du1, dJ1 = one.forward(g1, Q, R, Qf)
    assert dxn1.shape == (0, B, 2 * nq)
    _same(dJ1, g1.dV, "one segment: dJ is dV"); _same(du1, g1.k, "one segment: du is k")


# ---- 7. the line search ----------------------------------------------------------------------------------------------------------------------------
LS_ALPHAS = (1.0, 0.3, 0.0)


def _law_on_the_host(nom, new, gains, alpha, dxn, lo=None, hi=None):
    """What the candidates of step length alpha must have done, restated on the host from the rows they returned: (the nodes they started from,
    the controls their steps applied).  Node j >= 1 is x^_j + alpha dx_{jL}, one rounded product and one rounded sum; step (j, l) applies
    limit(limit(u_nom + alpha k) + K (x_ref - x)) with x = [q1 - 1.0 (q1 - q0); q1] of its own rows, x_ref the same expression of the parent
    segment's rows, and the sum over the state in ascending index (plant_feedback.h as tests/plant_linesearch_cases._cpu_rollout restates it)."""
    M, (T, B, nu) = nom.segments, nom.u.shape
    L, nq = T // M, nom.qs.shape[2]
    nodes = nom.nodes.copy()
    nodes[1:] = nom.nodes[1:] + np.float64(alpha) * dxn
    clip = (lambda v, b: v) if lo is None else (lambda v, b: np.where(v < lo[b], lo[b], np.where(v > hi[b], hi[b], v)))
    state = lambda qs, l, r: np.concatenate([qs[l + 1, r] - 1.0 * (qs[l + 1, r] - qs[l, r]), qs[l + 1, r]])
    u = np.zeros_like(nom.u)
    for j in range(M):
        for b in range(B):
            r = j * B + b
            for l in range(L):
                t = j * L + l
                e = state(nom.qs, l, r) - state(new.qs, l, r)
                s = np.zeros(nu)
                for i in range(2 * nq):
                    s = s + gains.K[t, b, :, i] * e[i]
                u[t, b] = clip(clip(nom.u[t, b] + np.float64(alpha) * gains.k[t, b], b) + s, b)
    return nodes, u


@pytest.mark.parametrize("which,M,limited", [("flight", 4, False), ("hopper_2D", 3, True), ("hopper_2D", 12, False), ("centroidal_quadruped_wall", 2, True)])
def test_every_candidate_is_its_closed_loop_rollout_and_the_choice_is_the_restatements(which, M, limited):
    """One launch of three step lengths against three launches of one; every candidate against the law restated on the host and against the
    open-loop `rollout_segments` of the nodes it started from under the controls it applied (a closed-loop rollout IS the open-loop rollout on
    its applied controls; that replay also holds the new tape to `rollout_segments`' on the chosen rows); J, D, phi, ok and choice against
    `evaluate_segments` and the restated rules; a forced rejection leaves that robot's rows and blocks the parent's and the others untouched."""
    from contactimplicitmpc.jl_amd import plant
    c = psc.problem(which)
    T, B, h = c["T"], c["q1"].shape[0], c["h"]
    L = T // M
    nq, nu, nc, nb = pgc.dims(c["model"])[:4]
    q1, v1 = psc.displaced_starts(c, _sequential(which)[0], M, seed=1)
    Q, R, Qf, xg, ug = psc.cost_of(c, seed=7)
    cost = plant.TrackingCost(Q, R, Qf, x_goal=xg, u_goal=ug)
    nom = plant.rollout_segments(c["model"], psc.nodes_of(q1, v1, h), c["u"], h, c["mu"], segments=M, cost=cost, **c["kw"])
    weight, armijo = np.linspace(2.0, 5.0, B), 1e-4
    rho = np.full(B, 1e-3)
    lims = {}
    if limited:
        span = 0.5 * (np.abs(nom.u).max(axis=(0, 2)) + 1e-3)[:, None] * np.ones((B, nu))      # per robot, wide enough for its nominal
        lims = dict(u_lo=nom.u.min(axis=0) - span, u_hi=nom.u.max(axis=0) + span)
    open_door = np.full(B, np.inf)      # every converged candidate with a finite merit is acceptable: the call returns it
    with nom.tape as tape:
        gains = tape.lqr(Q, R, Qf, q=nom.lin_q, r=nom.lin_r, rho=rho, defects=nom.defects, segment_len=L, **(dict(lims, u_nom=nom.u) if limited else {}))
        assert gains.status.tolist() == [0] * B
        dxn, _, dJ = nom.forward(gains, Q, R, Qf)
        every = nom.linesearch(gains, cost, LS_ALPHAS, weight, armijo, dx_nodes=dxn, dJ=dJ, phi_nom=open_door, **lims)
        every.nominal.tape.close()
        assert every.J.shape == (3, B) and every.ok.shape == (3, B)
        conv = np.zeros((3, B), dtype=bool)
        for ci, a in enumerate(LS_ALPHAS):
            one = nom.linesearch(gains, cost, (a,), weight, armijo, dx_nodes=dxn, dJ=dJ, phi_nom=open_door, **lims)
            new = one.nominal
            for name in ("J", "D", "phi", "ok"):
                _same(getattr(one, name)[0], getattr(every, name)[ci], f"alpha {a}: {name} of one launch against three")
            conv[ci] = new.status.all(axis=0)
            got = one.choice >= 0
            assert got.tolist() == (conv[ci] & np.isfinite(one.phi[0])).tolist()
            nodes, u = _law_on_the_host(nom, new, gains, a, dxn, lims.get("u_lo"), lims.get("u_hi"))
            with new.tape as t_new:
                replay = plant.rollout_segments(c["model"], new.nodes, new.u, h, c["mu"], segments=M, cost=cost, **c["kw"])
                with replay.tape as t_rep:
                    for b in np.nonzero(got)[0]:
                        cols = np.arange(M) * B + b
                        _same(new.nodes[:, b], nodes[:, b], f"alpha {a}, robot {b}: the nodes the candidates start from")
                        _same(new.u[:, b], u[:, b], f"alpha {a}, robot {b}: the controls the law applies")
                        _same(new.qs[:, cols], replay.qs[:, cols], f"alpha {a}, robot {b}: the rows")
                        for name in ("gamma", "b", "status", "iters", "defects", "lin_q", "lin_r"):
                            _same(getattr(new, name)[:, b], getattr(replay, name)[:, b], f"alpha {a}, robot {b}: {name}")
                        _same(new.J[b], replay.J[b], "J"); _same(new.D[b], replay.D[b], "D")
                        _same(one.J[0, b], replay.J[b], "the candidate's J"); _same(one.D[0, b], replay.D[b], "the candidate's D")
                    np.testing.assert_array_equal(t_new.grad_status[:, got], t_rep.grad_status[:, got])
                    cots = pac.random_cotangents(np.random.default_rng(ci), T, B, nq, nc, nb)
                    va, vb = _raw(t_new.vjp(*cots)), _raw(t_rep.vjp(*cots))
                    for key in ("g_q0", "g_q1"):
                        _same(va[key][got], vb[key][got], f"alpha {a}: vjp {key} of the new tape against the replay's")
                    _same(va["u_step"][:, got], vb["u_step"][:, got], f"alpha {a}: vjp u_step")
            if a == 0.0:      # alpha 0 retraces the parent
                for b in np.nonzero(got)[0]:
                    _same(new.qs[:, np.arange(M) * B + b], nom.qs[:, np.arange(M) * B + b], "alpha 0 retraces the parent")
        # the rules, on the candidates' own J, D and convergence
        phi, ok, choice = psr.linesearch_rules(LS_ALPHAS, weight, conv, every.J, every.D, nom.J + weight * nom.D, nom.D, dJ, armijo)
        real = nom.linesearch(gains, cost, LS_ALPHAS, weight, armijo, dx_nodes=dxn, dJ=dJ, **lims)
        _same(real.phi, phi, "phi"); assert real.ok.tolist() == ok.tolist() and real.choice.tolist() == choice.tolist()
        _same(real.J, every.J, "J does not depend on the door"); _same(real.D, every.D, "D does not depend on the door")
        # a forced rejection of the last robot
        door = (nom.J + weight * nom.D).copy(); door[B - 1] = -np.inf
        shut = nom.linesearch(gains, cost, LS_ALPHAS, weight, armijo, dx_nodes=dxn, dJ=dJ, phi_nom=door, **lims)
        assert shut.choice[B - 1] == -1 and shut.choice[:B - 1].tolist() == real.choice[:B - 1].tolist()
        cols = np.arange(M) * B + (B - 1)
        _same(shut.nominal.qs[:, cols], nom.qs[:, cols], "a rejected robot keeps its rows")
        for name in ("u", "gamma", "b", "status", "iters", "defects", "lin_q", "lin_r"):
            _same(getattr(shut.nominal, name)[:, B - 1], getattr(nom, name)[:, B - 1], f"a rejected robot keeps its {name}")
        cots = pac.random_cotangents(np.random.default_rng(9), T, B, nq, nc, nb)
        with shut.nominal.tape as t_shut, real.nominal.tape as t_real:
            vs, vr, vp = _raw(t_shut.vjp(*cots)), _raw(t_real.vjp(*cots)), _raw(tape.vjp(*cots))
            np.testing.assert_array_equal(t_shut.grad_status[:, B - 1], tape.grad_status[:, B - 1])
        _same(vs["u_step"][:, B - 1], vp["u_step"][:, B - 1], "a rejected robot keeps the parent's blocks")
        _same(vs["g_q0"][B - 1], vp["g_q0"][B - 1], "a rejected robot keeps the parent's blocks")
        if B > 1:
            _same(vs["u_step"][:, :B - 1], vr["u_step"][:, :B - 1], "the other robots are untouched")
            for name in ("u", "gamma", "defects"):
                _same(getattr(shut.nominal, name)[:, :B - 1], getattr(real.nominal, name)[:, :B - 1], f"the other robots' {name}")


# ---- 8. one segment is plant.ilqr -------------------------------------------------------------------------------------------------------------------
def _loop_equals_ilqr(what, args, cost, limited=False, **kw):
    import test_gpu_plant_ilqr as ti
    from contactimplicitmpc.jl_amd import plant
    mine, host = plant.ilqr_shooting(*args, cost, segments=1, **kw), plant.ilqr(*args, cost, **kw)
    with mine.tape, host.tape:
        for name in ("u", "q", "gamma", "b", "J", "alpha", "rho", "accepted", "J0"):
            ti._same(getattr(mine, name), getattr(host, name), f"{what}: {name}")
        for name in ("K", "k", "dV", "status") + (("clamped", "n_cut") if limited else ()):
            ti._same(getattr(mine.gains, name), getattr(host.gains, name), f"{what}: gains.{name}")
        a, b = (ti._tape_answers(r.tape, cost, r.q, r.u) for r in (mine, host))
    for key in b:
        ti._same(a[key], b[key], f"{what}: {key} of the final tape")
    _same(mine.phi, mine.J, "one segment: the merit is the cost")
    np.testing.assert_array_equal(mine.D, 0.0)
    return host


def test_one_segment_is_ilqr_through_contact_under_limits_and_through_a_rejection():
    import plant_ilqr_cases as pic
    import plant_linesearch_cases as plc
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    Q, R, Qf, x_goal, u_goal = plc.contact_cost()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)
    host = _loop_equals_ilqr("contact, four iterations", pic.args(c), cost, max_iter=4, **pic.CONTACT)
    assert host.J.shape == (4, 3) and host.accepted.any()
    bound = 0.6 * np.abs(host.u).max()
    assert (np.abs(host.u) > bound).any()
    lim = _loop_equals_ilqr("contact under limits", pic.args(c), cost, limited=True, max_iter=3, u_lo=np.full(2, -bound), u_hi=np.full(2, bound), **pic.CONTACT)
    assert lim.gains.clamped.any()
    cb, (Qb, Rb, Qfb, xgb, ugb), kw = pic.bookkeeping()
    rej = _loop_equals_ilqr("through a rejection", pic.args(cb), plant.TrackingCost(Qb, Rb, Qfb, x_goal=xgb, u_goal=ugb), **kw)
    assert not rej.accepted.all() and rej.accepted.any()


# ---- 9. flight: one full step from displaced nodes ----------------------------------------------------------------------------------------------------
FLIGHT_MARGIN = 10.0      # over the existing single-shooting flight test's bound, 10 x the CPU restatement's gap; the figure seen is in the README


@pytest.mark.parametrize("M", (2, 4, 8))
def test_one_full_step_in_flight_closes_the_gaps_and_lands_on_the_lq_optimum(M):
    """Nodes displaced from the sequential trajectory by a seeded 1e-2, ONE iteration with alpha = 1 and rho = 0: in flight the plant is linear
    up to the interior point's smoothing, so the step closes every gap and lands on the optimum of the single-shooting LQ problem.  D: each
    defect entry is the difference of two states that each come out of step solves converged to r_tol = 1e-8, so D <= 2nq (M - 1) 1e-8.  u:
    against `lq_optimum_ld` on the sequential nominal's blocks, relative to the LQ step; the bound is the single-shooting flight test's
    (10 x the CPU restatement's gap, 2.7e-9) times FLIGHT_MARGIN."""
    import plant_linesearch_cases as plc
    from contactimplicitmpc.jl_amd import plant
    case, Q, R, Qf, x_goal, u_goal = plc.flight_case()
    gu_cpu, _ = plc.flight_gaps_cpu()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)
    args = (case["model"], case["q1"], case["v1"], case["u"], case["h"], case["mu"])
    *_, q0, ua0, _, _, _, _, G = plant.rollout(*args, terrain=case["terrain"], diff_sol=True)
    J_nom, lq, lr = cost.evaluate(q0, ua0)
    T, B, nq = case["T"], 2, 3
    L = T // M
    guess = q0.copy()
    guess[L:] += 1e-2 * np.random.default_rng([3, M]).standard_normal(guess[L:].shape)      # every node j >= 1 displaced, node 0 as measured
    res = plant.ilqr_shooting(*args, cost, segments=M, defect_weight=10.0, defect_tol=1e-6, q_guess=guess, alphas=(1.0,), max_iter=1, rho0=0.0,
                              terrain=case["terrain"])
    res.tape.close()
    assert res.D0.min() > 1e-3 and res.accepted.all(), (res.D0, res.accepted)
    gu = 0.0
    for b in range(B):
        du, _, _ = plc.lq_optimum_ld(G.dz, b, nq, 3, Q, R, Qf, lq, lr)
        gu = max(gu, float(np.abs(np.asarray(res.u[:, b], dtype=plc.LD) - (np.asarray(ua0[:, b], dtype=plc.LD) + du)).max() / np.abs(du).max()))
    print(f"flight M {M}: D0 {res.D0.tolist()} -> D {res.D[-1].tolist()}; controls {gu:.3e} from the single-shooting LQ optimum "
          f"(single-shooting bound {10 * gu_cpu:.3e}, ratio {gu / (10 * gu_cpu):.2f}, margin {FLIGHT_MARGIN})")
    assert (res.D[-1] <= 2 * nq * (M - 1) * 1e-8).all(), res.D[-1]
    assert gu <= FLIGHT_MARGIN * 10 * gu_cpu, f"{gu:.3e}"


# ---- 10. contact: a state initial guess ------------------------------------------------------------------------------------------------------------------
# defect_weight: the merit is exact only with a weight above the node constraints' multipliers, which the backward pass's value gradient estimates;
# the first backward pass of these runs has max |p0| 6 to 10.6, and the weight is ten times that.  (With 10.0, at the multipliers' own size, the
# hopper on the lowest friction but one is left with D 2e-7 to 7e-4 after 30 iterations: tests/README_plant_shooting.md.)
CONTACT_SHOOTING = dict(defect_weight=100.0, defect_tol=1e-6, alphas=(1.0, 0.5, 0.25, 0.125), max_iter=60, rho0=1e-6)
REPLAY_BOUND = 1e-5      # 10 x defect_tol, of the sequential replay from the stitched trajectory; see the docstring


@pytest.mark.parametrize("M", (2, 3, 4, 12))
def test_contact_from_the_goal_trajectory_closes_the_gaps(M):
    """The hoppers through contact from a STATE guess, q_guess = the goal held at every row: phi never rises, every robot ends with
    D <= defect_tol, and a sequential `rollout` under the final u reproduces the stitched trajectory within REPLAY_BOUND: the gaps left open
    are at most defect_tol = 1e-6 in all, and a gap at a node is carried to the end of the horizon by the contact dynamics, whose transition over
    these 12 steps is of order 1 to 10: REPLAY_BOUND = 10 defect_tol.  Measured on the first runs: the replay gap is 3 to 4 x D.  Robots 0 and 2
    close their gaps to 1e-13 in 6 to 11 iterations; robot 1 (friction 0.3) goes on alternating between a rejection and an accepted small step and
    needs 33 to 60 iterations to get D below 1e-6 at M = 3, 4, 12 - a finding, recorded in tests/README_plant_shooting.md."""
    import plant_linesearch_cases as plc
    from contactimplicitmpc.jl_amd import plant
    c = psc.problem("hopper_2D")
    T, B = c["T"], 3
    Q, R, Qf, x_goal, u_goal = plc.contact_cost()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal[:T + 1], u_goal=u_goal[:T])
    guess = np.broadcast_to(x_goal[0, 0, :4], (T + 2, B, 4)).copy()
    res = plant.ilqr_shooting(c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"], cost, segments=M, q_guess=guess, **CONTACT_SHOOTING, **c["kw"])
    res.tape.close()
    ok, q, *_ = plant.rollout(c["model"], c["q1"], c["v1"], res.u, c["h"], c["mu"], **{k: v for k, v in c["kw"].items() if k != "grad_cols"})
    gap = np.abs(q - res.q).max(axis=(0, 2))
    print(f"contact M {M}: {res.J.shape[0]} iterations, phi0 {res.phi0.tolist()} -> phi {res.phi[-1].tolist()}, D0 {res.D0.tolist()} -> D {res.D[-1].tolist()}, "
          f"J {res.J[-1].tolist()}, accepted per iteration {res.accepted.sum(axis=1).tolist()}, replay gap {gap.tolist()}")
    prev = res.phi0
    for i in range(res.phi.shape[0]):
        assert (res.phi[i] <= prev).all(), f"phi rises at iteration {i + 1}"
        prev = res.phi[i]
    assert (res.D[-1] <= CONTACT_SHOOTING["defect_tol"]).all(), f"gaps left open: D {res.D[-1]}"
    assert ok and (gap <= REPLAY_BOUND).all(), gap


# ---- the optional staged arrays ----------------------------------------------------------------------------------------------------------------
def test_shared_absent_and_per_robot_arrays_give_the_same_bits():
    """`plant.ilqr_shooting` with two segments: cimpc_plant_rollout_segments, cimpc_plant_tape_lqr_shooting, cimpc_plant_shooting_forward and
    cimpc_plant_shooting_linesearch, iteration after iteration."""
    # the entry's optional staged arrays (csrc/plant_staging.h) at B = 2, T = 4, two step lengths, two iterations: mu, w and the limits shared
    # against the same values per robot, and no limits against infinite ones, every returned array bit for bit (tests/plant_staging_cases.py).
    from contactimplicitmpc.jl_amd import plant
    args, _, (Q, R, Qf, x_goal, u_goal) = pst.hopper()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)

    def run(mu, **kw):
        res = plant.ilqr_shooting(*args, mu, cost, segments=pst.SEGMENTS, defect_weight=10.0, defect_tol=1e-6, **pst.LOOP, **kw)
        out = pst.arrays(res)
        res.tape.close()
        return out

    print("the shooting entries:", pst.loop_pairs(run), "arrays compared")
