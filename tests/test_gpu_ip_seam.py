"""-m gpu: the per-knot interior-point operators of csrc/ip_kernel_impl.h (`IpSolver<M>`: residual, factorize, linear_solve, the sensitivity
pass) and of csrc/ip_generic.hip against `numpy.longdouble` (tests/ip_seam_ref.py) on the seeded inputs of tests/ip_seam_cases.py.

Every bound is min(1e-7, 100 max(d, 2.2e-16)) with d the distance of the float64 restatement of the device's algorithm (oracle/lcp.py) to the
same longdouble answer - built from the references alone (tests/test_ip_seam.py holds d <= 1e-9 without a device).  The factor 100 is the
margin tests/test_gpu_gains_edges.py gives a device LU over its float64 restatement: another summation order, reciprocals and rsq in place
of divisions.  What one MI355X run showed is in tests/README_ip_seam.md; the figures of a run are printed and kept in RECORD, which
scripts/ip_seam_record.py writes to profiles/ip_seam.json."""
import ctypes as C
import json

import numpy as np
import pytest

import ip_seam_cases as cases
import ip_seam_ref as ref
from common import make_case, make_solver

pytestmark = pytest.mark.gpu
RECORD = {}
SEAM_MODES = [(src, row, mode) for src, row in cases.SEAM for mode in (0, 1)]


def _record(key, val):
    RECORD[key] = val
    print("[ip_seam]", key, json.dumps(val))


@pytest.fixture(scope="module")
def solver_of():
    """One solver of H_ref = H = B = 1 per (source, row, mode), shared by the tests of this file and closed behind them."""
    made = {}

    def get(source, row, mode):
        if (source, row, mode) not in made:
            made[(source, row, mode)] = cases.one_knot_solver(source, row, mode)
        return made[(source, row, mode)]
    yield get
    for s in made.values():
        s.close()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _solve_calls(c):
    """(name, z, r, reg) of every linear-solve regime; (name, z, th, kappa, alt) of every residual case."""
    return [(name, s["z"], s["r"], s["reg"]) for name, s in c["solve"].items()], [(r["name"], r["z"], r["th"], r["kappa"], r["alt"]) for r in c["residual"]]


# ---- a. against the longdouble answers ---------------------------------------------------------------------------------------------------
def _judge(rec, key, err, d_ref):
    """Records the figures of one row and regime and returns the points beyond their own bounds.  err, d_ref: per point."""
    rec[key] = dict(err_dev=float(err.max()), d_ref=float(d_ref.max()), ratio=float((err / np.maximum(d_ref, ref.EPS64)).max()))
    return [(key, k, float(err[k]), ref.bound(d_ref[k])) for k in range(len(err)) if not err[k] <= ref.bound(d_ref[k])]


@pytest.mark.parametrize("source,row,mode", SEAM_MODES)
def test_linear_solve_and_residual_against_longdouble(gpu_required, solver_of, source, row, mode):
    """Every point of every call (n = 1, ppw - 1, ppw, ppw + 1, 2 ppw + 1) within ITS OWN bound min(1e-7, 100 max(d_ref, 2.2e-16)) of the
    longdouble answer.  d_ref of a linear-solve point is the float64 restatement's distance at the point and at a few last-place copies
    of it, the largest (`cases.N_NOISE`); of a residual point, the restatement's distance at the point.  A zero right-hand side (point 0
    of the synthetic knots) has d_ref = 0 and the answer 0: the device may be 2.2e-14 away from it, absolutely."""
    c = cases.seam_case(source, row)
    s = solver_of(source, row, mode)
    rec, bad = {}, []
    for name, sv in c["solve"].items():
        err = np.zeros(c["n"])
        for n in c["counts"]:
            delta = s.ip_linear_solve(1, sv["z"][:n], sv["r"][:n], reg=sv["reg"])
            assert delta.shape == (n, c["tab"].dims.nz) and np.isfinite(delta).all()
            err[:n] = np.maximum(err[:n], [ref.dist(delta[k], sv["ld"][k]) for k in range(n)])
        bad += _judge(rec, "solve/" + name, err, sv["d_ref"])
    for rs in c["residual"]:
        err = np.zeros(c["n"])
        for n in c["counts"]:
            r = s.ip_residual(1, rs["z"][:n], rs["th"][:n], rs["kappa"], alt=None if rs["alt"] is None else rs["alt"][:n])
            assert r.shape == (n, c["tab"].dims.nz) and np.isfinite(r).all()
            err[:n] = np.maximum(err[:n], [ref.dist(r[k], rs["ld"][k]) for k in range(n)])
        bad += _judge(rec, "residual/" + rs["name"], err, rs["d_ref"])
    _record(f"a/{source}/{row}/mode{mode}", rec)
    assert not bad, bad


# ---- b. bit identities ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,row,mode", SEAM_MODES)
def test_batch_position_and_denormal_reg_do_not_change_a_bit(gpu_required, solver_of, source, row, mode):
    """A batch of n points is n single-point calls; a point's answer does not depend on its place in the batch (reversed order); reg = 0.0
    is reg = 5e-324 where every y > 0.  The dead lane groups of the ragged last workgroup run on problem 0's data, and a store of theirs would
    land in problem 0's row or in the device's staging buffer: the comparisons above and part (a) on point 0 are what would see it.  The
    last check - the rows of a larger host buffer behind the last live point are still the zeros Python allocated - holds the HOST's copy
    to n rows; it says nothing about the kernel, which never sees that buffer."""
    c = cases.seam_case(source, row)
    s = solver_of(source, row, mode)
    n, nz = c["n"], c["tab"].dims.nz
    solves, residuals = _solve_calls(c)
    for name, z, r, reg in solves:
        full = s.ip_linear_solve(1, z, r, reg=reg)
        single = np.stack([s.ip_linear_solve(1, z[k], r[k], reg=reg)[0] for k in range(n)])
        assert _same_bits(full, single), ("solve", name, "batch against single calls")
        assert _same_bits(full, s.ip_linear_solve(1, z[::-1], r[::-1], reg=reg)[::-1]), ("solve", name, "reversed")
        if reg == 0.0:
            assert (z[:, c["tab"].dims.nq:] > 0).all()
            assert _same_bits(full, s.ip_linear_solve(1, z, r, reg=5e-324)), ("solve", name, "reg 5e-324")
    for name, z, th, kappa, alt in residuals:
        full = s.ip_residual(1, z, th, kappa, alt=alt)
        single = np.stack([s.ip_residual(1, z[k], th[k], kappa, alt=None if alt is None else alt[k])[0] for k in range(n)])
        assert _same_bits(full, single), ("residual", name, "batch against single calls")
        assert _same_bits(full, s.ip_residual(1, z[::-1], th[::-1], kappa, alt=None if alt is None else alt[::-1])[::-1]), ("residual", name, "reversed")
    # the host copies back n rows and no more: m points, a buffer of whole workgroups
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ppw = c["ppw"]
    for m in sorted({1, ppw + 1}):
        rows = (m + ppw - 1) // ppw * ppw + ppw
        name, z, r, reg = solves[2]
        zz, rr = np.ascontiguousarray(z[:m]), np.ascontiguousarray(r[:m])
        out = np.zeros((rows, nz))
        assert s.lib.cimpc_ip_linear_solve(s.h, 1, m, dp(zz), dp(rr), float(reg), dp(out)) == 0
        assert _same_bits(out[:m], s.ip_linear_solve(1, zz, rr, reg=reg)) and not out[m:].any() and not np.signbit(out[m:]).any()
        name, z, th, kappa, alt = residuals[0]
        zz, tt, aa = np.ascontiguousarray(z[:m]), np.ascontiguousarray(th[:m]), np.ascontiguousarray(alt[:m])
        out = np.zeros((rows, nz))
        assert s.lib.cimpc_ip_residual(s.h, 1, m, dp(zz), dp(tt), dp(aa), float(kappa), dp(out)) == 0
        assert _same_bits(out[:m], s.ip_residual(1, zz, tt, kappa, alt=aa)) and not out[m:].any() and not np.signbit(out[m:]).any()


@pytest.mark.parametrize("source,row", cases.SEAM)
def test_the_operators_do_not_depend_on_the_mode(gpu_required, solver_of, source, row):
    """:configurationforce mode (`RowModel<ID, 1>`) gives the Delta and the r of :configuration mode on the same table and point: only nd
    depends on the mode.  One MI355X run showed the two instantiations agree to the bit on every case (tests/README_ip_seam.md), so
    the bits are held."""
    c = cases.seam_case(source, row)
    s0, s1 = solver_of(source, row, 0), solver_of(source, row, 1)
    solves, residuals = _solve_calls(c)
    same = {}
    for name, z, r, reg in solves:
        same["solve/" + name] = _same_bits(s0.ip_linear_solve(1, z, r, reg=reg), s1.ip_linear_solve(1, z, r, reg=reg))
    for name, z, th, kappa, alt in residuals:
        same["residual/" + name] = _same_bits(s0.ip_residual(1, z, th, kappa, alt=alt), s1.ip_residual(1, z, th, kappa, alt=alt))
    _record(f"b/mode1_equals_mode0_bits/{source}/{row}", same)
    assert all(same.values()), same


# ---- c. the seam's refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_following_good_call_unchanged(gpu_required, solver_of):
    from contactimplicitmpc.jl_amd import CIMPCSolver
    from contactimplicitmpc.jl_amd._lib import CimpcError
    c = cases.seam_case("synth", "quadruped")
    good = solver_of("synth", "quadruped", 0)
    sv, rs = c["solve"]["reg"], c["residual"][0]

    def good_calls():
        return good.ip_linear_solve(1, sv["z"], sv["r"], reg=sv["reg"]), good.ip_residual(1, rs["z"], rs["th"], rs["kappa"], alt=rs["alt"])
    before = good_calls()

    def refused(s, t, message, n=2):
        d = s.nz, s.nth
        z, r, th = np.ones((n, d[0])), np.ones((n, d[0])), np.ones((n, d[1]))
        for call in (lambda: s.ip_linear_solve(t, z, r, reg=0.0), lambda: s.ip_residual(t, z, th, 1e-3)):
            with pytest.raises(CimpcError, match=message):
                call()
            after = good_calls()
            assert _same_bits(before[0], after[0]) and _same_bits(before[1], after[1]), message

    def other(model, mode, set_knot=True):
        d, prob, _, _ = make_case(model, mode, H_ref=3, H=1, B=1, seed=cases.SEED)
        s = CIMPCSolver(d.nq, d.nu, d.nw, d.nc, d.nb, 1, 1, B=1, mode=mode)
        if set_knot:
            s.set_linearization(1, prob["z0"][1], prob["th0"][1], prob["r0"][1], prob["rz0"][1], prob["rth0"][1])
        return s
    assert cases.model_table()["centroidal_wall"]["lanes"] == 64 and "anydims" not in cases.model_table()
    for model, mode, message in (("centroidal_wall", 0, "callback launch failed"),                      # a 64-lane row: a compiled sweep, no callback
                                 ("centroidal_wall", 1, "B2 callbacks exist for the compiled lane-group models only"),
                                 ("anydims", 0, "B2 callbacks exist for the compiled lane-group models only"),
                                 ("anydims", 1, "B2 callbacks exist for the compiled lane-group models only")):
        s = other(model, mode)
        refused(s, 1, message)
        s.close()
    refused(good, 0, "knot index out of range")
    refused(good, good.H_ref + 1, "knot index out of range")
    s = other("quadruped", 0, set_knot=False)
    refused(s, 1, "set_linearization has not been called for this knot")
    s.close()
    refused(good, 1, "null argument", n=0)


# ---- d. the sensitivities at the device's own converged point -----------------------------------------------------------------------------
def _implicit_dynamics(case, which, H):
    """implicit_dynamics of the rollouts `which` of the case in one solver of B = len(which), with the options of `cases.sens_device_opts`."""
    ro = [case["rollouts"][b] for b in which]
    tr = [case["trajs"][b] for b in which]
    s = make_solver(case["d"], case["prob"], ro, H, ip_opts=cases.sens_device_opts())
    out = s.implicit_dynamics(np.stack([t.q for t in tr]), np.stack([t.theta for t in tr]), np.stack([t.gamma for t in tr]),
                              np.stack([t.b for t in tr]), want_z=True)
    s.close()
    return out


@pytest.mark.parametrize("model,mode,H", cases.SENS_CASES)
def test_sensitivities_are_the_solve_at_the_converged_point(gpu_required, model, mode, H):
    """dq0, dq1, du1 of every problem against -rz_reg^-1 rtheta (longdouble) AT THE DEVICE'S OWN z, reg = kappa_tol gamma_reg (kappa_reg = 0:
    `cases.SENS_KAPPA_REG`).  The device's point is the argument of the reference only; the bound comes from the two float64 forms of the
    solve at the oracle's converged point of the same problem.  B H = 3 and 6 problems (5 in the H = 5 cases): fewer than a 16-lane
    wavefront's four lane groups, one more, two more."""
    case = cases.sens_case(model, mode, H)
    d = case["d"]
    nq, nd = d.nq, d.nd
    B = len(case["rollouts"])
    assert d.nd == (nq if mode == 0 else nq + d.nc + d.nb)
    out = _implicit_dynamics(case, range(B), H)
    assert out["status"].all(), (out["status"], out["iters"])          # every problem converges, no knot excluded
    z = out["z"]
    rec, bad = dict(err_dev=0.0, d=0.0, ratio=0.0, min_y=float(z[..., nq:].min()), iters=out["iters"].tolist()), []
    for b in range(B):
        window, tr = case["rollouts"][b][0], case["trajs"][b]
        for i in range(H):
            ld = cases.sens_block(ref.sensitivities_ld(case["tabs"][int(window[i])], z[b, i], cases.SENS_REG, d))
            dev = np.concatenate([out[k][b, i] for k in ("dq0", "dq1", "du1")], axis=-1)
            assert dev.shape == ld.shape == (nd, 2 * nq + d.nu) and np.isfinite(dev).all()
            err, dd = ref.dist(dev, ld), max(case["d_direct"][b][i], case["d_adjoint"][b][i])
            rec["err_dev"] = max(rec["err_dev"], err); rec["d"] = max(rec["d"], dd); rec["ratio"] = max(rec["ratio"], err / max(dd, ref.EPS64))
            if not err <= cases.sens_bound(case, b, i):
                bad.append((b, i, err, cases.sens_bound(case, b, i)))
            # d is the first nd entries of z, less the trajectory's own (implicit_dynamics.jl:180-190)
            own = np.concatenate([tr.q[i + 2], tr.gamma[i], tr.b[i]])[:nd]
            assert _same_bits(out["d"][b, i], z[b, i, :nd] - own), (b, i)
    _record(f"d/{model}/mode{mode}/H{H}", rec)
    assert not bad, bad
    assert (z[..., nq:] > 0).all()
    if model in cases.CLAMP_LIVE:          # the clamp at reg is live at the device's converged points
        assert rec["min_y"] < cases.SENS_REG, rec["min_y"]
    if B == 2:          # the blocks of the B = 2 call are those of its rollouts' B = 1 calls: to the bit on every case in one MI355X run, so the bits are held
        same = True
        for b in range(B):
            one = _implicit_dynamics(case, [b], H)
            assert one["status"].all()
            for k in ("z", "d", "dq0", "dq1", "du1"):
                same &= _same_bits(np.ascontiguousarray(out[k][b]), np.ascontiguousarray(one[k][0]))
            assert np.array_equal(out["iters"][b], one["iters"][0])
        _record(f"d/B2_equals_B1_bits/{model}/mode{mode}", bool(same))
        assert same
