"""The inputs of tests/test_gpu_ip_seam.py hold their conditions, by the references alone (no device): tests/ip_seam_ref.py is the
longdouble statement of the per-knot interior-point operators, tests/ip_seam_cases.py the seeded inputs, oracle/lcp.py the float64
restatement of the device's algorithm.  `d_ref`, the relative max-norm distance of the restatement to the longdouble answer, is what
every device bound is built from (min(1e-7, 100 max(d_ref, 2.2e-16))); it must be at most 1e-9 on every case, so that no bound exceeds
1e-7, the loosest figure the suite accepts anywhere for a linear solve.  A seed that misses a condition is changed, never the condition."""
import numpy as np
import pytest

from oracle import lcp

import ip_seam_cases as cases
import ip_seam_ref as ref
from common import MODELS
from gains_ref import LD, solve_ld

D_REF_MAX = 1e-9


def test_solve_ld_against_lapack_on_a_43_x_43_system():
    rng = np.random.default_rng(43)
    M = rng.standard_normal((43, 43)) + 3.0 * np.eye(43)
    rhs = rng.standard_normal((43, 3))
    x = solve_ld(M, rhs)
    assert x.dtype == LD
    assert np.abs(x.astype(np.float64) - np.linalg.solve(M, rhs)).max() <= 1e-13 * np.linalg.cond(M) * np.abs(x).max()
    # ... and to its own type's precision: the residual of the longdouble answer, evaluated in longdouble
    res = np.abs(np.matmul(M.astype(LD), x) - rhs.astype(LD)).max()
    assert res <= 43 * 50 * float(np.finfo(LD).eps) * float(np.abs(M).sum(axis=1).max() * np.abs(x).max())


def test_lane_widths_come_from_the_model_table():
    tab = cases.model_table()
    assert set(cases.ROWS) < set(tab) and len(tab) == 10
    for name, row in tab.items():
        m = MODELS[name]
        assert row["dims"] == tuple(m[k] for k in ("nq", "nu", "nw", "nc", "nb")), name
        assert row["lanes"] == cases.lanes_by_rule(m), name          # the rule the header states, applied to the oracle's own rows
    assert {tab[r]["lanes"] for r in cases.ROWS} == {16, 32} and tab["centroidal_wall"]["lanes"] == 64
    assert cases.point_counts(4) == [1, 3, 4, 5, 9] and cases.point_counts(2) == [1, 2, 3, 5] and cases.point_counts(1) == [1, 2, 3]


@pytest.mark.parametrize("source,row", cases.SEAM)
def test_rz_reg_is_the_system_the_restatement_solves(source, row):
    """`rz_reg` with reg = 0 is `lcp.dense_rz`; with reg > 0 the float64 restatement (rzlin + linear_solve_vec: Schur complement with the
    clamped D, dy2 from the clamped last line) satisfies rz_reg delta = r to its own precision - the reading of the device's
    `factorize(reg)` / `linear_solve()` the longdouble reference rests on."""
    c = cases.seam_case(source, row)
    tab = c["tab"]
    d = tab.dims
    for name in ("near", "late"):
        z = c["solve"][name]["z"][1]
        assert np.array_equal(ref.rz_reg(tab, z, 0.0).astype(np.float64), lcp.dense_rz(tab, z))
        assert np.array_equal(ref.rz_reg(tab, z, 5e-324).astype(np.float64), lcp.dense_rz(tab, z))
    z, r = c["solve"]["reg"]["z"][1], c["solve"]["reg"]["r"][1]
    M = ref.rz_reg(tab, z, cases.REG)
    assert not np.array_equal(M.astype(np.float64), lcp.dense_rz(tab, z))          # the clamp is live
    lcp.rzlin(tab, z, cases.REG)
    delta = lcp.linear_solve_vec(tab, r[d.ix], r[d.iy1], r[d.iy2], cases.REG)
    back = np.abs(np.matmul(M, delta.astype(LD)) - r.astype(LD)).max() / (np.abs(M).sum(axis=1).max() * np.abs(delta).max())
    assert back <= 1e-12, back          # a wrong reading of the clamp leaves a residual of the size of reg / y, not of round-off


@pytest.mark.parametrize("source,row", cases.SEAM)
def test_seam_inputs_hold_their_conditions(source, row):
    c = cases.seam_case(source, row)
    d = c["tab"].dims
    assert c["ppw"] == 64 // c["G"] and c["n"] == c["counts"][-1] == 2 * c["ppw"] + 1
    for name, s in c["solve"].items():
        print(f"[ip_seam] {source}/{row} solve/{name}: d_ref max {s['d_ref'].max():.2e} median {np.median(s['d_ref']):.2e} cond max {s['cond'].max():.2e}")
        assert np.isfinite(s["d_ref"]).all() and s["d_ref"].max() <= D_REF_MAX, (name, s["d_ref"])
        y1, y2 = s["z"][:, d.iy1], s["z"][:, d.iy2]
        assert (y1 > 0).all() and (y2 > 0).all()
    for r in c["residual"]:
        print(f"[ip_seam] {source}/{row} residual/{r['name']}: d_ref max {r['d_ref'].max():.2e}")
        assert np.isfinite(r["d_ref"]).all() and r["d_ref"].max() <= D_REF_MAX, (r["name"], r["d_ref"])
    assert sum(r["alt"] is not None for r in c["residual"]) * 2 == len(c["residual"])
    # late: every pair on y1 y2 = 1e-8, split unevenly, both orientations inside every point
    z = c["solve"]["late"]["z"]
    y1, y2 = z[:, d.iy1], z[:, d.iy2]
    np.testing.assert_allclose(y1 * y2, cases.LATE_PRODUCT, rtol=1e-14, atol=0)
    assert ((y1 < y2).any(axis=1) & (y1 > y2).any(axis=1)).all()
    assert np.minimum(y1, y2).min() >= 1e-6 * (1 - 1e-12) and np.minimum(y1, y2).max() <= 1e-4
    # reg: several y below reg and several above, in every point
    s = c["solve"]["reg"]
    y = np.concatenate([s["z"][:, d.iy1], s["z"][:, d.iy2]], axis=1)
    assert s["reg"] == cases.REG and ((y < s["reg"]).sum(axis=1) >= 2).all() and ((y > s["reg"]).sum(axis=1) >= 2).all()
    assert c["solve"]["near"]["reg"] == 0.0 and c["solve"]["late"]["reg"] == 0.0
    # right-hand sides: r0 for the first point
    assert np.array_equal(c["solve"]["near"]["r"][0], c["knot"][3])


def test_float64_lapack_on_the_same_systems():
    """The float64 dense LU (LAPACK) on the same systems, for the record: the longdouble answers are not an artefact of `solve_ld`."""
    worst = raw = 0.0
    for source, row in cases.SEAM:
        c = cases.seam_case(source, row)
        for name, s in c["solve"].items():
            for k in range(c["n"]):
                if np.abs(s["ld"][k]).max() == 0:
                    continue
                x = np.linalg.solve(ref.rz_reg(c["tab"], s["z"][k], s["reg"]).astype(np.float64), s["r"][k])
                raw = max(raw, ref.dist(x, s["ld"][k]))
                worst = max(worst, ref.dist(x, s["ld"][k]) / s["cond"][k])
    print(f"[ip_seam] float64 LAPACK LU: worst distance {raw:.2e}, worst distance / cond {worst:.2e}")
    assert worst <= 2.2e-16          # backward stable: far inside cond x eps on every system


@pytest.mark.parametrize("model,mode,H", cases.SENS_CASES)
def test_sensitivity_cases_converge_and_hold_their_distances(model, mode, H):
    """On the oracle, with the options the device test uses (kappa_reg = 0: the sensitivity solve runs at kappa_tol gamma_reg exactly):
    every problem converges, no knot excluded, and the two float64 forms of the sensitivity solve are within 1e-9 of the longdouble block
    at the oracle's converged points."""
    c = cases.sens_case(model, mode, H)
    d = c["d"]
    assert cases.SENS_REG == 2e-4 * 0.1 and cases.sens_oracle_opts().kappa_reg == 0.0
    assert len(c["oracle"]) == (2 if H == 3 else 1)
    for b, o in enumerate(c["oracle"]):
        assert o["status"].all(), (b, o["status"], o["iters"])
        assert o["z"].shape == (H, d.nz) and (o["z"][:, d.nq:] > 0).all()
        print(f"[ip_seam] sens {model} mode {mode} H {H} rollout {b}: iters {o['iters'].tolist()} d_direct max {c['d_direct'][b].max():.2e} "
              f"d_adjoint max {c['d_adjoint'][b].max():.2e} cond max {c['cond'][b].max():.2e} min y {o['z'][:, d.nq:].min():.2e}")
        assert c["d_direct"][b].max() <= D_REF_MAX and c["d_adjoint"][b].max() <= D_REF_MAX
    if model in cases.CLAMP_LIVE:      # the clamp at reg is live at the converged points
        assert min(o["z"][:, d.nq:].min() for o in c["oracle"]) < cases.SENS_REG
