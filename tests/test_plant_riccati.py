"""The LQ backward pass over a rollout tape (`cimpc_plant_tape_lqr`, `RolloutTape.lqr`) without a device: the
export, its ctypes signature and its Julia call; argument validation (which comes before any device call); csrc/plant_riccati.h built with
g++ and run by a team of one on synthetic tapes against the ordered float64 restatement `lq_f64` of tests/plant_riccati_cases.py, bit for
bit, and against the bounds of the longdouble restatement `lq_ld`; the same program under AddressSanitizer and UBSan; and `lq_ld` itself
against three things that do not share its recursion: the cost of the policy it returns, the KKT solve of the whole LQ problem, and
`gains_ref.tvlqr_ld` on the dense A_t, B_t.

Measured (this file's shapes): the host build equals `lq_f64` bit for bit at every shape, also under the sanitizers; `lq_f64` is at most
1.1e-15 from `lq_ld` (K of the largest model; bounds 2.2e-14 to 8.9e-14); the policy-cost identity holds to 5.1e-20 of the sum of |terms|
(allowed 1e-15); the KKT solve (210 unknowns, cond 1.2e2) and the policy's trajectory differ by 2.2e-19 (allowed 100 cond eps_ld =
1.3e-15); `lq_ld`'s K, P0 and `tvlqr_ld`'s differ by 0.0 (the sums are grouped alike; allowed 1e-15)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib
import gains_ref as gr
import plant_adjoint_cases as pac
import plant_riccati_cases as prc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID = -1
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip, "cimpc_plant_tape": C.c_void_p}
SRC = os.path.join(HERE, "native", "plant_riccati_check.cpp")
NAME = "cimpc_plant_tape_lqr"
LD = prc.LD


# ---- the export, its signature and validation --------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


def test_the_export_is_declared_and_bound():
    params = _prototype(NAME)
    assert NAME in _lib.SIGNATURES, f"{NAME} has no ctypes signature"
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(params) == 18
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), NAME)


JL_COMPAT = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*"}, "Ptr{Cvoid}": {"cimpc_plant_tape"}}


def test_julia_call_matches_the_prototype():
    assert "function plant_tape_lqr(" in JL, "julia/CIMPCHip.jl has no plant_tape_lqr"
    fn = JL[JL.index("function plant_tape_lqr("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\." + NAME + r"\((.*?)\)::Cint", fn, flags=re.S)
    assert m, f"plant_tape_lqr does not call {NAME}"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    params = _prototype(NAME)
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in JL_COMPAT[jt], f"argument {k}: Julia {jt} against C `{ct}`"


REFUSED = {"null tape": dict(tape=None), "rho negative": dict(rho=-1e-3), "rho NaN": dict(rho=float("nan")), "rho infinite": dict(rho=float("inf")),
           "n_Q = 0": dict(n_Q=0), "n_R = -1": dict(n_R=-1), "n_keep = 0": dict(n_keep=0), "laps = 0": dict(laps=0),
           "laps = 2 with q and r": dict(laps=2, lin=True), "q without r": dict(lin="q"), "k without q": dict(want_k=True), "null K": dict(K=None),
           "null status": dict(status=None)}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_lqr_refuses_invalid_arguments_without_a_device(what):
    """Each is refused before the tape is looked at: any non-null pointer stands in for one (zeroed memory, which a later check refuses too)."""
    stand_in = C.cast(C.create_string_buffer(4096), C.c_void_p)
    n, m, T, B = 4, 1, 3, 1
    a = dict(tape=stand_in, laps=1, n_Q=1, n_R=1, n_keep=1, rho=0.0, lin=False, want_k=False, K=np.zeros((1, B, n, m)), status=np.zeros(B, dtype=np.int32))
    a.update(REFUSED[what])
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib._dp)
    ip = lambda x: None if x is None else x.ctypes.data_as(_lib._ip)
    Q, Qf, R, q, r, k, n_cut = np.eye(n), np.eye(n), np.eye(m), np.zeros((T + 1, B, n)), np.zeros((T, B, m)), np.zeros((1, B, m)), np.zeros(B, dtype=np.int32)
    rc = _lib.load().cimpc_plant_tape_lqr(a["tape"], a["laps"], a["n_Q"], dp(Q), dp(Qf), a["n_R"], dp(R), dp(q) if a["lin"] else None,
                                          dp(r) if a["lin"] is True else None, a["rho"], a["n_keep"], dp(a["K"]), dp(k) if a["want_k"] or a["lin"] is True else None,
                                          None, None, None, ip(a["status"]), ip(n_cut))
    assert rc == INVALID


# ---- csrc/plant_riccati.h on the host ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_chain(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("riccati") / "plant_riccati_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", exe, SRC])
    return exe


# name: (nq, nu, nr, n_cols, T, B, dict(lin, per_step, rho, laps, keep, cut))
SHAPES = {
    "one by one, one step": (1, 1, 1, 3, 1, 1, dict(lin=True)),
    "one by one, pure gains": (1, 1, 1, 3, 1, 1, dict()),
    "strided block, a zero block, per-step weights, rho, keep 5": (3, 3, 7, 10, 14, 1, dict(lin=True, per_step=True, rho=0.25, keep=5, cut=7)),
    "strided block, three laps": (3, 3, 7, 10, 14, 1, dict(laps=3)),
    "strided block, rho 0, linear terms": (3, 3, 7, 10, 14, 1, dict(lin=True)),
    "the largest model, two robots, keep 1": (18, 12, 58, 53, 2, 2, dict(lin=True, keep=1, rho=1e-3)),
    "the largest model, two robots, pure gains": (18, 12, 58, 53, 2, 2, dict(per_step=True)),
}


def _case(name, seed=0):
    nq, nu, nr, n_cols, T, B, o = SHAPES[name]
    n, m = 2 * nq, nu
    rng = np.random.default_rng([seed, sorted(SHAPES).index(name)])
    D = rng.standard_normal((T, B, nr, n_cols)) / np.sqrt(n_cols)
    status = np.ones((T, B), dtype=np.int32)
    if o.get("cut") is not None:
        D[o["cut"], 0] = 0.0
        status[o["cut"], 0] = 0
    Q, R, Qf = prc.weights(rng, n, m, T, o.get("per_step", False))
    q = rng.standard_normal((T + 1, B, n)) if o.get("lin") else None
    r = rng.standard_normal((T, B, m)) if o.get("lin") else None
    kw = dict(q=q, r=r, rho=o.get("rho", 0.0), laps=o.get("laps", 1), keep=o.get("keep"))
    return D, status, (nq, nu, Q, R, Qf), kw


def _run_host(exe, D, status, nq, nu, Q, R, Qf, q=None, r=None, rho=0.0, laps=1, keep=None):
    T, B, nr, n_cols = D.shape
    n, m = 2 * nq, nu
    keep = T if keep is None else keep
    lin = q is not None
    hexes = lambda a: " ".join(float(x).hex() for x in np.asarray(a).ravel())
    cm = lambda M: np.swapaxes(np.asarray(M), -1, -2)      # the library's matrices are column-major
    text = [f"{B} {T} {nq} {nu} {nr} {n_cols} {laps} {1 if Q.ndim == 2 else T} {1 if R.ndim == 2 else T} {keep} {int(lin)} {float(rho).hex()}",
            " ".join(str(int(s)) for s in status.ravel()), hexes(cm(D)), hexes(cm(Q)), hexes(cm(Qf)), hexes(cm(R))]
    if lin:
        text += [hexes(q), hexes(r)]
    res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.split("\n")
    vals = [np.array([float.fromhex(v) for v in line.split()]) for line in lines[:5]]
    out = dict(K=cm(vals[0].reshape(keep, B, n, m)), P0=cm(vals[2].reshape(B, n, n)), k=None, p0=None, dV=None)
    if lin:
        out.update(k=vals[1].reshape(keep, B, m), p0=vals[3].reshape(B, n), dV=vals[4].reshape(B, 2))
    out["status"], out["n_cut"] = (np.array([int(v) for v in lines[i].split()], dtype=np.int32) for i in (5, 6))
    return out


def assert_bitwise(got, want, what=""):
    for key in prc.OUTPUTS:
        assert (got[key] is None) == (want[key] is None), (what, key)
        if want[key] is not None:
            assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(want[key]).tobytes(), f"{what}: {key} differs from lq_f64"
    assert got["status"].tolist() == want["status"].tolist() and got["n_cut"].tolist() == want["n_cut"].tolist(), what


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_build_of_the_kernels_statements_is_the_definition(host_chain, name):
    """Bit for bit `lq_f64`, which lies within 100 x max(d(lq_np, lq_ld), 2.2e-16) of `lq_ld` for every output."""
    D, status, args, kw = _case(name)
    got = _run_host(host_chain, D, status, *args, **kw)
    ld, f64, bound = prc.bounds(D, status, *args, **kw)
    assert_bitwise(got, f64, name)
    assert got["status"].tolist() == [0] * D.shape[1] and got["n_cut"].tolist() == (status == 0).sum(axis=0).tolist()
    for key in bound:
        dist = pac.distance(f64[key], ld[key])
        print(f"{name}, {key}: lq_f64 {dist:.2e} from lq_ld (bound {bound[key]:.2e})")
        assert dist <= bound[key]


def test_a_singular_step_ends_one_robot_alone(host_chain):
    """R = 0 and rho = 0 on a robot whose blocks are all zero: G = 0 at the first step walked, status 1, zero outputs; the robot beside it
    is the one it would be alone.  With rho > 0 both go through."""
    nq, nu, nr, n_cols, T, B = 3, 3, 7, 10, 4, 2
    rng = np.random.default_rng(5)
    D = rng.standard_normal((T, B, nr, n_cols)) / np.sqrt(n_cols)
    status = np.ones((T, B), dtype=np.int32)
    D[:, 0] = 0.0
    status[:, 0] = 0
    Q, _, Qf = prc.weights(rng, 2 * nq, nu)
    R = np.zeros((nu, nu))
    q, r = rng.standard_normal((T + 1, B, 2 * nq)), rng.standard_normal((T, B, nu))
    got = _run_host(host_chain, D, status, nq, nu, Q, R, Qf, q=q, r=r)
    assert_bitwise(got, prc.lq_f64(D, status, nq, nu, Q, R, Qf, q=q, r=r), "R = 0")
    assert got["status"].tolist() == [1, 0] and got["n_cut"].tolist() == [T, 0]
    for key in prc.OUTPUTS:
        robot0 = got[key][:, 0] if key in ("K", "k") else got[key][0]
        assert not robot0.any(), key
    alone = _run_host(host_chain, D[:, 1:], status[:, 1:], nq, nu, Q, R, Qf, q=q[:, 1:], r=r[:, 1:])
    assert alone["K"][:, 0].tobytes() == np.ascontiguousarray(got["K"][:, 1]).tobytes() and alone["p0"][0].tobytes() == got["p0"][1].tobytes()
    again = _run_host(host_chain, D, status, nq, nu, Q, R, Qf, q=q, r=r, rho=0.5)
    assert_bitwise(again, prc.lq_f64(D, status, nq, nu, Q, R, Qf, q=q, r=r, rho=0.5), "R = 0, rho = 0.5")
    assert again["status"].tolist() == [0, 0] and not again["K"][:, 0].any() and again["P0"][0].any()


def test_a_non_finite_weight_ends_the_chain_at_its_step(host_chain):
    """A NaN in Q_t of step t = 1 meets no pivot: the updated P is not finite there, walk step T - 1."""
    name = "strided block, a zero block, per-step weights, rho, keep 5"
    D, status, (nq, nu, Q, R, Qf), kw = _case(name)
    Q = Q.copy()
    Q[1, 2, 3] = np.nan
    got = _run_host(host_chain, D, status, nq, nu, Q, R, Qf, **kw)
    assert got["status"].tolist() == [D.shape[0] - 1]
    assert_bitwise(got, prc.lq_f64(D, status, nq, nu, Q, R, Qf, **kw), "NaN in Q")
    assert not got["K"].any() and not got["P0"].any()


def test_the_host_build_runs_clean_under_the_sanitizers(tmp_path):
    """The same program stand-alone with -fsanitize=address,undefined: every shape, the work array sized exactly as the kernel's LDS."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "plant_riccati_check_san")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, SRC], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr[-300:])
    for name in sorted(SHAPES):
        D, status, args, kw = _case(name)
        assert_bitwise(_run_host(exe, D, status, *args, **kw), prc.lq_f64(D, status, *args, **kw), name)


def test_the_plan_fits_a_cu_for_every_model(host_chain):
    text = open(os.path.join(ROOT, "contactimplicitmpc", "jl_amd", "csrc", "model_table.h")).read()
    rows = re.findall(r"X\((\w+), (\d+), (\d+), (\d+), (\d+), (\d+), \d\)", text)
    assert len(rows) >= 10
    for name, nq, nu, *_ in rows:
        nq, nu = int(nq), int(nu)
        if nu < 1:
            continue
        out = subprocess.run([host_chain, "plan", str(nq), str(nu)], capture_output=True, text=True, check=True)
        lds, fits = (int(v) for v in out.stdout.split())
        n, m = 2 * nq, nu
        assert lds == 8 * (2 * n * n + 2 * nq * (n + m) + 2 * nq * n + m * nq + 3 * m * n + m * (n + 1) + 2 * m * m + 2 * n + 3 * m + nq + 4), name
        assert fits == 1 and lds <= 160 * 1024, (name, lds)


# ---- lq_ld against what does not share its recursion -------------------------------------------------------------------------------------
def _policy_rollout(D, b, nq, nu, Q, R, Qf, q, r, K, k, x0):
    """x, u of δu_t = k_t - K_t δx_t from x0 through the dense A_t, B_t, and the terms of its cost, all longdouble."""
    T = D.shape[0]
    x, us, terms = np.asarray(x0, dtype=LD), [], []
    xs = [x]
    for t in range(T):
        A, Bm = prc.dense_AB(D[t, b], nq, nu, LD)
        Qt, Rt = (np.asarray(M if M.ndim == 2 else M[t], dtype=LD) for M in (Q, R))
        u = np.asarray(k[t, b], dtype=LD) - gr.mm_ld(np.asarray(K[t, b], dtype=LD), x)
        terms += [LD(0.5) * gr.mm_ld(x, gr.mm_ld(Qt, x)), gr.mm_ld(np.asarray(q[t, b], dtype=LD), x), LD(0.5) * gr.mm_ld(u, gr.mm_ld(Rt, u)),
                  gr.mm_ld(np.asarray(r[t, b], dtype=LD), u)]
        x = gr.mm_ld(A, x) + gr.mm_ld(Bm, u)
        us.append(u)
        xs.append(x)
    terms += [LD(0.5) * gr.mm_ld(x, gr.mm_ld(np.asarray(Qf, dtype=LD), x)), gr.mm_ld(np.asarray(q[T, b], dtype=LD), x)]
    return xs, us, terms


@pytest.mark.parametrize("name", ["strided block, a zero block, per-step weights, rho, keep 5", "strided block, rho 0, linear terms",
                                  "the largest model, two robots, keep 1"])
def test_the_value_of_lq_ld_is_the_cost_of_its_policy(name):
    """For any rho, ½ x0'P0 x0 + p0'x0 + dV1 + dV2 is the cost of δu = k - K δx from x0 (P, p are updated in the policy-evaluation form, and
    the constant collects k'Qu + ½ k'Quu k with the unregularized Quu).  Exact in exact arithmetic; both sides are longdouble (eps 1.1e-19)
    over some T (n + m)² ≈ 1e4 rounded operations an entry, so they are held to 1e-15 of the sum of the cost's |terms|: four orders above
    the longdouble unit and below what a float64 evaluation (eps 2.2e-16 times the same count) could meet."""
    D, status, (nq, nu, Q, R, Qf), kw = _case(name)
    kw = dict(kw, keep=None)
    ld = prc.lq_ld(D, status, nq, nu, Q, R, Qf, **kw)
    rng = np.random.default_rng(3)
    for b in range(D.shape[1]):
        x0 = rng.standard_normal(2 * nq)
        _, _, terms = _policy_rollout(D, b, nq, nu, Q, R, Qf, kw["q"], kw["r"], ld["K"], ld["k"], x0)
        x = np.asarray(x0, dtype=LD)
        value = LD(0.5) * gr.mm_ld(x, gr.mm_ld(ld["P0"][b], x)) + gr.mm_ld(ld["p0"][b], x) + ld["dV"][b, 0] + ld["dV"][b, 1]
        cost, mag = sum(terms), sum(abs(v) for v in terms)
        print(f"{name}, robot {b}: cost {float(cost):.12e}, value {float(value):.12e}, gap {float(abs(cost - value) / mag):.2e} of the terms")
        assert float(abs(cost - value)) <= 1e-15 * float(mag)


def test_lq_ld_at_rho_zero_solves_the_kkt_system():
    """The whole LQ problem from x0 as ONE linear system in z = (u_0, x_1, .., u_{T-1}, x_T) and the multipliers of the dynamics, solved in
    longdouble by `solve_ld`: the trajectory of lq_ld's policy is its solution.  A backward-stable solve errs by cond(KKT) eps_ld relative
    to the solution; 100 of that is allowed (cond from the float64 matrix)."""
    name = "strided block, rho 0, linear terms"
    D, status, (nq, nu, Q, R, Qf), kw = _case(name)
    T, n, m, b = D.shape[0], 2 * nq, nu, 0
    ld = prc.lq_ld(D, status, nq, nu, Q, R, Qf, **kw)
    x0 = np.asarray(np.random.default_rng(4).standard_normal(n), dtype=LD)
    w = n + m
    H, g, Cm, d = np.zeros((T * w, T * w), dtype=LD), np.zeros(T * w, dtype=LD), np.zeros((T * n, T * w), dtype=LD), np.zeros(T * n, dtype=LD)
    for t in range(T):
        A, Bm = prc.dense_AB(D[t, b], nq, nu, LD)
        iu, ix = slice(t * w, t * w + m), slice(t * w + m, (t + 1) * w)      # u_t, x_{t+1}
        H[iu, iu], g[iu] = R, kw["r"][t, b]
        H[ix, ix], g[ix] = (Qf, kw["q"][T, b]) if t == T - 1 else (Q, kw["q"][t + 1, b])
        rows = slice(t * n, (t + 1) * n)                                     # x_{t+1} - A_t x_t - B_t u_t = 0
        Cm[rows, ix], Cm[rows, iu] = np.eye(n, dtype=LD), -Bm
        if t == 0:
            d[rows] = gr.mm_ld(A, x0)
        else:
            Cm[rows, slice((t - 1) * w + m, t * w)] = -A
    KKT = np.block([[H, Cm.T], [Cm, np.zeros((T * n, T * n), dtype=LD)]])
    z = gr.solve_ld(KKT, np.concatenate([-g, d]))[:T * w]
    xs, us, _ = _policy_rollout(D, b, nq, nu, Q, R, Qf, kw["q"], kw["r"], ld["K"], ld["k"], x0)
    mine = np.concatenate([np.concatenate([us[t], xs[t + 1]]) for t in range(T)])
    cond = float(np.linalg.cond(KKT.astype(np.float64)))
    gap, allowed = pac.distance(mine, z), 100 * cond * float(np.finfo(LD).eps)
    print(f"KKT ({len(KKT)} unknowns, cond {cond:.1e}): the policy's trajectory {gap:.2e} from the solve (allowed {allowed:.2e})")
    assert gap <= allowed


@pytest.mark.parametrize("name", ["strided block, rho 0, linear terms", "the largest model, two robots, pure gains"])
def test_the_gains_of_lq_ld_are_those_of_tvlqr_ld_on_the_dense_matrices(name):
    """`gains_ref.tvlqr_ld` (the reference's recursion, written for the gain kernels) on A_t, B_t, Q_0 .. Q_{T-1}, Q_f: the same K, both
    longdouble, the sums grouped alike but the code apart; 1e-15 as for the policy's cost."""
    D, status, (nq, nu, Q, R, Qf), kw = _case(name)
    T = D.shape[0]
    ld = prc.lq_ld(D, status, nq, nu, Q, R, Qf, **dict(kw, q=None, r=None))
    for b in range(D.shape[1]):
        AB = [prc.dense_AB(D[t, b], nq, nu, LD) for t in range(T)]
        Qs = [Q if Q.ndim == 2 else Q[t] for t in range(T)] + [Qf]
        K, P = gr.tvlqr_ld([a for a, _ in AB], [bm for _, bm in AB], Qs, [R if R.ndim == 2 else R[t] for t in range(T)])
        gaps = pac.distance(ld["K"][:, b], np.stack(K)), pac.distance(ld["P0"][b], P[0])
        print(f"{name}, robot {b}: K {gaps[0]:.2e}, P0 {gaps[1]:.2e} from tvlqr_ld (allowed 1e-15)")
        assert max(gaps) <= 1e-15
