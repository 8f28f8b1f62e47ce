"""The limited LQ backward pass (`cimpc_plant_tape_lqr_box`, `RolloutTape.lqr(u_lo=, u_hi=, u_nom=)`) without a
device: csrc/plant_boxqp.h inside the BOX chain of csrc/plant_riccati.h, built with g++ and run by a team of one, against the ordered float64
restatement `lq_box_f64` of tests/plant_boxqp_cases.py bit for bit, against the bounds of the longdouble restatement `lq_box_ld`, against a
brute-force search over every active set, and against the KKT conditions; infinite and never-binding limits and a rho per robot against the
unlimited `lq_f64`; the value of the returned policy; the limiter; the refusals, which come before any device call; the export, its ctypes
signature and its Julia call; and the same host program under AddressSanitizer and UBSan.  tests/README_plant_boxqp.md has the figures."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib
import gains_ref as gr
import plant_adjoint_cases as pac
import plant_boxqp_cases as pbc
import plant_riccati_cases as prc
import test_plant_riccati as tpr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "plant_boxqp_check.cpp")
NAME = "cimpc_plant_tape_lqr_box"
LD = prc.LD
INVALID = -1
KEYS = prc.OUTPUTS


# ---- the host build ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_chain(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("boxqp") / "plant_boxqp_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", exe, SRC])
    return exe


def run_host(exe, D, status, nq, nu, Q, R, Qf, q, r, rho=0.0, u_lo=None, u_hi=None, u_nom=None, keep=None):
    T, B, nr, n_cols = D.shape
    n, m = 2 * nq, nu
    keep = T if keep is None else keep
    hexes = lambda a: " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel())
    cm = lambda M: np.swapaxes(np.asarray(M), -1, -2)      # the library's matrices are column-major
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    n_lim = 0 if u_lo is None else np.atleast_2d(u_lo).shape[0]
    text = [f"{B} {T} {nq} {nu} {nr} {n_cols} {1 if Q.ndim == 2 else T} {1 if R.ndim == 2 else T} {keep} {rho.size} {n_lim}",
            " ".join(str(int(s)) for s in status.ravel()), hexes(cm(D)), hexes(cm(Q)), hexes(cm(Qf)), hexes(cm(R)), hexes(q), hexes(r), hexes(rho)]
    if n_lim:
        text += [hexes(u_lo), hexes(u_hi), hexes(u_nom)]
    res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.split("\n")
    vals = [np.array([float.fromhex(v) for v in line.split()]) for line in lines[:5]]
    out = dict(K=cm(vals[0].reshape(keep, B, n, m)), k=vals[1].reshape(keep, B, m), P0=cm(vals[2].reshape(B, n, n)), p0=vals[3].reshape(B, n),
               dV=vals[4].reshape(B, 2))
    out["status"], out["n_cut"], clamped = (np.array([int(v) for v in lines[i].split()], dtype=np.int32) for i in (5, 6, 7))
    out["clamped"] = clamped.reshape(keep, B)
    return out


def assert_bitwise(got, want, what="", clamped=True):
    for key in KEYS:
        assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(want[key]).tobytes(), f"{what}: {key} differs"
    assert got["status"].tolist() == want["status"].tolist() and got["n_cut"].tolist() == want["n_cut"].tolist(), what
    if clamped:
        assert got["clamped"].tolist() == want["clamped"].tolist(), f"{what}: clamped differs"


def assert_some_but_not_all_clamp(clamped, nu, what=""):
    """The guard against a vacuous case: per robot 0 < clamped (step, control) pairs < steps x nu."""
    counts = pbc.clamped_counts(clamped, nu)
    full = np.asarray(clamped).shape[0] * nu
    print(f"{what}: clamped {counts.tolist()} of {full} per robot")
    assert np.all(counts > 0) and np.all(counts < full), (what, counts.tolist(), full)


@pytest.fixture(scope="module")
def restated():
    """Every case's restatements, computed once: name -> (ld, f64, bound, trace)."""
    memo = {}

    def get(name):
        if name not in memo:
            D, status, args, kw = pbc.case(name)
            trace = []
            ld, f64, bound = pbc.bounds(D, status, *args, **kw)
            pbc.lq_box_f64(D, status, *args, **kw, trace=trace)
            memo[name] = (ld, f64, bound, trace)
        return memo[name]
    return get


@pytest.mark.parametrize("name", sorted(pbc.SHAPES))
def test_the_cases_clamp_some_controls_and_not_all(name, restated):
    """On the restatement alone: the limits placed from the unlimited k bind somewhere and not everywhere, and the projected Newton
    iteration really runs."""
    ld, f64, _, _ = restated(name)
    nu = pbc.SHAPES[name][1]
    assert f64["status"].tolist() == [0] * f64["status"].size
    assert_some_but_not_all_clamp(f64["clamped"], nu, name)
    assert f64["clamped"].tolist() == ld["clamped"].tolist(), "the float64 and the longdouble restatements disagree on the clamped sets"
    assert f64["iterations"].max() >= 1
    print(f"{name}: at most {f64['iterations'].max()} Newton directions a step")


@pytest.mark.parametrize("name", sorted(pbc.SHAPES))
def test_host_build_is_the_definition_bit_for_bit_and_within_the_longdouble_bounds(host_chain, name, restated):
    D, status, args, kw = pbc.case(name)
    got = run_host(host_chain, D, status, *args, **kw)
    ld, f64, bound, _ = restated(name)
    assert_bitwise(got, f64, name)
    assert got["status"].tolist() == [0] * D.shape[1]
    assert_some_but_not_all_clamp(got["clamped"], args[1], name)
    for key in bound:
        dist = pac.distance(f64[key], ld[key])
        print(f"{name}, {key}: lq_box_f64 {dist:.2e} from lq_box_ld (bound {bound[key]:.2e})")
        assert dist <= bound[key]


@pytest.mark.parametrize("name", [n for n in sorted(pbc.SHAPES) if pbc.SHAPES[n][1] <= 4])
def test_every_step_finds_the_active_set_of_the_brute_force_search(name, restated):
    """All 3^nu active sets in longdouble at every walk step, on the G, Qu and bounds the device-order chain met there: exactly one is
    feasible with the right gradient signs, it is the chain's clamped set, and the chain's k lies within the case's bound of its x."""
    _, f64, bound, trace = restated(name)
    assert_some_but_not_all_clamp(f64["clamped"], pbc.SHAPES[name][1], name)
    worst = 0.0
    for rec in trace:
        found = pbc.brute_force(rec["G"], rec["Qu"], rec["lo"], rec["hi"])
        assert len(found) == 1, (name, rec["b"], rec["t"], len(found))
        x, mask = found[0]
        assert mask == rec["mask"], (name, rec["b"], rec["t"], mask, rec["mask"])
        worst = max(worst, pac.distance(rec["k"], x))
    print(f"{name}: k at most {worst:.2e} from the brute-force solution over {len(trace)} steps (bound {bound['k']:.2e})")
    assert worst <= bound["k"]


@pytest.mark.parametrize("name", [n for n in sorted(pbc.SHAPES) if pbc.SHAPES[n][1] >= 8])
def test_kkt_conditions_at_every_step(name, restated, host_chain):
    """nu 8 and 12, on the host build's own outputs where they are kept: lo <= k <= hi exactly, clamped rows of K exactly zero, k on its bound
    with the gradient pointing out of the box on the clamped set, and the free gradient within the case's bound of |Qu| + |G||k|."""
    D, status, args, kw = pbc.case(name)
    got = run_host(host_chain, D, status, *args, **kw)
    _, f64, bound, trace = restated(name)
    nu = args[1]
    assert_some_but_not_all_clamp(got["clamped"], nu, name)
    worst = 0.0
    for rec in trace:
        b, t = rec["b"], rec["t"]
        k, K, mask = got["k"][t, b], got["K"][t, b], int(got["clamped"][t, b])
        assert mask == rec["mask"]
        c = np.array([(mask >> i) & 1 for i in range(nu)], dtype=bool)
        lo, hi = rec["lo"], rec["hi"]
        assert np.all(k >= lo) and np.all(k <= hi)
        assert not K[c].any() and (K[~c] != 0).any()
        G, Qu = np.asarray(rec["G"], dtype=LD), np.asarray(rec["Qu"], dtype=LD)
        g = Qu + gr.mm_ld(G, np.asarray(k, dtype=LD))
        assert np.all((k[c] == lo[c]) | (k[c] == hi[c]))
        assert np.all(g[c][k[c] == lo[c]] > 0) and np.all(g[c][k[c] == hi[c]] < 0)
        scale = np.abs(Qu) + gr.mm_ld(np.abs(G), np.abs(np.asarray(k, dtype=LD)))
        inside = ~c & (k > lo) & (k < hi)
        assert inside.any()
        worst = max(worst, float(np.max(np.abs(g[inside]) / scale[inside])))
    print(f"{name}: free gradient at most {worst:.2e} of its terms (bound {bound['k']:.2e})")
    assert worst <= bound["k"]


# ---- limits that do not bind, and a rho per robot -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pbc.SHAPES))
@pytest.mark.parametrize("how", ["infinite", "wide"])
def test_limits_that_never_bind_give_the_unlimited_pass_bit_for_bit(host_chain, name, how):
    """±inf limits (no iteration runs) and finite limits a thousand times the largest |k| (the iteration runs and clamps nothing): K, k, P0,
    p0, dV, status, n_cut of `plant_riccati_cases.lq_f64`, robot by robot at its own rho."""
    D, status, (nq, nu, Q, R, Qf, q, r), kw = pbc.case(name)
    B = D.shape[1]
    rho = np.broadcast_to(np.asarray(kw["rho"], dtype=np.float64).reshape(-1), (B,))
    free = [prc.lq_f64(D[:, b:b + 1], status[:, b:b + 1], nq, nu, Q, R, Qf, q=q[:, b:b + 1], r=r[:, b:b + 1], rho=float(rho[b]), keep=kw["keep"])
            for b in range(B)]
    big = 1e3 * max(np.abs(f["k"]).max() for f in free) + np.abs(kw["u_nom"]).max()
    wide = np.inf if how == "infinite" else big
    got = run_host(host_chain, D, status, nq, nu, Q, R, Qf, q, r, rho=kw["rho"], u_lo=np.full((1, nu), -wide), u_hi=np.full((1, nu), wide),
                   u_nom=kw["u_nom"], keep=kw["keep"])
    assert not got["clamped"].any()
    for b in range(B):
        mine = {key: (got[key][:, b:b + 1] if key in ("K", "k") else got[key][b:b + 1]) for key in KEYS}
        mine.update(status=got["status"][b:b + 1], n_cut=got["n_cut"][b:b + 1])
        assert_bitwise(mine, free[b], f"{name}, {how}, robot {b}", clamped=False)
    none = run_host(host_chain, D, status, nq, nu, Q, R, Qf, q, r, rho=kw["rho"], keep=kw["keep"])      # null limits
    assert_bitwise(none, got, f"{name}: null limits")


def test_an_indefinite_G_without_binding_limits_is_the_unlimited_pass(host_chain):
    """R = −0.5 I makes G indefinite at the first step walked (Quu = R + B'Qf B has negative eigenvalues for a small B): the unlimited chain
    solves it by LU all the same, and so does the limited one under infinite limits, bit for bit; under wide finite limits the Newton
    direction is no descent direction and the robot's chain ends at that step, alone."""
    nq, nu, nr, n_cols, T, B = 3, 3, 7, 10, 4, 2
    rng = np.random.default_rng(11)
    D = 0.05 * rng.standard_normal((T, B, nr, n_cols))
    status = np.ones((T, B), dtype=np.int32)
    Q, _, Qf = prc.weights(rng, 2 * nq, nu)
    R = -0.5 * np.eye(nu)
    q, r = rng.standard_normal((T + 1, B, 2 * nq)), rng.standard_normal((T, B, nu))
    free = prc.lq_f64(D, status, nq, nu, Q, R, Qf, q=q, r=r)
    assert free["status"].tolist() == [0, 0] and np.linalg.eigvalsh(R + D[T - 1, 0, :nq, 6:9].T @ Qf[nq:, nq:] @ D[T - 1, 0, :nq, 6:9]).min() < 0
    got = run_host(host_chain, D, status, nq, nu, Q, R, Qf, q, r, u_lo=np.full((1, nu), -np.inf), u_hi=np.full((1, nu), np.inf), u_nom=np.zeros((T, B, nu)))
    assert_bitwise(got, free, "indefinite G, infinite limits", clamped=False)
    wide = run_host(host_chain, D, status, nq, nu, Q, R, Qf, q, r, u_lo=np.full((1, nu), -1e6), u_hi=np.full((1, nu), 1e6), u_nom=np.zeros((T, B, nu)))
    want = pbc.lq_box_f64(D, status, nq, nu, Q, R, Qf, q, r, u_lo=np.full((1, nu), -1e6), u_hi=np.full((1, nu), 1e6), u_nom=np.zeros((T, B, nu)))
    assert_bitwise(wide, want, "indefinite G, wide limits")
    assert wide["status"].tolist() == [1, 1] and not wide["K"].any() and not wide["P0"].any()


def test_a_rho_per_robot_is_the_scalar_chain_at_that_rho(host_chain):
    name = "nu 3, strided block, per-step weights, shared limits, keep 5"
    D, status, args, kw = pbc.case(name)
    rhos = np.array([0.0, 0.75])
    both = run_host(host_chain, D, status, *args, **dict(kw, rho=rhos))
    assert_some_but_not_all_clamp(both["clamped"], args[1], name)
    for b, rho in enumerate(rhos):
        one = run_host(host_chain, D, status, *args, **dict(kw, rho=float(rho)))
        for key in KEYS:
            a, w = (both[key][:, b], one[key][:, b]) if key in ("K", "k") else (both[key][b], one[key][b])
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(w).tobytes(), (key, b)
        assert both["clamped"][:, b].tolist() == one["clamped"][:, b].tolist() and both["status"][b] == one["status"][b]
    assert both["K"][:, 0].tobytes() != both["K"][:, 1].tobytes()


def test_with_every_control_clamped_the_gain_is_zero_and_the_chain_goes_on(host_chain):
    """u_lo = u_hi: every control is clamped at every step.  K_t = 0, k_t = the bound u_lo − u_nom[t] exactly, and the chain walks on through
    all of them, as the restatement does."""
    name = "nu 3, strided block, per-step weights, shared limits, keep 5"
    D, status, args, kw = pbc.case(name)
    nu, T = args[1], D.shape[0]
    kw = dict(kw, keep=None)
    width = kw["u_hi"] - kw["u_lo"]
    u_lo = kw["u_lo"] + 0.25 * width
    u_hi = u_lo.copy()                                    # lo == hi: every control is clamped at every step
    got = run_host(host_chain, D, status, *args, **dict(kw, u_lo=u_lo, u_hi=u_hi))
    want = pbc.lq_box_f64(D, status, *args, **dict(kw, u_lo=u_lo, u_hi=u_hi))
    assert_bitwise(got, want, "lo == hi")
    assert got["status"].tolist() == [0, 0] and (got["clamped"] == (1 << nu) - 1).all()
    assert not got["K"].any() and got["P0"].any()
    assert np.array_equal(got["k"], u_lo[None] - kw["u_nom"])


# ---- the value of the returned policy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nu 2, six steps, two robots, a rho each", "nu 3, strided block, per-step weights, shared limits, keep 5",
                                  "nu 12, the largest model"])
def test_the_value_is_the_cost_of_the_returned_policy(name):
    """½ x0'P0 x0 + p0'x0 + dV1 + dV2 of `lq_box_ld` is the cost of δu = k − K δx (the returned, unclamped policy) rolled through the linear
    model from any x0, for any rho and any clamped set: P and p are updated in the policy-evaluation form and the constant collects
    k'Qu + ½ k'Quu k whatever k is.  The identity needs symmetric weights (−K'(R k) is the cross term of ½ u'R u only then), so this test takes
    the case without its non-symmetric part.  The bound and its reason are `test_plant_riccati`'s: 1e-15 of the sum of the cost's |terms|."""
    D, status, (nq, nu, Q, R, Qf, q, r), kw = pbc.case(name, symmetric=True)
    kw = dict(kw, keep=None)
    ld = pbc.lq_box_ld(D, status, nq, nu, Q, R, Qf, q, r, **kw)
    assert_some_but_not_all_clamp(ld["clamped"], nu, name)
    rng = np.random.default_rng(3)
    for b in range(D.shape[1]):
        x0 = rng.standard_normal(2 * nq)
        _, _, terms = tpr._policy_rollout(D, b, nq, nu, Q, R, Qf, q, r, ld["K"], ld["k"], x0)
        x = np.asarray(x0, dtype=LD)
        value = LD(0.5) * gr.mm_ld(x, gr.mm_ld(ld["P0"][b], x)) + gr.mm_ld(ld["p0"][b], x) + ld["dV"][b, 0] + ld["dV"][b, 1]
        cost, mag = sum(terms), sum(abs(v) for v in terms)
        print(f"{name}, robot {b}: cost {float(cost):.12e}, value {float(value):.12e}, gap {float(abs(cost - value) / mag):.2e} of the terms")
        assert float(abs(cost - value)) <= 1e-15 * float(mag)


# ---- the limiter ----------------------------------------------------------------------------------------------------------------------------
def test_the_limiter(host_chain):
    """u < lo ? lo : (u > hi ? hi : u), bit for bit: inside, outside, ON a bound (-0.0 against a bound of 0.0 tells < from <=: the strict
    comparison returns u = -0.0, a non-strict one the bound +0.0), lo == hi, infinite bounds and a NaN u, which passes through."""
    inf, nan = np.inf, np.nan
    rows = [(0.5, -1.0, 1.0, 0.5), (-2.0, -1.0, 1.0, -1.0), (2.0, -1.0, 1.0, 1.0), (-0.0, 0.0, 1.0, -0.0), (0.0, -1.0, -0.0, 0.0),
            (3.0, 2.0, 2.0, 2.0), (1.0, 2.0, 2.0, 2.0), (2.0, 2.0, 2.0, 2.0), (1e300, -inf, inf, 1e300), (-1e300, -inf, 0.0, -1e300),
            (inf, -inf, inf, inf), (inf, -1.0, 1.0, 1.0), (-inf, -1.0, 1.0, -1.0), (nan, -1.0, 1.0, nan), (nan, -inf, inf, nan)]
    text = f"{len(rows)}\n" + " ".join(float(v).hex() for row in rows for v in row[:3]) + "\n"
    res = subprocess.run([host_chain, "limit"], input=text, capture_output=True, text=True, check=True)
    got = np.array([float.fromhex(v) for v in res.stdout.split()])
    want = np.array([row[3] for row in rows])
    mine = np.array([float(pbc.limit(*row[:3])) for row in rows])
    for g, w, mi, row in zip(got, want, mine, rows):
        if np.isnan(w):
            assert np.isnan(g) and np.isnan(mi), row
        else:
            assert g == w and np.signbit(g) == np.signbit(w) and mi == w and np.signbit(mi) == np.signbit(w), row


# ---- the export, its signature, its Julia call and its refusals -----------------------------------------------------------------------------
def test_the_export_is_declared_and_bound():
    params = tpr._prototype(NAME)
    assert NAME in _lib.SIGNATURES, f"{NAME} has no ctypes signature"
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(params) == 24
    assert [tpr.CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), NAME)


def test_julia_call_matches_the_prototype():
    import re
    assert "function plant_tape_lqr_box(" in tpr.JL, "julia/CIMPCHip.jl has no plant_tape_lqr_box"
    fn = tpr.JL[tpr.JL.index("function plant_tape_lqr_box("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\." + NAME + r"\((.*?)\)::Cint", fn, flags=re.S)
    assert m, f"plant_tape_lqr_box does not call {NAME}"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    params = tpr._prototype(NAME)
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in tpr.JL_COMPAT[jt], f"argument {k}: Julia {jt} against C `{ct}`"


# what is changed in the stand-in call -> the reason left for cimpc_last_error(NULL).  The stand-in tape is zeroed memory: model 0, B = 0.
REFUSED = {
    "u_lo above u_hi": (dict(u_lo=[[0.5]], u_hi=[[0.25]]), "u_lo above u_hi"),
    "a NaN limit": (dict(u_hi=[[float("nan")]]), "a NaN limit"),
    "n_lim = 3": (dict(n_lim=3), "n_lim neither 1 nor B"),
    "n_rho = 2": (dict(rho=[0.0, 0.0]), "n_rho neither 1 nor B"),
    "limits without u_nom": (dict(u_nom=None), "limits without u_nom"),
    "limits without q, r": (dict(lin=False), "limits without q, r"),
    "limits with laps = 2": (dict(laps=2), "limits with laps > 1"),
    "u_lo alone": (dict(u_hi=None), "one of u_lo, u_hi without the other"),
    "a negative rho": (dict(rho=[-1e-3]), "a rho that is negative or not finite"),
    "a NaN rho": (dict(rho=[float("nan")]), "a rho that is negative or not finite"),
    "clamped without q, r": (dict(lin=False, u_lo=None, u_hi=None, u_nom=None), "a rho per robot or clamped without q, r"),
    "a zeroed tape": (dict(), "a closed or empty tape"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_the_entry_refuses_by_reason_without_a_device(what):
    change, reason = REFUSED[what]
    stand_in = C.cast(C.create_string_buffer(4096), C.c_void_p)
    n, T, B = 4, 3, 1
    nu = 16                                                     # more than any model's nu: the limits' scan stays inside the arrays
    a = dict(laps=1, lin=True, rho=[0.0], n_lim=1, u_lo=[[-1.0] * nu], u_hi=[[1.0] * nu], u_nom=np.zeros((T, B, nu)))
    a.update(change)
    for key in ("u_lo", "u_hi"):
        if a[key] is not None and len(a[key][0]) == 1:
            a[key] = [[a[key][0][0]] * nu]
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib._dp)
    ip = lambda x: x.ctypes.data_as(_lib._ip)
    Q, Qf, R, q, r = np.eye(n), np.eye(n), np.eye(nu), np.zeros((T + 1, B, n)), np.zeros((T, B, nu))
    K, k, status, n_cut, clamped = np.zeros((1, B, n, nu)), np.zeros((1, B, nu)), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros((1, B), dtype=np.int32)
    rho, u_lo, u_hi, u_nom = arr(a["rho"]), arr(a["u_lo"]), arr(a["u_hi"]), arr(a["u_nom"])
    lib = _lib.load()
    rc = lib.cimpc_plant_tape_lqr_box(stand_in, a["laps"], 1, dp(Q), dp(Qf), 1, dp(R), dp(q) if a["lin"] else None, dp(r) if a["lin"] else None,
                                      rho.size, dp(rho), 1, dp(K), dp(k) if a["lin"] else None, None, None, None, ip(status), ip(n_cut),
                                      a["n_lim"], dp(u_lo), dp(u_hi), dp(u_nom), ip(clamped))
    assert rc == INVALID
    assert lib.cimpc_last_error(None).decode() == NAME + ": " + reason


# ---- the limited closed loop and the limited line search: exports, Julia calls, refusals ------------------------------------------------------
OTHER_CTYPE = dict(tpr.CTYPE, **{"const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts),
                                  "const cimpc_feedback*": C.POINTER(_lib.Feedback), "const cimpc_tracking_cost*": C.POINTER(_lib.TrackingCost),
                                  "cimpc_plant_tape*": C.POINTER(C.c_void_p)})
OTHER_JL = dict(tpr.JL_COMPAT, **{"Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"}, "Ref{Feedback}": {"const cimpc_feedback*"},
                                  "Ref{TrackingCostC}": {"const cimpc_tracking_cost*"}, "Ref{Ptr{Cvoid}}": {"cimpc_plant_tape*"}})
OTHERS = {"cimpc_plant_rollout_feedback_limits": ("cimpc_plant_rollout_feedback", "plant_rollout_feedback_limits", ["int", "const double*", "const double*"]),
          "cimpc_plant_tape_linesearch_box": ("cimpc_plant_tape_linesearch", "plant_tape_linesearch_box", ["int", "const double*", "const double*"])}


@pytest.mark.parametrize("name", sorted(OTHERS))
def test_the_other_two_exports_extend_their_siblings(name):
    """Declared in include/cimpc.h as the sibling's parameters plus (n_lim, u_lo, u_hi), bound with matching ctypes, called from Julia with
    matching types."""
    import re
    sibling, jl_name, more = OTHERS[name]
    params = tpr._prototype(name)
    assert params == tpr._prototype(sibling) + more
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args == [OTHER_CTYPE[p] for p in params] and args[:-3] == _lib.SIGNATURES[sibling][1]
    assert hasattr(_lib.load(), name)
    assert f"function {jl_name}(" in tpr.JL
    fn = tpr.JL[tpr.JL.index(f"function {jl_name}("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint", fn, flags=re.S)
    assert m, f"{jl_name} does not call {name}"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    assert len(types) == len(params)
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in OTHER_JL[jt], f"argument {k}: Julia {jt} against C `{ct}`"


LOOP_REFUSED = {"u_lo above u_hi": (dict(u_lo=0.5, u_hi=0.25), "u_lo above u_hi"), "a NaN limit": (dict(u_lo=float("nan")), "a NaN limit"),
                "n_lim = 3": (dict(n_lim=3), "n_lim neither 1 nor B"), "null u_hi": (dict(u_hi=None), "a null u_lo or u_hi"),
                "an unknown model": (dict(model=999), "a model without controls"),
                "null trajectory": (dict(), "an argument that cimpc_plant_rollout_feedback refuses")}


@pytest.mark.parametrize("what", sorted(LOOP_REFUSED))
def test_the_limited_closed_loop_refuses_by_reason_without_a_device(what):
    """The limits are tested first; the last case has good limits and nothing else, which the rollout's own check (no device either) refuses."""
    change, reason = LOOP_REFUSED[what]
    from contactimplicitmpc.jl_amd import plant
    a = dict(model=plant.model_dims("hopper_2D")[0], n_lim=1, u_lo=-1.0, u_hi=1.0)
    a.update(change)
    lim = lambda v: None if v is None else np.full((1, 16), v)
    lo, hi = lim(a["u_lo"]), lim(a["u_hi"])
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib._dp)
    lib = _lib.load()
    rc = lib.cimpc_plant_rollout_feedback_limits(a["model"], 2, 3, 0, 0, None, None, None, None, 1, 1, 1, None, 1, 1, 1, None, 1, 0.01, None, None, None, None,
                                                 None, None, None, None, None, a["n_lim"], dp(lo), dp(hi))
    assert rc == INVALID
    assert lib.cimpc_last_error(None).decode() == "cimpc_plant_rollout_feedback_limits: " + reason


def test_python_refuses_limits_where_the_clamps_derivative_would_be_needed():
    """`Feedback(u_lo=, u_hi=)` is checked on the host - shapes, NaN, order - and a call that asks for gradients refuses it by name, before
    any device call."""
    from contactimplicitmpc.jl_amd import plant
    nq, nu, B, T = 4, 2, 3, 5
    K, x_ref = np.zeros((T, nu, 2 * nq)), np.zeros((T, 2 * nq))
    args = ("hopper_2D", np.zeros((B, nq)), np.zeros((B, nq)), np.zeros((T, nu)), 0.01, 0.5)
    for bad, match in ((dict(u_lo=[-1.0, -1.0]), "go together"), (dict(u_lo=[-1.0], u_hi=[1.0]), "must be"), (dict(u_lo=[0.0, np.nan], u_hi=[1.0, 1.0]), "NaN"),
                       (dict(u_lo=[2.0, 0.0], u_hi=[1.0, 1.0]), "must not exceed"), (dict(u_lo=np.zeros((2, nu)), u_hi=np.ones((2, nu))), "must be")):
        with pytest.raises(ValueError, match=match):
            plant.rollout(*args, feedback=plant.Feedback(K, x_ref, **bad))
    limited = plant.Feedback(K, x_ref, u_lo=[-1.0, -np.inf], u_hi=[1.0, np.inf])
    with pytest.raises(ValueError, match="derivative of the clamp"):
        plant.rollout(*args, feedback=limited, diff_sol=True)
    with pytest.raises(ValueError, match="derivative of the clamp"):
        plant.rollout_tape(*args, feedback=limited)


# ---- limited iLQR in flight, on the CPU plant ------------------------------------------------------------------------------------------------
def test_limited_ilqr_in_flight_on_the_cpu_plant():
    """`ilqr_cpu_box` on the two particles of `plant_linesearch_cases.flight_case` under a thrust limit that binds (half of what each
    particle's unlimited LQ step asks for): both accept both iterations, every nominal's controls lie in the box exactly, some sit on it
    and some do not, and the largest projected gradient of J over the horizon (longdouble adjoint chain on the nominal's own blocks) falls
    from 1.73e-1 to 7.35e-3 in two iterations (4.2 %; two more bring it to 6.8e-12, which is the plant's own noise and is not held).
    The bound below is a property of the algorithm, not that figure: two iterations must cut it below a tenth."""
    import plant_linesearch_cases as plc
    its = pbc.flight_cpu()
    u_lo, u_hi = pbc.flight_limits()
    assert len(its) == pbc.FLIGHT_ITERATIONS == 2
    J = its[0]["J_nom"]
    for n, it in enumerate(its):
        assert it["accepted"].all() and it["status"].tolist() == [0, 0], f"iteration {n + 1}"
        assert (it["J_new"] < J).all()
        J = it["J_new"]
        assert np.all(it["u"] >= u_lo[None]) and np.all(it["u"] <= u_hi[None])
        on = (it["u"] == u_lo[None]) | (it["u"] == u_hi[None])
        assert 0 < on.sum() < on.size
        assert_some_but_not_all_clamp(it["clamped"], 3, f"flight, iteration {n + 1}")
    start, end = its[0]["pg"], its[-1]["pg_end"]
    print(f"flight: projected gradient {start:.3e} -> {end:.3e} ({end / start:.3e} of the start), J {its[0]['J_nom']} -> {J}")
    assert end <= 0.1 * start


# ---- the sanitizers -------------------------------------------------------------------------------------------------------------------------
def test_the_host_build_runs_clean_under_the_sanitizers(tmp_path):
    """The same program stand-alone with -fsanitize=address,undefined: every case, the work array sized exactly as the kernel's LDS."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "plant_boxqp_check_san")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, SRC], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr[-300:])
    for name in sorted(pbc.SHAPES):
        D, status, args, kw = pbc.case(name)
        assert_bitwise(run_host(exe, D, status, *args, **kw), pbc.lq_box_f64(D, status, *args, **kw), name)


def test_the_plan_keeps_two_workgroups_a_cu_for_every_model(host_chain):
    import re
    text = open(os.path.join(tpr.ROOT, "contactimplicitmpc", "jl_amd", "csrc", "model_table.h")).read()
    rows = re.findall(r"X\((\w+), (\d+), (\d+), (\d+), (\d+), (\d+), \d\)", text)
    assert len(rows) >= 10
    for name, nq, nu, *_ in rows:
        nq, nu = int(nq), int(nu)
        if nu < 1:
            continue
        out = subprocess.run([host_chain, "plan", str(nq), str(nu)], capture_output=True, text=True, check=True)
        lds, share = (int(v) for v in out.stdout.split())
        assert share == nu * nu + 7 * nu + 2, name
        n, m = 2 * nq, nu
        assert lds == 8 * (2 * n * n + 2 * nq * (n + m) + 2 * nq * n + m * nq + 3 * m * n + m * (n + 1) + 2 * m * m + 2 * n + 3 * m + nq + 4 + share), name
        assert 2 * lds <= 160 * 1024, (name, lds)
