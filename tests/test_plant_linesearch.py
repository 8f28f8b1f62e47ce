"""The tracking cost and the line search (`cimpc_plant_tracking_cost`, `cimpc_plant_tape_linesearch`, `TrackingCost`, `RolloutTape.linesearch`,
`plant.ilqr`) without a device: the exports, their ctypes signatures and Julia calls; csrc/plant_cost.h built
with g++ and run by a team of one against the ordered float64 restatement `cost_f64` of tests/plant_linesearch_cases.py bit for bit,
within the bounds of the longdouble restatement, and its linear terms against the analytic gradient; the same program under
AddressSanitizer and UBSan; the acceptance rule, the choice and the candidate-control formula case by case; every refusal of the entry's
check; `cimpc_plant_tracking_cost` through ctypes; and the iLQR restatement on the CPU plant, which fixes the tolerances of the device's
flight test.

Measured (this file's shapes): the host build and `cimpc_plant_tracking_cost` equal `cost_f64` bit for bit at every shape, also under the
sanitizers; `cost_f64` is at most 3.4e-16 from `cost_ld` (bounds from 2.2e-14); one full step of `ilqr_cpu` in flight is 2.7e-9 (controls,
relative to the LQ step) and 1.6e-10 (decrease, relative to dV1 + dV2) from the longdouble LQ optimum."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, plant
import plant_adjoint_cases as pac
import plant_gradient_cases as pgc
import plant_linesearch_cases as plc
import plant_riccati_cases as prc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
SRC = os.path.join(HERE, "native", "plant_cost_check.cpp")
INVALID = -1
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip, "cimpc_plant_tape": C.c_void_p,
         "cimpc_plant_tape*": C.POINTER(C.c_void_p), "const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts),
         "const cimpc_tracking_cost*": C.POINTER(_lib.TrackingCost)}
JL_COMPAT = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*"}, "Ptr{Cvoid}": {"cimpc_plant_tape"},
             "Ref{Ptr{Cvoid}}": {"cimpc_plant_tape*"}, "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"},
             "Ref{TrackingCostC}": {"const cimpc_tracking_cost*"}}
ENTRIES = {"cimpc_plant_tracking_cost": ("plant_tracking_cost", 10), "cimpc_plant_tape_linesearch": ("plant_tape_linesearch", 36)}


# ---- the exports ------------------------------------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_exports_are_declared_and_bound(name):
    params = _prototype(name)
    assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(params) == ENTRIES[name][1]
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), name)


def test_the_cost_struct_mirrors_the_header():
    body = re.search(r"typedef struct cimpc_tracking_cost\s*\{(.*?)\}\s*cimpc_tracking_cost\s*;", HDR, flags=re.S).group(1)
    names = [n.strip() for stmt in body.split(";") if stmt.strip() for n in stmt.replace("const double*", "").replace("int", "").split(",")]
    assert names == [f[0] for f in _lib.TrackingCost._fields_] == ["Q", "Qf", "R", "x_goal", "u_goal", "n_Q", "n_R", "n_x"]
    jl = re.search(r"struct TrackingCostC\n(.*?)\nend", JL, flags=re.S)
    assert jl, "julia/CIMPCHip.jl has no TrackingCostC"
    assert [d.split("::")[0].strip() for line in jl.group(1).split("\n") for d in line.split("#")[0].split(";") if "::" in d] == names


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_julia_calls_match_the_prototypes(name):
    fn_name = ENTRIES[name][0]
    assert f"function {fn_name}(" in JL, f"julia/CIMPCHip.jl has no {fn_name}"
    fn = JL[JL.index(f"function {fn_name}("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint", fn, flags=re.S)
    assert m, f"{fn_name} does not call {name}"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    params = _prototype(name)
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in JL_COMPAT[jt], f"argument {k}: Julia {jt} against C `{ct}`"


# ---- csrc/plant_cost.h on the host ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("cost") / "plant_cost_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", exe, SRC])
    return exe


# name: (nq, nu, T, B, per-step weights, per-robot goals)
SHAPES = {"nq 3, one step, shared goals": (3, 3, 1, 1, False, False), "nq 3, T weight blocks, goals per robot": (3, 3, 5, 2, True, True),
          "nq 4, goals per robot": (4, 2, 14, 3, False, True), "nq 4, one step, T weight blocks": (4, 2, 1, 2, True, False),
          "nq 11, shared goals": (11, 8, 6, 2, False, False), "nq 11, T weight blocks, goals per robot": (11, 8, 3, 2, True, True),
          "nq 18, goals per robot": (18, 12, 2, 2, False, True), "nq 18, one step, T weight blocks, shared goals": (18, 12, 1, 1, True, False)}


def _case(name, symmetric=False):
    """(q, u, Q, R, Qf, x_goal, u_goal); the weights are not symmetric unless asked for, so that a transposed block shows."""
    nq, nu, T, B, per_step, per_robot = SHAPES[name]
    rng = np.random.default_rng([1, sorted(SHAPES).index(name)])
    Q, R, Qf = prc.weights(rng, 2 * nq, nu, T, per_step)
    if not symmetric:
        Q, R, Qf = (M + 0.1 * rng.standard_normal(M.shape) for M in (Q, R, Qf))
    n_x = B if per_robot else 1
    return (rng.standard_normal((T + 2, B, nq)), rng.standard_normal((T, B, nu)), Q, R, Qf, rng.standard_normal((T + 1, n_x, 2 * nq)),
            rng.standard_normal((T, n_x, nu)))


def _hex(*arrays):
    return " ".join(float(v).hex() for a in arrays for v in np.asarray(a, dtype=np.float64).ravel())


def _run(exe, mode, text):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.strip("\n").split("\n")


def _run_cost(exe, q, u, Q, R, Qf, xg, ug):
    T, B, nu = u.shape
    nq = q.shape[2]
    col = lambda M: np.swapaxes(M, -1, -2)      # the header reads column-major blocks
    head = f"{B} {T} {nq} {nu} {1 if Q.ndim == 2 else T} {1 if R.ndim == 2 else T} {xg.shape[1]} "
    lines = _run(exe, "cost", head + _hex(q, u, col(Q), col(Qf), col(R), xg, ug))
    vals = [np.array([float.fromhex(t) for t in line.split()]) for line in lines]
    return vals[0], vals[1].reshape(T + 1, B, 2 * nq), vals[2].reshape(T, B, nu)


def _bitwise(got, ref, what):
    for name, g, r in zip(("J", "lin_q", "lin_r"), got, ref):
        assert g.shape == r.shape and g.tobytes() == np.ascontiguousarray(r).tobytes(), f"{what}: {name} differs from the float64 restatement"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_header_equals_the_ordered_restatement_and_sits_within_the_longdouble_bounds(host, name):
    case = _case(name)
    got = _run_cost(host, *case)
    _bitwise(got, plc.cost_f64(*case), name)
    ld, f64, bound = plc.cost_bounds(*case)
    for key, g in zip(("J", "lin_q", "lin_r"), got):
        dist = pac.distance(g, ld[key])
        print(f"{name}, {key}: {dist:.2e} from cost_ld (bound {bound[key]:.2e})")
        assert dist <= bound[key], f"{name} {key}: {dist:.3e} > {bound[key]:.3e}"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_linear_terms_are_the_gradient_of_the_cost(host, name):
    """lin_q, lin_r against the longdouble restatement's analytic gradient (the weights are symmetric), and the gradient against a central
    difference of the longdouble cost along a random direction."""
    q, u, Q, R, Qf, xg, ug = _case(name, symmetric=True)
    _, lin_q, lin_r = _run_cost(host, q, u, Q, R, Qf, xg, ug)
    J, _, _, gx, gu = plc.cost_ld(q, u, Q, R, Qf, xg, ug)
    assert pac.distance(lin_q, gx) <= 1e-13 and pac.distance(lin_r, gu) <= 1e-13
    rng = np.random.default_rng(2)
    dq, du, eps = rng.standard_normal(q.shape), rng.standard_normal(u.shape), plc.LD(1e-6)
    Jp = plc.cost_ld(q.astype(plc.LD) + eps * dq, u.astype(plc.LD) + eps * du, Q, R, Qf, xg, ug)[0]
    Jm = plc.cost_ld(q.astype(plc.LD) - eps * dq, u.astype(plc.LD) - eps * du, Q, R, Qf, xg, ug)[0]
    dx = np.concatenate([dq[:-1], dq[1:]], axis=2)
    slope = np.einsum("tbi,tbi->b", gx, dx) + np.einsum("tbi,tbi->b", gu, du)
    assert pac.distance((Jp - Jm) / (2 * eps), slope) <= 1e-9      # a quadratic: the central difference is exact up to rounding


def test_the_host_build_runs_clean_under_the_sanitizers(tmp_path):
    """The same program stand-alone with -fsanitize=address,undefined: every shape, the work array sized exactly as a workgroup's LDS."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "plant_cost_check_san")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, SRC], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr[-300:])
    for name in sorted(SHAPES):
        case = _case(name)
        _bitwise(_run_cost(exe, *case), plc.cost_f64(*case), name)
    assert _accept(exe, 1e-4, [1.0, 0.5], [[1], [1]], [[2.0], [1.0]], [3.0], [[-1.0, 0.5]]) == ([[1], [1]], [1])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tracking_cost_through_ctypes_equals_the_restatement(name):
    q, u, Q, R, Qf, xg, ug = _case(name)
    got = plant.TrackingCost(Q, R, Qf, x_goal=xg, u_goal=ug).evaluate(q, u)
    _bitwise(got, plc.cost_f64(q, u, Q, R, Qf, xg, ug), name)


def test_tracking_cost_defaults():
    q, u, Q, R, Qf, xg, ug = _case("nq 4, one step, T weight blocks")
    got = plant.TrackingCost(Q, R).evaluate(q, u)
    _bitwise(got, plc.cost_f64(q, u, Q, R, Q[-1], np.zeros_like(xg), np.zeros_like(ug)), "defaults")
    with pytest.raises(ValueError):
        plant.TrackingCost(Q[:, :3], R).evaluate(q, u)
    with pytest.raises(ValueError):
        plant.TrackingCost(Q, R, x_goal=np.zeros((3, 5))).evaluate(q, u)


# ---- the rules ------------------------------------------------------------------------------------------------------------------------------
def _accept(exe, armijo, alpha, conv, J, J_nom, dV):
    """conv and J (n_alpha, B), J_nom (B), dV (B, 2) -> (ok (n_alpha, B), choice (B)) as the header's two rules give them."""
    conv, J = np.asarray(conv, dtype=int), np.asarray(J, dtype=float)
    assert conv.shape == J.shape == (len(alpha), len(J_nom))
    B = J.shape[1]
    text = f"{len(alpha)} {B} {float(armijo).hex()} {_hex(alpha)} " + " ".join(str(int(v)) for v in conv.ravel()) + " " + _hex(J, J_nom, dV)
    ok, choice = _run(exe, "accept", text)
    return np.array(ok.split(), dtype=int).reshape(len(alpha), B).tolist(), [int(v) for v in choice.split()]


INF, NAN = float("inf"), float("nan")
# name: (armijo, alpha, converged (n_alpha, B), J (n_alpha, B), J_nom (B), dV (B, 2))
RULE = {
    "the least J of the acceptable wins": (1e-4, [1.0, 0.5, 0.25], [[1], [1], [1]], [[2.0], [1.5], [2.5]], [3.0], [[-1.0, 0.5]]),
    "a non-finite J is not acceptable": (1e-4, [1.0, 0.5, 0.25], [[1], [1], [1]], [[NAN], [-INF], [2.5]], [3.0], [[-1.0, 0.5]]),
    "an unconverged step is not acceptable": (1e-4, [1.0, 0.5], [[0], [1]], [[1.0], [2.0]], [3.0], [[-1.0, 0.5]]),
    "a tie goes to the lower index": (1e-4, [1.0, 0.5, 0.25], [[1], [1], [1]], [[2.0], [1.0], [1.0]], [3.0], [[-1.0, 0.5]]),
    "armijo 0 accepts equality": (0.0, [1.0, 0.0], [[1], [1]], [[3.5], [3.0]], [3.0], [[-1.0, 0.5]]),
    "armijo 0 refuses an increase": (0.0, [1.0], [[1]], [[3.0000000000000004]], [3.0], [[-1.0, 0.5]]),
    "not enough decrease": (0.5, [1.0], [[1]], [[2.9]], [3.0], [[-1.0, 0.5]]),
    "none acceptable": (1e-4, [1.0, 0.5], [[1], [0]], [[4.0], [1.0]], [3.0], [[-1.0, 0.5]]),
    "J_nom -inf rejects all": (1e-4, [1.0, 0.0], [[1], [1]], [[1.0], [1.0]], [-INF], [[-1.0, 0.5]]),
    "J_nom +inf accepts every finite J": (1e-4, [1.0, 0.5], [[1], [1]], [[7.0], [9.0]], [INF], [[-1.0, 0.5]]),
    "a NaN dV rejects": (1e-4, [1.0], [[1]], [[1.0]], [3.0], [[NAN, 0.5]]),
    "two robots choose apart": (1e-4, [1.0, 0.5], [[1, 0], [1, 1]], [[1.0, 0.5], [2.0, 2.5]], [3.0, 3.0], [[-1.0, 0.5], [-1.0, 0.5]]),
}


@pytest.mark.parametrize("name", sorted(RULE))
def test_the_acceptance_rule_and_the_choice(host, name):
    armijo, alpha, conv, J, J_nom, dV = RULE[name]
    ok, choice = _accept(host, armijo, alpha, conv, J, J_nom, dV)
    J, conv = np.asarray(J), np.asarray(conv)
    want_ok = [[int(plc.acceptable(conv[c, b], J[c, b], J_nom[b], armijo, alpha[c], dV[b][0], dV[b][1])) for b in range(J.shape[1])] for c in range(len(alpha))]
    want = [plc.choose(J[:, b], np.asarray(want_ok)[:, b]) for b in range(J.shape[1])]
    assert ok == want_ok and choice == want
    expected = {"the least J of the acceptable wins": [1], "a non-finite J is not acceptable": [2], "an unconverged step is not acceptable": [1],
                "a tie goes to the lower index": [1], "armijo 0 accepts equality": [1], "armijo 0 refuses an increase": [-1], "not enough decrease": [-1],
                "none acceptable": [-1], "J_nom -inf rejects all": [-1], "J_nom +inf accepts every finite J": [0], "a NaN dV rejects": [-1],
                "two robots choose apart": [0, 1]}
    assert choice == expected[name]


def test_the_candidate_control_is_one_product_and_one_sum(host):
    rng = np.random.default_rng(4)
    u, a, k = rng.standard_normal(64), rng.standard_normal(64), rng.standard_normal(64) * 1e3
    a[:4] = 0.0
    text = "64 " + " ".join(f"{float(x).hex()} {float(y).hex()} {float(z).hex()}" for x, y, z in zip(u, a, k))
    got = np.array([float.fromhex(t) for t in _run(host, "control", text)[0].split()])
    want = plc.candidate_controls(u, a, k)
    assert got.tobytes() == want.tobytes()
    assert got[:4].tobytes() == u[:4].tobytes()      # alpha 0 leaves the nominal control
    fused = np.array([float(np.longdouble(x) + np.longdouble(y) * np.longdouble(z)) for x, y, z in zip(u, a, k)])
    assert (fused != want).any(), "the sample tells a fused multiply-add from two roundings"


# ---- every refusal of the entry's check --------------------------------------------------------------------------------------------------------
def _linesearch_args(**over):
    """A call of cimpc_plant_tape_linesearch on stand-in memory (zeroed: a tape that a later check refuses), every pointer set."""
    nq, nu, nc, nb, T, B, na = 4, 2, 1, 2, 3, 1, 2
    z = lambda *s: np.zeros(s)
    zi = lambda *s: np.zeros(s, dtype=np.int32)
    a = dict(tape=C.cast(C.create_string_buffer(4096), C.c_void_p), steps_per_launch=0, n_terrain=0, terrain=None, q_nom=z(T + 2, B, nq), u_nom=z(T, B, nu),
             w=None, K_w=1, n_w=1, hold_w=1, mu=np.array([0.5]), n_mu=1, h=0.01, opts=_lib.IpOpts(**plant.dataclasses.asdict(plant.SIM_OPTS)),
             K=z(T, B, 2 * nq, nu), k=z(T, B, nu), dV=z(B, 2), J_nom=z(B), n_alpha=na, alpha=np.array([1.0, 0.5]), armijo=1e-4,
             cost=plant.TrackingCost(np.eye(2 * nq), np.eye(nu))._struct(nq, nu, B, T), reg=1e-9, J=z(na, B), ok=zi(na, B), choice=zi(B), q=z(T + 2, B, nq),
             u_applied=z(T, B, nu), gamma=z(T, B, nc), b=z(T, B, nb), status=zi(T, B), iters=zi(T, B), lin_q=z(T + 1, B, 2 * nq), lin_r=z(T, B, nu),
             grad_status=zi(T, B), new_tape=C.c_void_p(77))
    a.update(over)
    return a


def _call_linesearch(a):
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib._dp)
    ip = lambda x: None if x is None else x.ctypes.data_as(_lib._ip)
    cost = a["cost"]
    return _lib.load().cimpc_plant_tape_linesearch(
        a["tape"], a["steps_per_launch"], a["n_terrain"], a["terrain"], dp(a["q_nom"]), dp(a["u_nom"]), dp(a["w"]), a["K_w"], a["n_w"], a["hold_w"],
        dp(a["mu"]), a["n_mu"], a["h"], None if a["opts"] is None else C.byref(a["opts"]), dp(a["K"]), dp(a["k"]), dp(a["dV"]), dp(a["J_nom"]), a["n_alpha"],
        dp(a["alpha"]), a["armijo"], None if cost is None else C.byref(cost[0]), a["reg"], dp(a["J"]), ip(a["ok"]), ip(a["choice"]), dp(a["q"]),
        dp(a["u_applied"]), dp(a["gamma"]), dp(a["b"]), ip(a["status"]), ip(a["iters"]), dp(a["lin_q"]), dp(a["lin_r"]), ip(a["grad_status"]),
        None if a["new_tape"] is None else C.byref(a["new_tape"]))


POINTERS = ("tape", "q_nom", "u_nom", "mu", "opts", "K", "k", "dV", "J_nom", "alpha", "cost", "J", "ok", "choice", "q", "u_applied", "gamma", "b", "status",
            "iters", "lin_q", "lin_r", "grad_status", "new_tape")


def _cost_struct(**over):
    """The stand-in call's cost with one field changed; (struct, the arrays it points to)."""
    cc, keep = plant.TrackingCost(np.eye(8), np.eye(2))._struct(4, 2, 1, 3)
    for k, v in over.items():
        setattr(cc, k, v)
    return cc, keep


# what is changed in the stand-in call -> the reason the entry leaves for cimpc_last_error(NULL).  The stand-in tape is zeroed memory (a
# closed tape), so every reason but the last is one the entry finds BEFORE it looks at the tape: a test fails if its check is missing
REFUSED = {f"null {p}": ({p: None}, f"null {p}") for p in POINTERS}
REFUSED.update({"n_alpha 0": (dict(n_alpha=0), "n_alpha outside 1 .. 64"), "n_alpha 65": (dict(n_alpha=65, alpha=np.ones(65)), "n_alpha outside 1 .. 64"),
                "alpha NaN": (dict(alpha=np.array([1.0, NAN])), "a non-finite alpha"), "alpha infinite": (dict(alpha=np.array([INF, 0.5])), "a non-finite alpha"),
                "armijo negative": (dict(armijo=-1e-4), "armijo negative or not a number"), "armijo NaN": (dict(armijo=NAN), "armijo negative or not a number"),
                "null Qf in the cost": (dict(cost=_cost_struct(Qf=None)), "a null pointer in the cost"),
                "null u_goal in the cost": (dict(cost=_cost_struct(u_goal=None)), "a null pointer in the cost"),
                "n_Q 0 in the cost": (dict(cost=_cost_struct(n_Q=0)), "n_Q, n_R or n_x of the cost below 1"),
                "n_x -1 in the cost": (dict(cost=_cost_struct(n_x=-1)), "n_Q, n_R or n_x of the cost below 1"),
                "h 0": (dict(h=0.0), "h not positive"), "h NaN": (dict(h=NAN), "h not positive"),
                "a closed tape": (dict(), "a closed tape")})


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_linesearch_refuses_invalid_arguments_without_a_device(what):
    over, reason = REFUSED[what]
    a = _linesearch_args(**over)
    assert _call_linesearch(a) == INVALID
    assert _lib.load().cimpc_last_error(None).decode() == "cimpc_plant_tape_linesearch: " + reason
    if a["new_tape"] is not None:
        assert a["new_tape"].value is None, "a refused call leaves *new_tape null"


def test_the_sizes_the_check_refuses(host):
    """plant_linesearch_refusal case by case, and plant_linesearch_fits on sizes no stand-in tape can carry: n_alpha B T beyond an int, B or
    T below 1."""
    def valid(na, armijo, B, T, alpha):
        why, fits = _run(host, "valid", f"{na} {float(armijo).hex()} {B} {T} {_hex(alpha)}")
        return why, int(fits)
    assert valid(2, 1e-4, 3, 4, [1.0, 0.5]) == ("ok", 1) and valid(64, 0.0, 1, 1, np.ones(64)) == ("ok", 1) and valid(1, INF, 1, 1, [0.0]) == ("ok", 1)
    assert valid(64, 1e-4, 1 << 15, 1 << 10, np.ones(64)) == ("ok", 0)      # 2^31
    assert valid(63, 1e-4, 1 << 15, 1 << 10, np.ones(63)) == ("ok", 1)
    assert valid(2, 1e-4, 0, 4, [1.0, 0.5])[1] == 0 and valid(2, 1e-4, 3, 0, [1.0, 0.5])[1] == 0
    assert valid(65, 1e-4, 1, 1, np.ones(65))[0] == "n_alpha outside 1 .. 64" and valid(0, 1e-4, 1, 1, [])[0] == "n_alpha outside 1 .. 64"
    assert valid(2, 1e-4, 1, 1, [1.0, NAN])[0] == "a non-finite alpha" and valid(2, 1e-4, 1, 1, [-INF, 1.0])[0] == "a non-finite alpha"
    assert valid(1, -0.5, 1, 1, [1.0])[0] == "armijo negative or not a number" and valid(1, NAN, 1, 1, [1.0])[0] == "armijo negative or not a number"


COST_REFUSED = {"null cost": dict(cost=None), "null q": dict(q=None), "null J": dict(J=None), "nq 0": dict(nq=0), "T 0": dict(T=0), "B 0": dict(B=0),
                "n_Q 2 with T 3": dict(n_Q=2), "n_R 0": dict(n_R=0), "n_x 2 with B 1": dict(n_x=2), "null Qf": dict(Qf=None)}


@pytest.mark.parametrize("what", sorted(COST_REFUSED))
def test_tracking_cost_refuses_invalid_arguments(what):
    nq, nu, T, B = 3, 2, 3, 1
    o = dict(nq=nq, T=T, B=B, cost=True, q=np.zeros((T + 2, B, nq)), J=np.zeros(B), n_Q=1, n_R=1, n_x=1, Qf=np.eye(2 * nq))
    o.update(COST_REFUSED[what])
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib._dp)
    Q, R, xg, ug, u = np.eye(2 * nq), np.eye(nu), np.zeros((T + 1, 1, 2 * nq)), np.zeros((T, 1, nu)), np.zeros((T, B, nu))
    cc = _lib.TrackingCost(dp(Q), dp(o["Qf"]), dp(R), dp(xg), dp(ug), o["n_Q"], o["n_R"], o["n_x"])
    rc = _lib.load().cimpc_plant_tracking_cost(o["nq"], nu, o["B"], o["T"], C.byref(cc) if o["cost"] else None, dp(o["q"]), dp(u), dp(o["J"]), None, None)
    assert rc == INVALID


def test_linesearch_refuses_gains_it_cannot_use():
    """`RolloutTape.linesearch` on gains without linear terms or with keep < T, before the library is called (no tape needed: the method's
    checks come first on an object that only carries the shapes)."""
    tape = object.__new__(plant.RolloutTape)
    tape.model, tape.B, tape.T, tape.n_cols, tape._N_sample, tape._feedback = "hopper_2D", 1, 3, 10, 1, None
    tape._finalizer = type("F", (), {"alive": True})()
    K, k, dV = np.zeros((3, 1, 2, 8)), np.zeros((3, 1, 2)), np.zeros((1, 2))
    cost = plant.TrackingCost(np.eye(8), np.eye(2))
    gains = lambda **kw: plant.TapeGains(**{**dict(K=K, k=k, P0=None, p0=None, dV=dV, status=np.zeros(1), n_cut=np.zeros(1)), **kw})
    args = (np.zeros((5, 1, 4)), np.zeros((3, 1, 2)), cost, np.zeros(1), (1.0,))
    for bad, why in ((gains(k=None), "k"), (gains(dV=None), "dV"), (gains(K=K[:2], k=k[:2]), "keep")):
        with pytest.raises(ValueError, match=why):
            tape.linesearch(bad, *args)
    with pytest.raises(ValueError, match="alphas"):
        tape.linesearch(gains(), *args[:4], ())
    with pytest.raises(ValueError, match="armijo"):
        tape.linesearch(gains(), *args, armijo=-1.0)


# ---- iLQR on the CPU plant ----------------------------------------------------------------------------------------------------------------------
def test_one_full_step_in_flight_lands_on_the_lq_optimum_on_the_cpu():
    """The gaps that fix the device test's bounds (10 x these): they are small, and the step is a real one."""
    gu, gj = plc.flight_gaps_cpu()
    print(f"flight on the CPU: controls {gu:.3e} from the LQ optimum, decrease {gj:.3e} from dV1 + dV2")
    assert 0.0 < gu < 1e-6 and 0.0 < gj < 1e-6
    case, Q, R, Qf, x_goal, u_goal = plc.flight_case()
    it = plc.ilqr_cpu(case, Q, R, Qf, x_goal, u_goal, (1.0,), 1)[0]
    assert it["accepted"].all() and (it["J_new"] < 0.9 * it["J_nom"]).all() and np.abs(it["q"][:, :, 2]).min() > 0.9      # never near the ground


def test_the_lq_optimum_is_the_backward_pass():
    """`lq_optimum_ld` (a KKT solve) against the policy of `lq_ld` rolled through the linear model: two routes to the same minimizer."""
    rng = np.random.default_rng(6)
    nq, nu, T, B, nr, n_cols = 3, 3, 5, 1, 7, 9
    D = rng.standard_normal((T, B, nr, n_cols)) / 3.0
    Q, R, Qf = prc.weights(rng, 2 * nq, nu)
    lq, lr = rng.standard_normal((T + 1, B, 2 * nq)), rng.standard_normal((T, B, nu))
    g = prc.lq_ld(D, np.ones((T, B), dtype=np.int32), nq, nu, Q, R, Qf, q=lq, r=lr)
    du, dx, value = plc.lq_optimum_ld(D, 0, nq, nu, Q, R, Qf, lq, lr)
    x = np.zeros(2 * nq, dtype=plc.LD)
    for t in range(T):
        u = g["k"][t, 0] - g["K"][t, 0] @ x
        assert np.abs(u - du[t]).max() <= 1e-15 * max(1.0, float(np.abs(du).max()))
        A, Bm = prc.dense_AB(D[t, 0], nq, nu, plc.LD)
        x = A @ x + Bm @ u
    assert abs(value - (g["dV"][0, 0] + g["dV"][0, 1])) <= 1e-15 * abs(value)


def test_the_cpu_restatement_accepts_the_first_iteration_through_contact():
    c = pgc.rollout_case("hopper_2D")
    Q, R, Qf, x_goal, u_goal = plc.contact_cost()
    it = plc.ilqr_cpu(c, Q, R, Qf, x_goal, u_goal, (1.0, 0.5, 0.25), 1, rho=1e-6)[0]
    assert it["accepted"].all() and (it["J_new"] < it["J_nom"]).all()
    for b in range(3):
        a = (1.0, 0.5, 0.25)[it["choice"][b]]
        assert it["J_new"][b] <= it["J_nom"][b] + 1e-4 * (a * it["dV"][b, 0] + a * a * it["dV"][b, 1])
