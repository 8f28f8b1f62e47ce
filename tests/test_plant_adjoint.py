"""The reverse chain of a rollout (`cimpc_plant_rollout_tape`, `cimpc_plant_tape_vjp`, `plant.rollout_tape`, `RolloutTape.vjp`) without a
device: the exports and their ctypes signatures, argument validation (which comes before any device call), csrc/plant_adjoint.h built
with g++ and run by a team of one against the restatements of tests/plant_adjoint_cases.py - also under AddressSanitizer and UBSan, as
a stand-alone program -, the adjoint identity between the reverse and the forward restatement, the fold of per-step control
gradients, and the chain over the longdouble step gradients of the hopper's flight against central differences of the CPU rollout.

Measured: the host build equals `chain_f64` bit for bit at the three shapes and is at most 1.8e-15 from `chain_ld` (bounds from
2.2e-14); the adjoint identity holds to 3.6e-19 and better; the flight finite differences differ from the chain by 2.8e-6 (robot 0)
and 3.1e-5 (robot 2) of the derivative."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, plant
import plant_adjoint_cases as pac
import plant_gradient_cases as pgc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID, NO_DEVICE = -1, -2
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip,
         "const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts),
         "cimpc_plant_tape": C.c_void_p, "cimpc_plant_tape*": C.POINTER(C.c_void_p)}


# ---- exports and signatures ----------------------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("cimpc_plant_rollout_tape", 30), ("cimpc_plant_tape_vjp", 11), ("cimpc_plant_tape_dims", 5),
                                         ("cimpc_plant_tape_destroy", 1)])
def test_exports_are_declared_and_bound(name, n_args):
    params = _prototype(name)
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(params) == n_args
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), name)


def test_rollout_tape_extends_the_rollout_prototype():
    assert _prototype("cimpc_plant_rollout_tape")[:25] == _prototype("cimpc_plant_rollout")
    assert _prototype("cimpc_plant_rollout_tape")[25:] == ["double", "int", "double*", "int*", "cimpc_plant_tape*"]
    assert re.search(r"typedef\s+struct\s+\w+\s*\*\s*cimpc_plant_tape\s*;", HDR)      # opaque, as cimpc_handle is


# ---- validation: hopper_2D (nq 4, nu 2, nc 1, nb 2, nw 2: nz 12, ntheta 14, nr 7) -----------------------------------------------------------
def _arg(k, v):
    if k == "opts":
        return None if v is None else C.byref(v)
    if k == "tape":
        return None if v is None else C.byref(v)
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(_lib._ip if v.dtype == np.int32 else _lib._dp)
    return v


def _terrains(*names):
    from contactimplicitmpc.jl_amd import terrain
    return (_lib.Terrain * len(names))(*[terrain.get(n).to_c() for n in names])


def _tape(**over):
    """cimpc_plant_rollout_tape on a valid hopper_2D call with `over` laid on top: (return code, the handle it left)."""
    mid = plant.model_dims("hopper_2D")[0]
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims("hopper_2D")
    B, T = 2, 3
    handle = C.c_void_p(0xdead)      # a failed call must leave NULL behind
    a = dict(model=mid, B=B, T=T, steps_per_launch=0, n_terrain=0, terrain=None, q0=np.zeros((B, nq)), q1=np.zeros((B, nq)),
             u=np.zeros((2, B, nu)), K_u=2, n_u=B, hold_u=2, w=None, K_w=1, n_w=1, hold_w=1, mu=np.array([0.5, 0.6]), n_mu=B,
             h=0.01, opts=_lib.IpOpts(**dataclasses.asdict(plant.SIM_OPTS)), q=np.zeros((T + 2, B, nq)), gamma=np.zeros((T, B, nc)),
             b=np.zeros((T, B, nb)), status=np.zeros((T, B), dtype=np.int32), iters=np.zeros((T, B), dtype=np.int32),
             reg=1e-9, n_cols=2 * nq + nu, z=np.zeros((T, B, nz)), grad_status=np.zeros((T, B), dtype=np.int32), tape=handle)
    a.update(over)
    order = ["model", "B", "T", "steps_per_launch", "n_terrain", "terrain", "q0", "q1", "u", "K_u", "n_u", "hold_u", "w", "K_w", "n_w", "hold_w",
             "mu", "n_mu", "h", "opts", "q", "gamma", "b", "status", "iters", "reg", "n_cols", "z", "grad_status", "tape"]
    return _lib.load().cimpc_plant_rollout_tape(*[_arg(k, a[k]) for k in order]), handle.value


BAD_TAPE = {
    "n_cols = 2 nq + nu - 1": dict(n_cols=9), "null tape": dict(tape=None),
    # the BAD_GRAD entries of tests/test_plant_gradients.py, re-stated (the tape has no dz argument)
    "n_cols = 0": dict(n_cols=0), "n_cols = ntheta + 1": dict(n_cols=15), "reg < 0": dict(reg=-1.0), "reg NaN": dict(reg=float("nan")),
    "null grad_status": dict(grad_status=None), "unknown model": dict(model=9),
    "terrain count neither 1 nor B": dict(n_terrain=3, terrain=_terrains("sine1_2D_lc", "sine1_2D_lc", "sine1_2D_lc")),
    "null q": dict(q=None), "T = 0": dict(T=0), "n_u neither 1 nor B": dict(n_u=3), "h = 0": dict(h=0.0),
}


@pytest.mark.parametrize("what", sorted(BAD_TAPE))
def test_rollout_tape_refuses_invalid_arguments_without_a_device(what):
    rc, handle = _tape(**BAD_TAPE[what])
    assert rc == INVALID
    if what != "null tape":
        assert handle is None, "a refused call must leave *tape NULL"


def _vjp(tape, gq, B=2, T=3):
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims("hopper_2D")
    out = [np.zeros((B, nq)), np.zeros((B, nq)), np.zeros((T, B, nu))]
    n_cut = np.zeros(B, dtype=np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib._dp)
    return _lib.load().cimpc_plant_tape_vjp(tape, dp(gq), None, None, *[dp(a) for a in out], None, None, None, n_cut.ctypes.data_as(_lib._ip))


@pytest.mark.parametrize("what", ["null tape", "no cotangent"])
def test_vjp_refuses_invalid_arguments_without_a_device(what):
    if what == "null tape":
        assert _vjp(None, np.zeros((5, 2, 4))) == INVALID
    else:      # refused before the tape is looked at: any non-null pointer stands in for one
        stand_in = C.create_string_buffer(1024)
        assert _vjp(C.cast(stand_in, C.c_void_p), None) == INVALID


def test_null_tape_is_refused_by_dims_and_ignored_by_destroy():
    lib = _lib.load()
    assert lib.cimpc_plant_tape_dims(None, None, None, None, None) == INVALID
    assert lib.cimpc_plant_tape_destroy(None) == 0


def test_a_valid_call_needs_a_gfx950():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    assert _tape() == (NO_DEVICE, None)
    assert _tape(z=None, n_cols=14, reg=0.0, steps_per_launch=1) == (NO_DEVICE, None)
    with pytest.raises(_lib.CimpcError):
        plant.rollout_tape("hopper_2D", np.zeros(4), np.zeros(4), np.zeros((2, 2)), 0.01, 0.5)


def test_python_checks_columns_before_the_library_is_called():
    for kw in (dict(grad_cols=9), dict(grad_cols=15), dict(grad_reg=-1.0)):
        with pytest.raises(ValueError):
            plant.rollout_tape("hopper_2D", np.zeros(4), np.zeros(4), np.zeros((2, 2)), 0.01, 0.5, **kw)


# ---- csrc/plant_adjoint.h on the host ------------------------------------------------------------------------------------------------------
# (nq, nu, nw, nc, nb, n_cols, T): one step of hopper_2D's nine blocks; every column of hopper_2D; nr = 58 with more columns than a wavefront
SHAPES = {(7, 10, 1): (4, 2, 2, 1, 2, 10, 1), (7, 14, 5): (4, 2, 2, 1, 2, 14, 5), (58, 70, 3): (18, 12, 20, 8, 32, 70, 3)}
SRC = os.path.join(HERE, "native", "plant_adjoint_check.cpp")


def _build(tmp_path_factory, name, *flags):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp(name) / "plant_adjoint_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_chain(tmp_path_factory):
    return _build(tmp_path_factory, "adjoint", "-O1")


@pytest.fixture(scope="module")
def host_chain_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "adjoint_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _random_case(shape, B=2, seed=0, cotangents=(True, True, True)):
    nq, nu, nw, nc, nb, n_cols, T = SHAPES[shape]
    rng = np.random.default_rng([seed, *shape])
    D = rng.standard_normal((T, B, nq + nc + nb, n_cols))
    status = np.ones((T, B), dtype=np.int32)
    if T > 1:      # a cut step: an all-zero block with status 0
        D[1, 0] = 0.0
        status[1, 0] = 0
    gq, gg, gb = [g if keep else None for g, keep in zip(pac.random_cotangents(rng, T, B, nq, nc, nb), cotangents)]
    return D, status, gq, gg, gb


def _run_host(exe, shape, D, status, gq, gg, gb):
    nq, nu, nw, nc, nb, n_cols, T = SHAPES[shape]
    B = D.shape[1]
    hexes = lambda a: " ".join(float(x).hex() for x in np.asarray(a).ravel())
    text = [f"{B} {T} {nq} {nu} {nw} {nc} {nb} {n_cols} {int(gq is not None)} {int(gg is not None)} {int(gb is not None)}",
            " ".join(str(int(s)) for s in status.ravel()), hexes(D.transpose(0, 1, 3, 2))]      # the library's blocks are column-major
    text += [hexes(g) for g in (gq, gg, gb) if g is not None]
    res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.split("\n")
    vals = [np.array([float.fromhex(v) for v in line.split()]) for line in lines[:6]]
    c_u, c_w, c_mu, c_h = pac.columns(nq, nu, nw)
    out = dict(g_q0=vals[0].reshape(B, nq), g_q1=vals[1].reshape(B, nq), u_step=vals[2].reshape(T, B, nu),
               w_step=vals[3].reshape(T, B, nw) if n_cols >= c_mu else None, g_mu=vals[4] if n_cols > c_mu else None,
               g_h=vals[5] if n_cols > c_h else None)
    return out, np.array([int(v) for v in lines[6].split()])


@pytest.mark.parametrize("cotangents", [(True, True, True), (True, False, False), (False, True, True)], ids=["all", "gq", "ggamma+gb"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_host_build_of_the_kernels_statements_is_the_definition(host_chain, shape, cotangents):
    """Bit for bit `chain_f64`, and within 100 x max(d(chain_np, chain_ld), 2.2e-16) of `chain_ld` relative to max|chain_ld|."""
    nq, nu, nw, nc, nb, n_cols, T = SHAPES[shape]
    D, status, gq, gg, gb = _random_case(shape, cotangents=cotangents)
    got, n_cut = _run_host(host_chain, shape, D, status, gq, gg, gb)
    ld, f64, bound = pac.bounds(D, gq, gg, gb, nq, nu, nw)
    assert n_cut.tolist() == (status == 0).sum(axis=0).tolist()
    for k in pac.OUTPUTS:
        assert (got[k] is None) == (ld[k] is None), k
        if ld[k] is None:
            continue
        d = pac.distance(got[k], ld[k])
        print(f"{shape} {k}: host build {d:.2e} from chain_ld (bound {bound[k]:.2e})")
        assert got[k].tobytes() == np.ascontiguousarray(f64[k]).tobytes(), f"{k} differs from chain_f64"
        assert d <= bound[k]
    assert (ld["g_h"] is not None) == (shape != (7, 10, 1))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_host_build_runs_clean_under_the_sanitizers(host_chain, host_chain_sanitized, shape):
    """The same stand-alone program with -fsanitize=address,undefined: its workspace is exactly plant_adjoint_work_doubles, the
    kernel's LDS, so an index past either block, `a` or the ring of λ ends the run."""
    case = _random_case(shape, seed=1)
    clean, cut = _run_host(host_chain_sanitized, shape, *case)
    plain, cut_plain = _run_host(host_chain, shape, *case)
    for k in pac.OUTPUTS:
        if plain[k] is not None:
            assert clean[k].tobytes() == plain[k].tobytes()
    assert cut.tolist() == cut_plain.tolist()


# ---- the restatements against each other ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_reverse_and_forward_restatements_are_adjoint(shape):
    """⟨cotangents, forward_tangent(δ)⟩ = ⟨chain_ld(cotangents), δ⟩ to 1e-15 relative, in longdouble, on random blocks."""
    nq, nu, nw, nc, nb, n_cols, T = SHAPES[shape]
    D, status, gq, gg, gb = _random_case(shape, seed=2)
    B = D.shape[1]
    rng = np.random.default_rng(7)
    c_u, c_w, c_mu, c_h = pac.columns(nq, nu, nw)
    dq0, dq1, du = rng.standard_normal((B, nq)), rng.standard_normal((B, nq)), rng.standard_normal((T, B, nu))
    dw = rng.standard_normal((T, B, nw)) if n_cols >= c_mu else None
    dmu = rng.standard_normal(B) if n_cols > c_mu else None
    dh = rng.standard_normal(B) if n_cols > c_h else None
    dq, dgb = pac.forward_tangent(D, dq0, dq1, du, nq, nu, nw, dw, dmu, dh)
    g = pac.chain_ld(D, gq, gg, gb, nq, nu, nw)
    L = pac.LD
    lhs = (np.asarray(gq, L) * dq).sum() + (np.concatenate([gg, gb], axis=2).astype(L) * dgb).sum()
    rhs = (g["g_q0"] * dq0).sum() + (g["g_q1"] * dq1).sum() + (g["u_step"] * du).sum()
    for name, d in (("w_step", dw), ("g_mu", dmu), ("g_h", dh)):
        if d is not None:
            rhs = rhs + (g[name] * d).sum()
    rel = float(abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    print(f"{shape}: <g, J d> = {float(lhs):.6e}, <J' g, d> = {float(rhs):.6e}, relative difference {rel:.2e}")
    assert rel <= 1e-15


CASES_FOLD = [(3, 2, 6), (2, 2, 7), (1, 1, 4)]


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per robot"])
@pytest.mark.parametrize("K,N_sample,T", CASES_FOLD)
def test_fold_of_the_control_gradients(K, N_sample, T, shared):
    """`fold_u` and the library's `plant.fold_schedule` against a brute-force loop over (t, b): (2, 2, 7) holds its last row for the
    steps past K N_sample."""
    B, nu = 3, 2
    g = np.random.default_rng(K + 10 * T).standard_normal((T, B, nu))
    want = np.zeros((K, nu) if shared else (K, B, nu))
    for t in range(T):
        for r in range(B):
            k = t // N_sample if t // N_sample < K else K - 1
            if shared:
                want[k] = want[k] + g[t, r]
            else:
                want[k, r] = want[k, r] + g[t, r]
    want = want / N_sample
    np.testing.assert_array_equal(pac.fold_u(g, K, N_sample, shared), want)
    np.testing.assert_array_equal(plant.fold_schedule(g, K, N_sample, shared, N_sample), want)
    if (K, N_sample, T) == (2, 2, 7):
        assert pac.schedule_row(6, N_sample, K) == 1 and pac.schedule_row(4, N_sample, K) == 1


# ---- the chain against finite differences of the CPU rollout, in flight --------------------------------------------------------------------
def _cpu_flight_rollout(c, P, r, q1, v1, u, T):
    """Robot r of the hopper case stepped T times by `cpu_step_z` from (q1, v1) under u (T, nu): (q (T + 2, nq), γ (T, nc), b (T, nb))."""
    from oracle import plant as pl
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(c["model"])
    q = [q1 - c["h"] * v1, q1.copy()]
    gam, bb = [], []
    for t in range(T):
        ok, z, th = pgc.cpu_step_z(P, q[t], q[t + 1], u[t], np.zeros(nw), c["mu"][r], c["h"], pl.SIM_OPTS)
        assert ok
        q.append(z[:nq].copy()); gam.append(z[nq:nq + nc].copy()); bb.append(z[nq + nc:nq + nc + nb].copy())
    return np.array(q), np.array(gam), np.array(bb)


@pytest.mark.parametrize("robot", [0, 2])
def test_chain_matches_finite_differences_of_the_cpu_rollout_in_flight(robot):
    """hopper_2D steps 0-3 (flight): `chain_ld` over the longdouble step gradients at the CPU rollout's z against central differences
    (ε = 1e-5) of that rollout, for a loss linear in (q, γ, b) with random weights and a random direction in (q1, v1, u).  Through
    the impact the regularized definition leaves the limit derivative, so the check stops before it."""
    T, eps = 4, 1e-5
    c = pgc.rollout_case("hopper_2D")
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims("hopper_2D")
    st, Z, TH = pgc.cpu_rollout("hopper_2D")
    refs = pgc.rollout_references(c, Z[:T, robot:robot + 1], TH[:T, robot:robot + 1], pgc.REG, 2 * nq + nu)
    D = np.array([[refs[t, 0]["ld"]] for t in range(T)])                      # (T, 1, nr, n_cols), longdouble
    rng = np.random.default_rng(100 + robot)
    gq, gg, gb = pac.random_cotangents(rng, T, 1, nq, nc, nb)
    dq1, dv1, du = rng.standard_normal(nq), rng.standard_normal(nq), rng.standard_normal((T, nu))
    g = pac.chain_ld(D, gq, gg, gb, nq, nu, nw)
    l0, l1 = g["g_q0"][0], g["g_q1"][0]
    adj = float(((l0 + l1) * dq1).sum() + (-c["h"] * l0 * dv1).sum() + (g["u_step"][:, 0] * du).sum())
    P = pgc.cpu_plant(c)

    def loss(s):
        q, gam, bb = _cpu_flight_rollout(c, P, robot, c["q1"][robot] + s * dq1, c["v1"][robot] + s * dv1, c["u"][:T, robot] + s * du, T)
        return float((gq[:, 0] * q).sum() + (gg[:, 0] * gam).sum() + (gb[:, 0] * bb).sum())
    fd = (loss(eps) - loss(-eps)) / (2 * eps)
    rel = abs(fd - adj) / max(abs(fd), abs(adj))
    print(f"robot {robot}: chain {adj:.9e}, central differences {fd:.9e}, relative difference {rel:.2e}")
    assert rel <= 1e-4


# ---- the Julia binding ---------------------------------------------------------------------------------------------------------------------
JL_COMPAT = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*"},
             "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"}, "Ptr{Cvoid}": {"cimpc_plant_tape"},
             "Ref{Ptr{Cvoid}}": {"cimpc_plant_tape*"}}


@pytest.mark.parametrize("fn_name,symbol", [("plant_rollout_tape", "cimpc_plant_rollout_tape"), ("plant_tape_vjp", "cimpc_plant_tape_vjp")])
def test_julia_calls_match_the_prototypes(fn_name, symbol):
    fn = JL[JL.index(f"function {fn_name}("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\." + symbol + r"\((.*?)\)::Cint", fn, flags=re.S)
    assert m, f"{fn_name} does not call {symbol}"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    params = _prototype(symbol)
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in JL_COMPAT[jt], f"argument {k}: Julia {jt} against C `{ct}`"
    assert "finalizer(" in JL[JL.index("mutable struct PlantTape"):JL.index("function plant_tape_vjp(")]
    assert "cimpc_plant_tape_destroy" in JL
