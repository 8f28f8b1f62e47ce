"""The forward chain of a rollout (`cimpc_plant_tape_jvp`, `cimpc_plant_tape_jvp_feedback`, `RolloutTape.jvp`) without a device: the exports
and their ctypes signatures, argument validation (which comes before any device call), csrc/plant_tangent.h built with g++ and run by a
team of one on random synthetic tapes against the restatements of tests/plant_tangent_cases.py, the plan's group size over every row of
csrc/model_table.h, the spread helpers against the folds they transpose, the adjoint identity between `tangent_f64` and `chain_f64`, and
`tangent_ld` against the two forward recursions written earlier and independently (`plant_adjoint_cases.forward_tangent`,
`plant_feedback_cases.forward_tangent`).

Measured: the host build equals `tangent_f64` bit for bit at every shape and is at most 5.6e-16 from `tangent_ld` (bounds 2.2e-14 to
5.1e-14); `tangent_ld` equals both earlier recursions to 2.7e-19 relative (their own longdouble rounding: they sum with `@`; allowed
1.2e-17); the adjoint identity holds to 7.9e-17 and 2.2e-16 where the formula allows 4.1e-12 and 1.1e-13.  Run once by hand, not a
test: the host program built with -fsanitize=address,undefined, clean on every shape at groups of 1, 3 and the plan's."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, plant
import plant_adjoint_cases as pac
import plant_feedback_cases as pfc
import plant_tangent_cases as ptc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID = -1
CTYPE = {"int": C.c_int, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip, "cimpc_plant_tape": C.c_void_p}
SRC = os.path.join(HERE, "native", "plant_tangent_check.cpp")


# ---- exports, signatures and validation ----------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("cimpc_plant_tape_jvp", 12), ("cimpc_plant_tape_jvp_feedback", 14)])
def test_exports_are_declared_and_bound(name, n_args):
    params = _prototype(name)
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(params) == n_args
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), name)


def test_the_feedback_entry_extends_the_plain_one():
    assert _prototype("cimpc_plant_tape_jvp_feedback")[:12] == _prototype("cimpc_plant_tape_jvp")
    assert _prototype("cimpc_plant_tape_jvp_feedback")[12:] == ["const double*", "double*"]


@pytest.mark.parametrize("what", ["null tape", "n_dir = 0", "no input", "null dq", "null n_cut"])
def test_jvp_refuses_invalid_arguments_without_a_device(what):
    """Each is refused before the tape is looked at: any non-null pointer stands in for one."""
    stand_in = C.cast(C.create_string_buffer(1024), C.c_void_p)
    dq0, dq, n_cut = np.zeros((1, 2, 4)), np.zeros((1, 5, 2, 4)), np.zeros(2, dtype=np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib._dp)
    a = dict(tape=stand_in, n_dir=1, dq0=dq0, dq=dq, n_cut=n_cut)
    a.update({"null tape": dict(tape=None), "n_dir = 0": dict(n_dir=0), "no input": dict(dq0=None), "null dq": dict(dq=None),
              "null n_cut": dict(n_cut=None)}[what])
    cut = None if a["n_cut"] is None else a["n_cut"].ctypes.data_as(_lib._ip)
    lib = _lib.load()
    assert lib.cimpc_plant_tape_jvp(a["tape"], a["n_dir"], dp(a["dq0"]), None, None, None, None, None, dp(a["dq"]), None, None, cut) == INVALID
    assert lib.cimpc_plant_tape_jvp_feedback(a["tape"], a["n_dir"], dp(a["dq0"]), None, None, None, None, None, dp(a["dq"]), None, None, cut,
                                             None, None) == INVALID


# ---- csrc/plant_tangent.h on the host --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_chain(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("tangent") / "plant_tangent_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", exe, SRC])
    return exe


HOPPER, WALL = (4, 2, 2, 1, 2), (18, 12, 3, 8, 32)      # (nq, nu, nw, nc, nb): hopper_2D, nr 7; centroidal_quadruped_wall, nr 58
# name: (dims, n_cols, T, B, n_dir (None: the plan's group + 1), feedback (n_f, K_f, hold, n_sample) or None)
SHAPES = {
    "one step, least columns, one direction, one robot": (HOPPER, 10, 1, 1, 1, None),
    "every column, a cut step, a group and one more": (HOPPER, 14, 5, 3, None, None),
    "shared feedback, n_sample 1": (HOPPER, 14, 5, 3, 3, (1, 5, 1, 1.0)),
    "per-robot feedback held, n_sample 4, least columns": (HOPPER, 10, 7, 3, 2, (3, 2, 2, 4.0)),
    "per-robot feedback, a group and one more, one step": (HOPPER, 14, 1, 3, None, (3, 1, 1, 4.0)),
    "the largest block, feedback, a group and one more": (WALL, 53, 2, 1, None, (1, 2, 1, 1.0)),
}


def _case(name, seed=0):
    """(D, status, directions, loop for the restatements, K rows or None, n_dir) of a synthetic tape."""
    (nq, nu, nw, nc, nb), n_cols, T, B, n_dir, fb = SHAPES[name]
    nr = nq + nc + nb
    if n_dir is None:
        n_dir = _plan(nr, n_cols, nq, nu, fb is not None) + 1
    rng = np.random.default_rng([seed, sorted(SHAPES).index(name)])
    D = rng.standard_normal((T, B, nr, n_cols)) / np.sqrt(n_cols)
    status = np.ones((T, B), dtype=np.int32)
    if T >= 3:      # a cut step in the middle: an all-zero block with status 0, later δq restart from zero
        D[T // 2, 0] = 0.0
        status[T // 2, 0] = 0
    dirs = [ptc.random_direction(rng, T, B, nq, nu, nw, n_cols, closed=fb is not None) for _ in range(n_dir)]
    loop = K = None
    if fb is not None:
        n_f, K_f, hold, n_sample = fb
        K = 0.3 * rng.standard_normal((K_f, n_f, nu, 2 * nq))
        Ks = np.array([[K[ptc.row_of(t, hold, K_f), b if n_f == B else 0] for b in range(B)] for t in range(T)])
        loop = (Ks, n_sample)
    return D, status, dirs, loop, K


def _plan(nr, n_cols, nq, nu, feedback):
    per = n_cols + 3 * nq + (2 * nq if feedback else 0)
    room = 160 * 1024 // 8 - 2 * nr * n_cols
    return 0 if room < per else min(room // per, 64)


KEYS = ("dq0", "dq1", "du_step", "dw_step", "dmu", "dh", "dxref_step")


def _run_host(exe, name, D, status, dirs, K, group=0):
    (nq, nu, nw, nc, nb), n_cols, T, B, _, fb = SHAPES[name]
    n_dir = len(dirs)
    n_f, K_f, hold, n_sample = fb if fb is not None else (1, 0, 1, 1.0)
    hexes = lambda a: " ".join(float(x).hex() for x in np.asarray(a).ravel())
    has = [int(k in dirs[0]) for k in KEYS]
    text = [f"{B} {T} {nq} {nu} {nw} {nc} {nb} {n_cols} {n_dir} {group} {K_f} {n_f} {hold} {float(n_sample).hex()}", " ".join(map(str, has)),
            " ".join(str(int(s)) for s in status.ravel()), hexes(D.transpose(0, 1, 3, 2))]      # the library's blocks are column-major
    if K is not None:
        text.append(hexes(K.transpose(0, 1, 3, 2)))
    text += [hexes(np.stack([d[k] for d in dirs])) for k in KEYS if k in dirs[0]]
    res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.split("\n")
    vals = [np.array([float.fromhex(v) for v in line.split()]) for line in lines[:4]]
    out = dict(q=vals[0].reshape(n_dir, T + 2, B, nq), gamma=vals[1].reshape(n_dir, T, B, nc), b=vals[2].reshape(n_dir, T, B, nb),
               u_applied=vals[3].reshape(n_dir, T, B, nu) if fb is not None else None)
    return out, np.array([int(v) for v in lines[4].split()])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_build_of_the_kernels_statements_is_the_definition(host_chain, name):
    """Bit for bit `tangent_f64` in every direction, within 100 x max(d(tangent_np, tangent_ld), 2.2e-16) of `tangent_ld` relative to
    max|tangent_ld| (checked on the first and the last direction, the one that rides alone in the second group), and n_cut counts."""
    (nq, nu, nw, nc, nb), n_cols, T, B, _, fb = SHAPES[name]
    D, status, dirs, loop, K = _case(name)
    got, n_cut = _run_host(host_chain, name, D, status, dirs, K)
    assert n_cut.tolist() == (status == 0).sum(axis=0).tolist()
    f64 = ptc.stacked(ptc.tangent_f64, D, dirs, nq, nu, nw, nc, loop)
    for k in ptc.OUTPUTS:
        assert (got[k] is None) == (f64[k] is None) == (k == "u_applied" and fb is None), k
        if got[k] is not None:
            assert got[k].tobytes() == np.ascontiguousarray(f64[k]).tobytes(), f"{k} differs from tangent_f64"
    for d in sorted({0, len(dirs) - 1}):
        ld, _, bound = ptc.bounds(D, dirs[d], nq, nu, nw, nc, loop)
        for k in bound:
            dist = pac.distance(got[k][d], ld[k])
            print(f"{name}, direction {d}, {k}: host build {dist:.2e} from tangent_ld (bound {bound[k]:.2e})")
            assert dist <= bound[k]
    if T >= 3:      # behind the cut step the flow restarts from zero
        np.testing.assert_array_equal(got["q"][:, T // 2 + 2, 0], 0.0)
        assert np.abs(got["q"][:, T // 2 + 2, 1]).min() > 0


@pytest.mark.parametrize("name", ["every column, a cut step, a group and one more", "shared feedback, n_sample 1"])
def test_grouping_does_not_matter_on_the_host(host_chain, name):
    D, status, dirs, loop, K = _case(name, seed=1)
    dirs = dirs[:5]
    whole, _ = _run_host(host_chain, name, D, status, dirs, K)
    for group in (1, 2):
        parts, _ = _run_host(host_chain, name, D, status, dirs, K, group=group)
        for k in ptc.OUTPUTS:
            if whole[k] is not None:
                assert parts[k].tobytes() == whole[k].tobytes(), (k, group)
    alone, _ = _run_host(host_chain, name, D, status, dirs[-1:], K)
    assert alone["q"][0].tobytes() == whole["q"][-1].tobytes()


@pytest.mark.parametrize("name", ["every column, a cut step, a group and one more", "shared feedback, n_sample 1"])
def test_an_input_of_explicit_zeros_is_the_input_left_out(host_chain, name):
    (nq, nu, nw, nc, nb), n_cols, T, B, _, fb = SHAPES[name]
    D, status, dirs, loop, K = _case(name, seed=2)
    keep = ("dq1", "dmu")
    left_out = [{k: d[k] for k in keep} for d in dirs[:2]]
    zeros = [{k: d[k] if k in keep else np.zeros_like(d[k]) for k in d} for d in dirs[:2]]
    a, _ = _run_host(host_chain, name, D, status, left_out, K)
    b, _ = _run_host(host_chain, name, D, status, zeros, K)
    f64 = ptc.stacked(ptc.tangent_f64, D, left_out, nq, nu, nw, nc, loop)
    for k in ptc.OUTPUTS:
        if a[k] is not None:
            assert a[k].tobytes() == b[k].tobytes() == np.ascontiguousarray(f64[k]).tobytes(), k


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def _model_rows():
    text = open(os.path.join(ROOT, "contactimplicitmpc", "jl_amd", "csrc", "model_table.h")).read()
    rows = re.findall(r"X\((\w+), (\d+), (\d+), (\d+), (\d+), (\d+), \d\)", text)
    assert len(rows) >= 10
    return [(n, *map(int, v)) for n, *v in rows]


def test_the_plans_group_fits_a_cu_for_every_model(host_chain):
    """`plant_tangent_group` for every row of csrc/model_table.h, the least and every column, with and without feedback: at least one
    direction, within 160 KB, and the Python restatement `plant.tangent_group` and this file's agree with the header."""
    for name, nq, nu, nw, nc, nb in _model_rows():
        nr = nq + nc + nb
        for n_cols in (2 * nq + nu, 2 * nq + nu + nw + 2):
            for fb in (False, True):
                out = subprocess.run([host_chain, "plan", str(nr), str(n_cols), str(nq), str(nu), str(int(fb))], capture_output=True, text=True, check=True)
                g, lds, fits = (int(v) for v in out.stdout.split())
                assert 1 <= g <= 64 and lds <= 160 * 1024 and fits == 1, (name, n_cols, fb, g, lds)
                assert g == _plan(nr, n_cols, nq, nu, fb)
                assert lds == 8 * (2 * nr * n_cols + g * (n_cols + 3 * nq + (2 * nq if fb else 0)))
    for model in ("quadruped", "hopper_2D", "centroidal_quadruped_wall", "pushbot", "hopper_3D", "particle"):
        mid, nq, nu, nc, fd, nw = plant.model_dims(model)
        for fb in (False, True):
            assert plant.tangent_group(model, 2 * nq + nu + nw + 2, fb) == _plan(nq + nc + fd * nc, 2 * nq + nu + nw + 2, nq, nu, fb)


# ---- the spread helpers are the transposes of the folds --------------------------------------------------------------------------------------
def _inner(terms):
    """(Σ terms in float64 as NumPy sums them, Σ |terms| in longdouble): a sum of n terms in any order is within n ε Σ|terms| of the exact one."""
    t = np.asarray(terms, dtype=np.float64).ravel()
    return float(t.sum()), float(np.abs(t.astype(ptc.LD)).sum()), t.size


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per robot"])
@pytest.mark.parametrize("K,hold,T", [(3, 2, 6), (2, 2, 7), (1, 3, 4)])
def test_spread_schedule_is_the_transpose_of_fold_schedule(K, hold, T, shared):
    """⟨fold_schedule(g), δ⟩ = ⟨g, spread_schedule(δ)⟩, both with a scale of `hold`.  Each side is a sum of the same T B n products
    g δ / scale grouped differently, every partial result rounded: the two differ by at most 2 (N + 3) ε Σ|g δ / scale| with N = T B n
    terms (N roundings of a sum, one of the product, one of the division on each side, first order)."""
    B, n = 3, 2
    rng = np.random.default_rng(K + 10 * T)
    g, d = rng.standard_normal((T, B, n)), rng.standard_normal((K, n) if shared else (K, B, n))
    s = plant.spread_schedule(d, T, B, hold, hold)
    np.testing.assert_array_equal(s, ptc.spread_rows(d, T, B, hold, hold))
    lhs, _, _ = _inner(plant.fold_schedule(g, K, hold, shared, hold) * d)
    rhs, mag, N = _inner(g * s)
    assert abs(lhs - rhs) <= 2 * (N + 3) * 2.2e-16 * mag
    assert s.shape == (T, B, n)
    if (K, hold, T) == (2, 2, 7):      # the last row is held
        np.testing.assert_array_equal(s[6], s[2])


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per robot"])
@pytest.mark.parametrize("K,hold,T", [(3, 2, 6), (2, 2, 7)])
def test_spread_gains_is_the_transpose_of_fold_gains(K, hold, T, shared):
    """⟨fold_gains(g_u, e), δK⟩ = ⟨g_u, spread_gains(δK, e)⟩: sums of the same T B nu 2nq products g_u e δK / scale, held as above."""
    B, nu, n2, scale = 3, 2, 4, 2.0
    rng = np.random.default_rng(K + 10 * T)
    gu, e = rng.standard_normal((T, B, nu)), rng.standard_normal((T, B, n2))
    dK = rng.standard_normal((K, nu, n2) if shared else (K, B, nu, n2))
    s = plant.spread_gains(dK, e, hold, scale)
    np.testing.assert_array_equal(s, ptc.spread_gain_rows(dK, e, hold, scale))
    lhs, _, _ = _inner(plant.fold_gains(gu, e, K, hold, shared, scale) * dK)
    rhs, _, _ = _inner(gu * s)
    Ks = dK[[ptc.row_of(t, hold, K) for t in range(T)]]
    Ks = np.broadcast_to(Ks[:, None], (T, B, nu, n2)) if shared else Ks
    _, mag, N = _inner(gu[..., None] * e[:, :, None, :] * Ks / scale)
    assert abs(lhs - rhs) <= 2 * (N + 4) * 2.2e-16 * mag


# ---- the restatements against each other ---------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (np.asarray(a, ptc.LD) * np.asarray(b, ptc.LD)).sum()


@pytest.mark.parametrize("name", ["every column, a cut step, a group and one more", "one step, least columns, one direction, one robot"])
def test_forward_and_reverse_restatements_are_adjoint_in_float64(name):
    """⟨g, tangent_f64(δ)⟩ = ⟨chain_f64(g), δ⟩ on random blocks, held to the formula of test 3 of tests/test_gpu_plant_adjoint.py:
    Σ_k bound_k max|chain_ld_k| ‖δ_k‖₁ over the outputs k of the reverse chain that meet a direction δ_k."""
    (nq, nu, nw, nc, nb), n_cols, T, B, _, fb = SHAPES[name]
    D, status, dirs, loop, K = _case(name, seed=3)
    d = dirs[0]
    gq, gg, gb = pac.random_cotangents(np.random.default_rng(11), T, B, nq, nc, nb)
    tan = ptc.tangent_f64(D, d, nq, nu, nw, nc)
    ld, f64, bound = pac.bounds(D, gq, gg, gb, nq, nu, nw)
    pairs = [("g_q0", "dq0"), ("g_q1", "dq1"), ("u_step", "du_step"), ("w_step", "dw_step"), ("g_mu", "dmu"), ("g_h", "dh")]
    lhs = _dot(gq, tan["q"]) + _dot(gg, tan["gamma"]) + _dot(gb, tan["b"])
    rhs = sum(_dot(f64[k], d[v]) for k, v in pairs if v in d)
    tol = sum(bound[k] * float(np.abs(ld[k]).max()) * float(np.abs(d[v]).sum()) for k, v in pairs if v in d)
    print(f"{name}: <g, J d> = {float(lhs):.12e}, <J' g, d> = {float(rhs):.12e}, difference {float(abs(lhs - rhs)):.2e} (allowed {tol:.2e})")
    assert float(abs(lhs - rhs)) <= tol


def test_tangent_ld_is_the_two_forward_recursions_written_earlier():
    """`plant_adjoint_cases.forward_tangent` (open loop) and `plant_feedback_cases.forward_tangent` (closed loop, δu = δū − K δx + K δx_ref)
    were written independently of this chain; all three are longdouble and differ by the order of their sums alone."""
    name = "every column, a cut step, a group and one more"
    (nq, nu, nw, nc, nb), n_cols, T, B, _, fb = SHAPES[name]
    D, status, dirs, loop, K = _case(name)
    d = dirs[0]
    mine = ptc.tangent_ld(D, d, nq, nu, nw, nc)
    dq, dgb = pac.forward_tangent(D, d["dq0"], d["dq1"], d["du_step"], nq, nu, nw, d["dw_step"], d["dmu"], d["dh"])
    gaps = [pac.distance(mine["q"], dq), pac.distance(np.concatenate([mine["gamma"], mine["b"]], axis=2), dgb)]
    name = "shared feedback, n_sample 1"
    D, status, dirs, loop, K = _case(name)
    d = {k: v for k, v in dirs[0].items() if k not in ("dw_step", "dh")}      # the earlier closed-loop recursion has no δw, δh
    for n_sample in (1.0, 4.0):
        mine = ptc.tangent_ld(D, d, nq, nu, nw, nc, (loop[0], n_sample))
        dq, dgb = pfc.forward_tangent(D, d["dq0"], d["dq1"], d["du_step"], nq, nu, nw, loop[0], None, n_sample, dxref=d["dxref_step"], dmu=d["dmu"])
        gaps += [pac.distance(mine["q"], dq), pac.distance(np.concatenate([mine["gamma"], mine["b"]], axis=2), dgb)]
    # every output is a sum of at most n_cols + 2nq terms per step over T steps, regrouped: T (n_cols + 2nq) longdouble roundings
    allowed = T * (n_cols + 2 * nq) * float(np.finfo(ptc.LD).eps)
    print("tangent_ld against the earlier recursions:", " ".join(f"{g:.1e}" for g in gaps), f"(allowed {allowed:.1e})")
    assert max(gaps) <= allowed


# ---- the Julia binding ---------------------------------------------------------------------------------------------------------------------
JL_COMPAT = {"Cint": {"int"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*"}, "Ptr{Cvoid}": {"cimpc_plant_tape"}}


@pytest.mark.parametrize("fn_name,symbol", [("plant_tape_jvp", "cimpc_plant_tape_jvp"), ("plant_tape_jvp_feedback", "cimpc_plant_tape_jvp_feedback")])
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
