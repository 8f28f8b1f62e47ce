"""Closed-loop device rollouts under linear state feedback (`cimpc_plant_rollout_feedback`, `_grad_feedback`, `_tape_feedback`,
`cimpc_plant_tape_vjp_feedback`; `plant.Feedback`) without a device: the exports and their ctypes signatures, the validation that comes
before any device call, csrc/plant_feedback.h and the extended chain of csrc/plant_adjoint.h built with g++ and run by a team of one
against the restatements of tests/plant_feedback_cases.py - also under AddressSanitizer and UBSan, as a stand-alone program -, the
adjoint identity between the extended chain and an independent forward recursion, the host folds for K and x_ref, and the condition
on the test inputs: every step of every case converges on the CPU under the law."""
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
import plant_feedback_cases as pfc
import plant_gradient_cases as pgc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID, NO_DEVICE = -1, -2
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip,
         "const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts),
         "cimpc_plant_tape": C.c_void_p, "cimpc_plant_tape*": C.POINTER(C.c_void_p), "const cimpc_feedback*": C.POINTER(_lib.Feedback)}
TAIL = ["const cimpc_feedback*", "double*", "double*"]


# ---- exports and signatures ----------------------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,base", [("cimpc_plant_rollout_feedback", "cimpc_plant_rollout"), ("cimpc_plant_rollout_grad_feedback", "cimpc_plant_rollout_grad"),
                                       ("cimpc_plant_rollout_tape_feedback", "cimpc_plant_rollout_tape")])
def test_rollout_entries_extend_their_open_loop_prototypes(name, base):
    params = _prototype(name)
    assert params == _prototype(base) + TAIL
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), name)


def test_vjp_entry_extends_its_open_loop_prototype_and_the_struct_is_mirrored():
    params = _prototype("cimpc_plant_tape_vjp_feedback")
    assert params == _prototype("cimpc_plant_tape_vjp") + ["double*"]
    assert [CTYPE[p] for p in params] == _lib.SIGNATURES["cimpc_plant_tape_vjp_feedback"][1]
    body = re.search(r"typedef struct cimpc_feedback\s*\{(.*?)\}\s*cimpc_feedback\s*;", HDR, flags=re.S).group(1)
    fields = [n.strip() for stmt in body.split(";") if stmt.strip() for n in re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", " ".join(stmt.split())).split(",")]
    assert fields == [n for n, _ in _lib.Feedback._fields_] == ["K", "x_ref", "K_f", "n_f", "hold_f", "n_sample"]


# ---- validation: hopper_2D (nq 4, nu 2, nc 1, nb 2, nw 2) ------------------------------------------------------------------------------------
ORDER = ["model", "B", "T", "steps_per_launch", "n_terrain", "terrain", "q0", "q1", "u", "K_u", "n_u", "hold_u", "w", "K_w", "n_w", "hold_w",
         "mu", "n_mu", "h", "opts", "q", "gamma", "b", "status", "iters"]
GRAD = {"cimpc_plant_rollout_feedback": [], "cimpc_plant_rollout_grad_feedback": ["reg", "n_cols", "z", "dz", "grad_status"],
        "cimpc_plant_rollout_tape_feedback": ["reg", "n_cols", "z", "grad_status", "tape"]}


def _arg(k, v):
    if k in ("opts", "tape", "fb"):
        return None if v is None else C.byref(v)
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(_lib._ip if v.dtype == np.int32 else _lib._dp)
    return v


def _call(entry, fb_over=None, **over):
    """A closed-loop entry on a valid hopper_2D call with `over` laid on top, `fb_over` on the schedule: (return code, tape handle)."""
    mid = plant.model_dims("hopper_2D")[0]
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims("hopper_2D")
    B, T, K_f = 2, 3, 2
    handle = C.c_void_p(0xdead)
    f = dict(K=np.zeros((K_f, B, 2 * nq, nu)), x_ref=np.zeros((K_f, B, 2 * nq)), K_f=K_f, n_f=B, hold_f=2, n_sample=4.0)
    f.update(fb_over or {})
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib._dp)
    fb = _lib.Feedback(dp(f["K"]), dp(f["x_ref"]), f["K_f"], f["n_f"], f["hold_f"], f["n_sample"])
    a = dict(model=mid, B=B, T=T, steps_per_launch=0, n_terrain=0, terrain=None, q0=np.zeros((B, nq)), q1=np.zeros((B, nq)),
             u=np.zeros((2, B, nu)), K_u=2, n_u=B, hold_u=2, w=None, K_w=1, n_w=1, hold_w=1, mu=np.array([0.5, 0.6]), n_mu=B,
             h=0.01, opts=_lib.IpOpts(**dataclasses.asdict(plant.SIM_OPTS)), q=np.zeros((T + 2, B, nq)), gamma=np.zeros((T, B, nc)),
             b=np.zeros((T, B, nb)), status=np.zeros((T, B), dtype=np.int32), iters=np.zeros((T, B), dtype=np.int32),
             reg=1e-9, n_cols=2 * nq + nu, z=np.zeros((T, B, nz)), dz=np.zeros((T, B, 2 * nq + nu, nr)), grad_status=np.zeros((T, B), dtype=np.int32),
             tape=handle, fb=fb, u_applied=np.zeros((T, B, nu)), fb_err=np.zeros((T, B, 2 * nq)))
    a.update(over)
    order = ORDER + GRAD[entry] + ["fb", "u_applied", "fb_err"]
    return getattr(_lib.load(), entry)(*[_arg(k, a[k]) for k in order]), handle.value


def _with(shape, where, value):
    a = np.zeros(shape)
    a[where] = value
    return a


BAD = {
    "null fb": (None, dict(fb=None)), "null K": (dict(K=None), {}), "null x_ref": (dict(x_ref=None), {}),
    "null u_applied": (None, dict(u_applied=None)), "null fb_err": (None, dict(fb_err=None)),
    "K_f = 0": (dict(K_f=0), {}), "hold_f = 0": (dict(hold_f=0), {}), "n_f neither 1 nor B": (dict(n_f=3), {}),
    "n_sample = 0": (dict(n_sample=0.0), {}), "n_sample < 0": (dict(n_sample=-1.0), {}), "n_sample NaN": (dict(n_sample=float("nan")), {}),
    "n_sample inf": (dict(n_sample=float("inf")), {}),
    "NaN in K": (dict(K=_with((2, 2, 8, 2), (1, 1, 7, 1), float("nan"))), {}), "inf in x_ref": (dict(x_ref=_with((2, 2, 8), (1, 1, 7), float("inf"))), {}),
    # what the base calls validate
    "unknown model": (None, dict(model=9)), "T = 0": (None, dict(T=0)), "null q": (None, dict(q=None)), "n_u neither 1 nor B": (None, dict(n_u=3)),
    "h = 0": (None, dict(h=0.0)), "B = 0": (None, dict(B=0)),
}


@pytest.mark.parametrize("entry", sorted(GRAD))
@pytest.mark.parametrize("what", sorted(BAD))
def test_closed_loop_entries_refuse_invalid_arguments_without_a_device(entry, what):
    fb_over, over = BAD[what]
    rc, handle = _call(entry, fb_over, **over)
    assert rc == INVALID
    if entry.endswith("tape_feedback"):
        assert handle is None, "a refused call must leave *tape NULL"


@pytest.mark.parametrize("entry,over", [("cimpc_plant_rollout_grad_feedback", dict(n_cols=0)), ("cimpc_plant_rollout_grad_feedback", dict(dz=None)),
                                        ("cimpc_plant_rollout_tape_feedback", dict(n_cols=9)), ("cimpc_plant_rollout_tape_feedback", dict(tape=None))])
def test_gradient_entries_keep_their_base_validation(entry, over):
    assert _call(entry, None, **over)[0] == INVALID


def test_vjp_feedback_refuses_invalid_arguments_without_a_device():
    out = [np.zeros((2, 4)), np.zeros((2, 4)), np.zeros((3, 2, 2))]
    n_cut, gq, gx = np.zeros(2, dtype=np.int32), np.zeros((5, 2, 4)), np.zeros((3, 2, 8))
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib._dp)
    vjp = _lib.load().cimpc_plant_tape_vjp_feedback
    assert vjp(None, dp(gq), None, None, *[dp(a) for a in out], None, None, None, n_cut.ctypes.data_as(_lib._ip), dp(gx)) == INVALID
    stand_in = C.cast(C.create_string_buffer(1024), C.c_void_p)      # refused before the tape is looked at
    assert vjp(stand_in, None, None, None, *[dp(a) for a in out], None, None, None, n_cut.ctypes.data_as(_lib._ip), dp(gx)) == INVALID


def test_a_valid_call_needs_a_gfx950():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    for entry in sorted(GRAD):
        assert _call(entry) == (NO_DEVICE, None if entry.endswith("tape_feedback") else 0xdead)
    assert _call("cimpc_plant_rollout_feedback", dict(K=np.zeros((2, 1, 8, 2)), x_ref=np.zeros((2, 1, 8)), n_f=1, n_sample=1.0))[0] == NO_DEVICE


@pytest.mark.parametrize("K,x_ref,kw", [
    (np.zeros((3, 2, 7)), np.zeros((3, 8)), {}), (np.zeros((3, 2, 8)), np.zeros((3, 7)), {}), (np.zeros((3, 2, 8)), np.zeros((2, 8)), {}),
    (np.zeros((3, 3, 2, 8)), np.zeros((3, 3, 8)), {}), (np.zeros((3, 2, 2, 8)), np.zeros((3, 8)), {}), (np.zeros((2, 8)), np.zeros(8), {}),
    (np.zeros((0, 2, 8)), np.zeros((0, 8)), {}), (np.zeros((3, 2, 8)), np.zeros((3, 8)), dict(hold=0)),
    (np.zeros((3, 2, 8)), np.zeros((3, 8)), dict(n_sample=0.0)), (np.full((3, 2, 8), np.nan), np.zeros((3, 8)), {})])
def test_feedback_refuses_wrong_shapes(K, x_ref, kw):
    """hopper_2D, B = 2: K is (K_f, 2, 8) beside x_ref (K_f, 8), or (K_f, 2, 2, 8) beside (K_f, 2, 8); refused before the library is called."""
    for call in (plant.rollout, plant.rollout_tape):
        with pytest.raises(ValueError):
            call("hopper_2D", np.zeros((2, 4)), np.zeros((2, 4)), np.zeros((3, 2)), 0.01, 0.5, feedback=plant.Feedback(K, x_ref, **kw))


def test_feedback_arrays_are_laid_out_for_the_library():
    rng = np.random.default_rng(0)
    K, xr = rng.standard_normal((3, 2, 8)), rng.standard_normal((3, 8))
    Kc, xc, hold, ns, shared = plant._feedback_arrays("hopper_2D", plant.Feedback(K, xr, hold=2), 5, 4)
    assert Kc.shape == (3, 1, 8, 2) and xc.shape == (3, 1, 8) and (hold, ns, shared) == (2, 4.0, True) and Kc.flags.c_contiguous
    np.testing.assert_array_equal(Kc[:, 0].transpose(0, 2, 1), K / 4)      # column-major blocks of K / N_sample
    Kc, xc, hold, ns, shared = plant._feedback_arrays("hopper_2D", plant.Feedback(np.stack([K] * 5, 1), np.stack([xr] * 5, 1), n_sample=2.5), 5, 1)
    assert Kc.shape == (3, 5, 8, 2) and xc.shape == (3, 5, 8) and (hold, ns, shared) == (1, 2.5, False)


def test_gait_feedback_pairs_consecutive_reference_states():
    from contactimplicitmpc.jl_amd import gains
    rng = np.random.default_rng(1)
    q, K = rng.standard_normal((7, 4)), rng.standard_normal((5, 2, 8))
    fb = gains.gait_feedback(q, K, N_sample=3)
    assert fb.hold == 3 and fb.n_sample is None and fb.x_ref.shape == (5, 8)
    for k in range(5):
        np.testing.assert_array_equal(fb.x_ref[k], np.concatenate([q[k], q[k + 1]]))
    with pytest.raises(ValueError):
        gains.gait_feedback(q[:6], K)


# ---- the condition on the inputs of the device tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pfc.CASES)
def test_every_step_of_every_case_converges_on_the_cpu_under_the_law(which):
    st, _ = pfc.cpu_open_loop(which)
    assert st.all()
    for v in pfc.variants(which):
        st, q, ua = pfc.cpu_closed_loop(which, v)
        assert st.all(), (which, v)
        assert np.abs(ua - pfc.base_case(which)["u"]).max() > 1e-4, "the feedback moves the controls"


def test_the_cases_cover_the_schedules_the_issue_names():
    assert pfc.variants("hopper_2D") == ("shared", "per_robot", "held")
    fb = pfc.feedback("hopper_2D", "held")
    assert fb["K"].shape == (2, 3, 2, 8) and fb["hold"] == 2 and pfc.row_of(13, 2, 2) == 1 and pfc.base_case("hopper_2D")["T"] >= 5
    assert {pfc.feedback(w, v)["n_sample"] for w in pfc.CASES for v in pfc.variants(w)} == {1.0, 4.0}
    assert all(pfc.feedback(w, "shared")["K"].ndim == 3 and pfc.feedback(w, "per_robot")["K"].ndim == 4 for w in pfc.CASES)
    assert all(pfc.base_case(w)["T"] > pfc.STEPS_PER_LAUNCH or pfc.base_case(w)["T"] == 2 for w in pfc.CASES)


# ---- csrc/plant_feedback.h and the extended chain on the host --------------------------------------------------------------------------------
# (nq, nu, nw, nc, nb, n_cols, T, K_f, hold_f, shared, n_sample)
SHAPES = {"one step": (4, 2, 2, 1, 2, 10, 1, 1, 1, True, 1.0), "hopper, held rows": (4, 2, 2, 1, 2, 14, 5, 2, 2, False, 4.0),
          "wide": (18, 12, 20, 8, 32, 70, 3, 3, 1, True, 2.5)}
SRC = os.path.join(HERE, "native", "plant_feedback_check.cpp")


def _build(tmp_path_factory, name, *flags):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp(name) / "plant_feedback_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_build(tmp_path_factory):
    return _build(tmp_path_factory, "feedback", "-O1")


@pytest.fixture(scope="module")
def host_build_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "feedback_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _random_case(name, B=2, seed=0):
    nq, nu, nw, nc, nb, n_cols, T, K_f, hold, shared, ns = SHAPES[name]
    rng = np.random.default_rng([seed, nq, n_cols, T])
    D = rng.standard_normal((T, B, nq + nc + nb, n_cols))
    status = np.ones((T, B), dtype=np.int32)
    if T > 1:      # a cut step: an all-zero block with status 0
        D[1, 0] = 0.0
        status[1, 0] = 0
    cot = pac.random_cotangents(rng, T, B, nq, nc, nb)
    fb = dict(K=rng.standard_normal((K_f, nu, 2 * nq) if shared else (K_f, B, nu, 2 * nq)),
              x_ref=rng.standard_normal((K_f, 2 * nq) if shared else (K_f, B, 2 * nq)), hold=hold, n_sample=ns)
    q, ubar = rng.standard_normal((T + 2, B, nq)), rng.standard_normal((T, B, nu))
    return D, status, cot, fb, q, ubar


def _run_host(exe, name, D, status, cot, fb, q, ubar):
    nq, nu, nw, nc, nb, n_cols, T, K_f, hold, shared, ns = SHAPES[name]
    B = D.shape[1]
    hexes = lambda a: " ".join(float(x).hex() for x in np.asarray(a).ravel())
    Kc = fb["K"].swapaxes(-1, -2)      # column-major blocks
    text = [f"{B} {T} {nq} {nu} {nw} {nc} {nb} {n_cols} 1 1 1 {K_f} {1 if shared else B} {hold} {float(ns).hex()}",
            " ".join(str(int(s)) for s in status.ravel()), hexes(D.transpose(0, 1, 3, 2)), *[hexes(g) for g in cot], hexes(Kc), hexes(fb["x_ref"]),
            hexes(q), hexes(ubar)]
    res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.split("\n")
    val = lambda k: np.array([float.fromhex(v) for v in lines[k].split()])
    c_u, c_w, c_mu, c_h = pac.columns(nq, nu, nw)
    out = dict(g_q0=val(0).reshape(B, nq), g_q1=val(1).reshape(B, nq), u_step=val(2).reshape(T, B, nu),
               w_step=val(3).reshape(T, B, nw) if n_cols >= c_mu else None, g_mu=val(4) if n_cols > c_mu else None,
               g_h=val(5) if n_cols > c_h else None, xref_step=val(7).reshape(T, B, 2 * nq))
    return out, np.array([int(v) for v in lines[6].split()]), val(8).reshape(T, B, nu), val(9).reshape(T, B, 2 * nq)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_build_of_the_law_and_the_chain_is_the_definition(host_build, name):
    """The law and the extended chain bit for bit the float64 restatements in the stated order; the chain within
    100 x max(d(chain_np, chain_ld), 2.2e-16) of the longdouble restatement, the bound `plant_adjoint_cases.bounds` builds."""
    nq, nu, nw, nc, nb, n_cols, T, K_f, hold, shared, ns = SHAPES[name]
    D, status, cot, fb, q, ubar = _random_case(name)
    got, n_cut, ua, e = _run_host(host_build, name, D, status, cot, fb, q, ubar)
    want_u, want_e = pfc.law_on(q, ubar, fb)
    assert ua.tobytes() == want_u.tobytes() and e.tobytes() == want_e.tobytes()
    Ks, _ = pfc.per_step(fb, T, D.shape[1])
    ld, f64, bound = pfc.bounds(D, *cot, nq, nu, nw, Ks, ns)
    assert n_cut.tolist() == (status == 0).sum(axis=0).tolist()
    for k in pfc.OUTPUTS:
        assert (got[k] is None) == (ld[k] is None), k
        if ld[k] is None:
            continue
        d = pac.distance(got[k], ld[k])
        print(f"{name} {k}: host build {d:.2e} from chain_ld (bound {bound[k]:.2e})")
        assert got[k].tobytes() == np.ascontiguousarray(f64[k]).tobytes(), f"{k} differs from chain_f64"
        assert d <= bound[k]
    if T > 1:
        np.testing.assert_array_equal(got["xref_step"][1, 0], 0.0)      # the cut step
    # and the feedback path is there: the open-loop chain on the same blocks gives other λ
    open_loop = pac.chain_f64(D, *cot, nq, nu, nw)
    assert not np.array_equal(open_loop["g_q0"], got["g_q0"])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_build_runs_clean_under_the_sanitizers(host_build, host_build_sanitized, name):
    """The stand-alone program with -fsanitize=address,undefined: its workspace is exactly plant_adjoint_work_doubles +
    plant_adjoint_feedback_doubles, the kernel's LDS, so an index past gu or gx ends the run."""
    case = _random_case(name, seed=1)
    clean, plain = _run_host(host_build_sanitized, name, *case), _run_host(host_build, name, *case)
    for k in pfc.OUTPUTS:
        if plain[0][k] is not None:
            assert clean[0][k].tobytes() == plain[0][k].tobytes()
    for a, b in zip(clean[1:], plain[1:]):
        assert a.tobytes() == b.tobytes()


# ---- the restatements against each other ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_extended_chain_is_adjoint_to_the_forward_recursion(name):
    """⟨cotangents, forward_tangent(δ)⟩ = ⟨chain_ld(cotangents), δ⟩ to 1e-15 relative in longdouble on random blocks, δ in
    (q0, q1, ū, K, x_ref, μ): the gradient of K_t is gu_t ⊗ e_t, that of x_ref,t is gx_t."""
    nq, nu, nw, nc, nb, n_cols, T, K_f, hold, shared, ns = SHAPES[name]
    D, status, (gq, gg, gb), fb, q, ubar = _random_case(name, seed=2)
    B, L = D.shape[1], pfc.LD
    rng = np.random.default_rng(7)
    Ks, _ = pfc.per_step(fb, T, B)
    es = rng.standard_normal((T, B, 2 * nq))
    c_u, c_w, c_mu, c_h = pac.columns(nq, nu, nw)
    dq0, dq1, du = rng.standard_normal((B, nq)), rng.standard_normal((B, nq)), rng.standard_normal((T, B, nu))
    dK, dx = rng.standard_normal((T, B, nu, 2 * nq)), rng.standard_normal((T, B, 2 * nq))
    dmu = rng.standard_normal(B) if n_cols > c_mu else None
    dq, dgb = pfc.forward_tangent(D, dq0, dq1, du, nq, nu, nw, Ks, es, ns, dK=dK, dxref=dx, dmu=dmu)
    g = pfc.chain_ld(D, gq, gg, gb, nq, nu, nw, Ks, ns)
    lhs = (np.asarray(gq, L) * dq).sum() + (np.concatenate([gg, gb], axis=2).astype(L) * dgb).sum()
    gK = g["u_step"][..., :, None] * np.asarray(es, L)[..., None, :]
    rhs = (g["g_q0"] * dq0).sum() + (g["g_q1"] * dq1).sum() + (g["u_step"] * du).sum() + (gK * dK).sum() + (g["xref_step"] * dx).sum()
    if dmu is not None:
        rhs = rhs + (g["g_mu"] * dmu).sum()
    rel = float(abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    print(f"{name}: <g, J d> = {float(lhs):.6e}, <J' g, d> = {float(rhs):.6e}, relative difference {rel:.2e}")
    assert rel <= 1e-15


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per robot"])
@pytest.mark.parametrize("K_f,hold,T", [(3, 2, 6), (2, 2, 7), (1, 1, 4)])
def test_host_folds_for_the_gains_and_the_reference_states(K_f, hold, T, shared):
    """`plant.fold_gains` and `plant.fold_schedule` against element-by-element restatements; (2, 2, 7) holds its last row from step 2 on."""
    B, nu, n2 = 3, 2, 4
    rng = np.random.default_rng(K_f + 10 * T)
    gu, es, gx = rng.standard_normal((T, B, nu)), rng.standard_normal((T, B, n2)), rng.standard_normal((T, B, n2))
    np.testing.assert_array_equal(plant.fold_gains(gu, es, K_f, hold, shared, 4), pfc.fold_gains(gu, es, K_f, hold, shared, 4))
    np.testing.assert_array_equal(plant.fold_schedule(gx, K_f, hold, shared), pfc.fold_rows(gx, K_f, hold, shared))
    assert plant.fold_gains(gu, es, K_f, hold, shared).shape == ((K_f, nu, n2) if shared else (K_f, B, nu, n2))


# ---- the Julia binding ---------------------------------------------------------------------------------------------------------------------
JL_COMPAT = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*"},
             "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"}, "Ptr{Cvoid}": {"cimpc_plant_tape"},
             "Ref{Ptr{Cvoid}}": {"cimpc_plant_tape*"}, "Ref{Feedback}": {"const cimpc_feedback*"}}


@pytest.mark.parametrize("fn_name,symbol", [("plant_rollout_feedback", "cimpc_plant_rollout_feedback"),
                                            ("plant_rollout_tape_feedback", "cimpc_plant_rollout_tape_feedback"),
                                            ("plant_tape_vjp_feedback", "cimpc_plant_tape_vjp_feedback")])
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
    body = re.search(r"struct Feedback\n(.*?)\nend", JL, flags=re.S).group(1)
    assert [d.split("::")[0].strip() for line in body.split("\n") for d in line.split("#")[0].split(";") if "::" in d] == [n for n, _ in _lib.Feedback._fields_]
