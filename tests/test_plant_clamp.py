"""The derivative of the clamped closed loop (`Feedback(..., clamp_grad=True)`) without a device: the rule
`plant_feedback_free` and the mask words at their edges (the host header, `plant.clamped_controls` and the restatement agree); the masked
chains of csrc/plant_adjoint.h and csrc/plant_tangent.h, built with g++ and run by a team of one, against the ordered float64
restatements of tests/plant_clamp_cases.py bit for bit and within the bounds of the longdouble ones; an all-free mask against the
unmasked restatements of tests/plant_feedback_cases.py and tests/plant_tangent_cases.py bit for bit; the two chains against each other
(duality); the same stand-alone program under AddressSanitizer and UBSan; the two exports, their ctypes signatures and Julia calls; the
refusals, which come before any device call.  tests/README_plant_clamp.md has the figures."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib
import plant_adjoint_cases as pac
import plant_clamp_cases as pcc
import plant_feedback_cases as pfc
import plant_tangent_cases as ptc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "plant_clamp_check.cpp")
HDR = open(os.path.join(ROOT, "include", "cimpc.h")).read()
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID = -1
INF, NAN = float("inf"), float("nan")


# ---- the host build ------------------------------------------------------------------------------------------------------------------------------
def _build(tmp, name, *flags):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("clamp"), "plant_clamp_check", "-O1")


hexes = lambda a: " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel())
ints = lambda a: " ".join(str(int(x)) for x in np.asarray(a).ravel())
cm = lambda M: np.swapaxes(np.asarray(M), -1, -2)      # the library's blocks are column-major


def _run(exe, mode, text, env=None):
    res = subprocess.run([exe, mode], input="\n".join(text) + "\n", capture_output=True, text=True, env=env)
    assert res.returncode == 0, (res.returncode, res.stderr[-3000:])
    return res.stdout.split("\n")


def _doubles(line, shape):
    return np.array([float.fromhex(v) for v in line.split()]).reshape(shape)


def _schedule(case):
    """(K rows as the library takes them (K_f, n_f, 2nq, nu), K_f, n_f) of a case's gains."""
    K = np.asarray(case["K"])
    K4 = K[:, None] if K.ndim == 3 else K
    return cm(K4), K4.shape[0], K4.shape[1]


def adjoint_text(case, mask=True):
    D, (gq, gg, gb) = case["D"], case["cots"]
    T, B, nr, n_cols = D.shape
    Kc, K_f, n_f = _schedule(case)
    text = [f"{B} {T} {case['nq']} {case['nu']} {case['nw']} {case['nc']} {case['nb']} {n_cols} 1 1 1 {K_f} {n_f} {case['hold']} "
            f"{float(case['n_sample']).hex()} {1 if mask else 0}", ints(case["status"]), hexes(cm(D)), hexes(gq), hexes(gg), hexes(gb), hexes(Kc)]
    if mask:
        text.append(ints(case["mask"]))
    return text


def run_adjoint(exe, case, mask=True, env=None):
    """The reverse chain of the host build on a case of `plant_clamp_cases.random_case` (or the same keys): dict of OUTPUTS + n_cut."""
    T, B, nr, n_cols = case["D"].shape
    nq, nu, nw = case["nq"], case["nu"], case["nw"]
    c_u, c_w, c_mu, c_h = pac.columns(nq, nu, nw)
    lines = _run(exe, "adjoint", adjoint_text(case, mask), env)
    out = dict(g_q0=_doubles(lines[0], (B, nq)), g_q1=_doubles(lines[1], (B, nq)), u_step=_doubles(lines[2], (T, B, nu)),
               w_step=_doubles(lines[3], (T, B, nw)) if n_cols >= c_mu else None, g_mu=_doubles(lines[4], (B,)) if n_cols > c_mu else None,
               g_h=_doubles(lines[5], (B,)) if n_cols > c_h else None, xref_step=_doubles(lines[7], (T, B, 2 * nq)))
    out["n_cut"] = [int(v) for v in lines[6].split()]
    return out


TANGENT_KEYS = ("dq0", "dq1", "du_step", "dw_step", "dmu", "dh", "dxref_step")


def run_tangent(exe, case, dirs, mask=True, group=0, env=None):
    """The forward chain of the host build on a list of directions: dict of TANGENT_OUTPUTS with a leading axis of n_dir, + n_cut."""
    D = case["D"]
    T, B, nr, n_cols = D.shape
    nq, nu, nw, nc, nb = case["nq"], case["nu"], case["nw"], case["nc"], case["nb"]
    Kc, K_f, n_f = _schedule(case)
    n_dir = len(dirs)
    has = [int(all(d.get(k) is not None for d in dirs)) for k in TANGENT_KEYS]
    text = [f"{B} {T} {nq} {nu} {nw} {nc} {nb} {n_cols} {n_dir} {group} {K_f} {n_f} {case['hold']} {float(case['n_sample']).hex()} "
            + " ".join(map(str, has)) + f" {1 if mask else 0}", ints(case["status"]), hexes(cm(D)), hexes(Kc)]
    if mask:
        text.append(ints(case["mask"]))
    for k, given in zip(TANGENT_KEYS, has):
        if given:
            text.append(hexes(np.stack([d[k] for d in dirs])))
    lines = _run(exe, "tangent", text, env)
    out = dict(q=_doubles(lines[0], (n_dir, T + 2, B, nq)), gamma=_doubles(lines[1], (n_dir, T, B, nc)), b=_doubles(lines[2], (n_dir, T, B, nb)),
               u_applied=_doubles(lines[3], (n_dir, T, B, nu)))
    out["n_cut"] = [int(v) for v in lines[4].split()]
    return out


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


# ---- 1. the rule at its edges ---------------------------------------------------------------------------------------------------------------------
# (u, lo, hi, free?)
EDGES = [(0.25, 0.25, 1.0, False),          # u == lo
         (1.0, 0.25, 1.0, False),           # u == hi
         (0.5, 0.25, 1.0, True),
         (0.5, 0.5, 0.5, False),            # lo == hi
         (0.5, -INF, INF, True),            # infinite bounds never clamp
         (1e300, -INF, INF, True),
         (-1e300, -INF, 0.0, True),
         (0.5, -INF, 0.5, False),           # one infinite bound, on the other
         (NAN, -1.0, 1.0, False),           # NaN is clamped
         (NAN, -INF, INF, False),
         (-0.0, 0.0, 1.0, False),           # a bound of 0.0 against u = -0.0: equal, so on the bound
         (0.0, -0.0, 1.0, False),
         (-0.0, -1.0, 0.0, False),
         (np.nextafter(0.25, 1.0), 0.25, 1.0, True),      # one ulp inside
         (np.nextafter(1.0, 0.0), 0.25, 1.0, True),
         (INF, -INF, INF, False),           # an infinite control sits on the infinite bound
         (5e-324, 0.0, 1.0, True)]          # the smallest subnormal is inside


def test_the_rule_at_its_edges(host):
    """`plant_feedback_free` of the header, its restatement and `plant.clamped_controls` on every edge the definition names."""
    from contactimplicitmpc.jl_amd import plant
    got = [int(v) for v in _run(host, "free", [str(len(EDGES)), " ".join(hexes(row[:3]) for row in EDGES)])[0].split()]
    for row, g in zip(EDGES, got):
        u, lo, hi, want = row
        assert bool(g) == want, row
        assert pcc.free(u, lo, hi) == want, row
        word = plant.clamped_controls(np.array([[[u]]]), [lo], [hi])
        assert word.dtype == np.int32 and word.tolist() == [[0 if want else 1]], row


def test_mask_words_at_nu_1_and_bit_11_at_nu_12(host):
    """The words of the header (as plant_clamp_mask_kernel forms them), of `plant.clamped_controls` and of the restatement are identical: nu = 1;
    nu = 12 with only control 11 clamped (bit 11 = 2048) and with every control clamped (4095); shared and per-robot limit rows."""
    from contactimplicitmpc.jl_amd import plant
    rng = np.random.default_rng(0)
    for nu, n_lim in ((1, 1), (1, 3), (2, 3), (12, 1), (12, 3)):
        T, B = 5, 3
        ua = rng.uniform(-1.0, 1.0, (T, B, nu))
        lo, hi = np.full((n_lim, nu), -0.5), np.full((n_lim, nu), 0.5)
        lo[:, 0], hi[-1, -1] = -INF, INF
        ua[0, 0, :] = 0.5                       # on the upper bound, where there is one
        ua[1, 1, -1] = NAN
        ua[2, :, :] = 0.0                       # everything free
        ua[3, :, :] = 0.0
        ua[3, :, nu - 1] = -0.5                 # only the last control, on its lower bound: bit nu - 1 alone
        words = [int(v) for v in _run(host, "words", [f"{T} {B} {nu} {n_lim}", hexes(ua), hexes(lo), hexes(hi)])[0].split()]
        want = pcc.clamped_words(ua, lo, hi)
        mine = plant.clamped_controls(ua, lo if n_lim > 1 else lo[0], hi if n_lim > 1 else hi[0])
        assert np.array(words).reshape(T, B).tolist() == want.tolist() == mine.tolist(), (nu, n_lim)
        assert want[2].tolist() == [0] * B
        # row 3: control 0 has no lower limit, so at nu = 1 nothing is clamped; otherwise the last control alone is, and its bit is nu - 1
        assert want[3].tolist() == [0 if nu == 1 else 1 << (nu - 1)] * B, (nu, n_lim, want[3].tolist())
    full = plant.clamped_controls(np.zeros((1, 1, 12)), np.zeros(12), np.zeros(12))
    assert full.tolist() == [[4095]] and full.dtype == np.int32
    with pytest.raises(ValueError):
        plant.clamped_controls(np.zeros((1, 1, 2)), None, None)
    with pytest.raises(ValueError, match="NaN"):
        plant.clamped_controls(np.zeros((1, 1, 2)), [NAN, 0.0], [1.0, 1.0])


# ---- 2. the headers against the restatements ------------------------------------------------------------------------------------------------------
# (shape, T, mask, hold, n_sample, shared schedule, every column of theta)
HOST_CASES = [(s, T, m, 1, 1.0, False, True) for s in ("hopper_2D", "pushbot", "walledcartpole") for T in (1, 2, 5) for m in pcc.MASKS]
HOST_CASES += [("centroidal_quadruped_wall", 1, "random", 1, 1.0, False, True), ("centroidal_quadruped_wall", 2, "free", 1, 1.0, False, False),
               ("centroidal_quadruped_wall", 2, "clamped", 1, 1.0, False, False), ("centroidal_quadruped_wall", 5, "random", 1, 1.0, False, False),
               ("hopper_2D", 5, "random", 2, 4.0, False, True), ("hopper_2D", 5, "random", 3, 0.5, True, False), ("walledcartpole", 5, "random", 2, 4.0, True, True)]
HOST_IDS = [f"{s}-T{T}-{m}-hold{h}-ns{ns:g}{'-shared' if sh else ''}{'' if full else '-nine'}" for s, T, m, h, ns, sh, full in HOST_CASES]


def _case(spec):
    s, T, m, hold, ns, shared, full = spec
    return pcc.random_case(s, T, m, hold=hold, n_sample=ns, shared=shared, full=full)


@pytest.mark.parametrize("spec", HOST_CASES, ids=HOST_IDS)
def test_host_chains_are_the_restatements_bit_for_bit_and_within_the_longdouble_bounds(host, spec):
    c = _case(spec)
    nq, nu, nw, nc = c["nq"], c["nu"], c["nw"], c["nc"]
    args = (nq, nu, nw, c["Ks"], c["n_sample"], c["mask"])
    ld, f64, bound = pcc.chain_bounds(c["D"], *c["cots"], *args)
    rev = run_adjoint(host, c)
    for k in pcc.OUTPUTS:
        if f64[k] is None:
            assert rev[k] is None
            continue
        assert same_bits(rev[k], f64[k]), f"reverse {k} differs from chain_f64"
        dist = pac.distance(rev[k], ld[k])
        print(f"reverse {k}: host {dist:.2e} from chain_ld (bound {bound[k]:.2e})")
        assert dist <= bound[k]
    assert rev["n_cut"] == [0] * c["D"].shape[1]
    fr = pcc.free_mask(c["mask"], nu)
    assert np.all(rev["u_step"][~fr] == 0.0) and not np.signbit(rev["u_step"][~fr]).any(), "a clamped control's cotangent is not exactly +0.0"
    # the forward chain: one direction, then a stack of three whose first is that one
    rng = np.random.default_rng(7)
    T, B, nr, n_cols = c["D"].shape
    dirs = [c["d"]] + [ptc.random_direction(rng, T, B, nq, nu, nw, n_cols, closed=True) for _ in range(2)]
    targs = (nq, nu, nw, nc, c["Ks"], c["n_sample"], c["mask"])
    tld, tf64, tbound = pcc.tangent_bounds(c["D"], c["d"], *targs)
    one = run_tangent(host, c, dirs[:1])
    three = run_tangent(host, c, dirs, group=2)      # two groups: a direction's bits do not depend on what rides with it
    want3 = pcc.stacked(pcc.tangent_f64, c["D"], dirs, *targs)
    for k in pcc.TANGENT_OUTPUTS:
        assert same_bits(one[k][0], tf64[k]), f"forward {k} differs from tangent_f64"
        assert same_bits(three[k], want3[k]) and same_bits(three[k][0], one[k][0]), f"forward {k}: the stack differs"
        dist = pac.distance(one[k][0], tld[k])
        print(f"forward {k}: host {dist:.2e} from tangent_ld (bound {tbound[k]:.2e})")
        assert dist <= tbound[k]
    assert np.all(one["u_applied"][0][~fr] == 0.0) and not np.signbit(one["u_applied"][0][~fr]).any()
    # duality of the two host chains, within the sum of the two longdouble bounds
    lhs, rhs, allowed = pcc.duality(c["cots"], {k: one[k][0] for k in pcc.TANGENT_OUTPUTS}, rev, c["d"], tld, tbound, ld, bound)
    print(f"<g, J d> = {float(lhs):.12e}, <J' g, d> = {float(rhs):.12e}, difference {float(abs(lhs - rhs)):.2e} (allowed {allowed:.2e})")
    assert float(abs(lhs - rhs)) <= allowed
    if spec[2] == "free":      # the unmasked restatements, and the closed-loop instantiation without a mask
        want = pfc.chain_f64(c["D"], *c["cots"], nq, nu, nw, c["Ks"], c["n_sample"])
        plain = run_adjoint(host, c, mask=False)
        for k in pcc.OUTPUTS:
            if want[k] is not None:
                assert same_bits(rev[k], want[k]) and same_bits(plain[k], want[k]), f"all free: reverse {k} differs from plant_feedback_cases.chain_f64"
        twant = ptc.tangent_f64(c["D"], c["d"], nq, nu, nw, nc, loop=(c["Ks"], c["n_sample"]))
        tplain = run_tangent(host, c, dirs[:1], mask=False)
        for k in pcc.TANGENT_OUTPUTS:
            assert same_bits(one[k][0], twant[k]) and same_bits(tplain[k][0], twant[k]), f"all free: forward {k} differs from plant_tangent_cases.tangent_f64"
    if spec[2] == "clamped":   # nothing reaches the gains, the reference or the open-loop controls
        assert np.all(rev["u_step"] == 0.0) and np.all(rev["xref_step"] == 0.0) and np.all(one["u_applied"] == 0.0)
        open_loop = pac.chain_f64(c["D"], *c["cots"], nq, nu, nw)
        assert same_bits(rev["g_q0"], open_loop["g_q0"]) and same_bits(rev["g_q1"], open_loop["g_q1"]), "all clamped: not the open-loop chain's λ"


def test_a_cut_step_is_counted_on_a_masked_chain(host):
    c = pcc.random_case("hopper_2D", 5, "random")
    c["status"] = c["status"].copy()
    c["status"][2, 1] = 0
    assert run_adjoint(host, c)["n_cut"] == [0, 1] and run_tangent(host, c, [c["d"]])["n_cut"] == [0, 1]


# ---- 3. the sanitizers, on the host only ---------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The program is built once with -fsanitize=address,undefined and run directly - no Python in the process, nothing preloaded - on one
    case with a random mask, hold 2, the largest model's sizes for the work buffer's ends; its answers are the restatements' bits."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "plant_clamp_check_san")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, SRC], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr[-300:])
    env = None
    c = pcc.random_case("centroidal_quadruped_wall", 2, "random", hold=2, n_sample=4.0)
    rev = run_adjoint(exe, c, env=env)
    f64 = pcc.chain_f64(c["D"], *c["cots"], c["nq"], c["nu"], c["nw"], c["Ks"], c["n_sample"], c["mask"])
    assert all(same_bits(rev[k], f64[k]) for k in pcc.OUTPUTS)
    fwd = run_tangent(exe, c, [c["d"]], env=env)
    tf64 = pcc.tangent_f64(c["D"], c["d"], c["nq"], c["nu"], c["nw"], c["nc"], c["Ks"], c["n_sample"], c["mask"])
    assert all(same_bits(fwd[k][0], tf64[k]) for k in pcc.TANGENT_OUTPUTS)
    ua = np.zeros((2, 2, 12))
    words = _run(exe, "words", ["2 2 12 1", hexes(ua), hexes(np.zeros(12)), hexes(np.ones(12))], env=env)[0].split()
    assert [int(w) for w in words] == [4095] * 4


# ---- 4. the exports, their signatures, their Julia calls -------------------------------------------------------------------------------------------
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip, "cimpc_plant_tape": C.c_void_p,
         "const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts), "const cimpc_feedback*": C.POINTER(_lib.Feedback),
         "cimpc_plant_tape*": C.POINTER(C.c_void_p)}
JL_COMPAT = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*"}, "Ptr{Cvoid}": {"cimpc_plant_tape"},
             "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"}, "Ref{Feedback}": {"const cimpc_feedback*"},
             "Ref{Ptr{Cvoid}}": {"cimpc_plant_tape*"}}
# name -> (the sibling it extends, the Julia function, the parameters behind the sibling's)
ENTRIES = {"cimpc_plant_rollout_tape_feedback_limits": ("cimpc_plant_rollout_tape_feedback", "plant_rollout_tape_feedback_limits", ["int", "const double*", "const double*", "int*"]),
           "cimpc_plant_rollout_grad_feedback_limits": ("cimpc_plant_rollout_grad_feedback", "plant_rollout_grad_feedback_limits", ["int", "const double*", "const double*"])}


def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_two_exports_extend_their_siblings(name):
    """Declared in include/cimpc.h as the sibling's parameters plus (n_lim, u_lo, u_hi[, clamped]), exported, bound with matching ctypes, called
    from Julia with matching types."""
    sibling, jl_name, more = ENTRIES[name]
    params = _prototype(name)
    assert params == _prototype(sibling) + more
    assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args == [CTYPE[p] for p in params] and args[:-len(more)] == _lib.SIGNATURES[sibling][1]
    assert hasattr(_lib.load(), name)
    assert f"function {jl_name}(" in JL, f"julia/CIMPCHip.jl has no {jl_name}"
    fn = JL[JL.index(f"function {jl_name}("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint", fn, flags=re.S)
    assert m, f"{jl_name} does not call {name}"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in JL_COMPAT[jt], f"argument {k}: Julia {jt} against C `{ct}`"


# ---- 5. the refusals, before any device is touched ---------------------------------------------------------------------------------------------------
LIMIT_REFUSALS = {"u_lo above u_hi": (dict(u_lo=0.5, u_hi=0.25), "u_lo above u_hi"), "a NaN limit": (dict(u_lo=NAN), "a NaN limit"),
                  "n_lim = 3": (dict(n_lim=3), "n_lim neither 1 nor B"), "null u_hi": (dict(u_hi=None), "a null u_lo or u_hi"),
                  "null u_lo": (dict(u_lo=None), "a null u_lo or u_hi"), "an unknown model": (dict(model=999), "a model without controls")}


def _call(entry, a):
    lim = lambda v: None if v is None else np.full((1, 16), v)      # more than any model's nu: the limits' scan stays inside the arrays
    lo, hi = lim(a["u_lo"]), lim(a["u_hi"])
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib._dp)
    clamped = np.zeros((3, 2), dtype=np.int32)
    lib = _lib.load()
    base = (a["model"], 2, 3, 0, 0, None, None, None, None, 1, 1, 1, None, 1, 1, 1, None, 1, 0.01, None, None, None, None, None, None)
    if entry == "cimpc_plant_rollout_tape_feedback_limits":
        handle = C.c_void_p(1)
        rc = lib.cimpc_plant_rollout_tape_feedback_limits(*base, 1e-9, 10, None, None, C.byref(handle), None, None, None, a["n_lim"], dp(lo), dp(hi),
                                                          clamped.ctypes.data_as(_lib._ip) if a.get("clamped", True) else None)
        assert handle.value is None, "a refused call left a tape behind"
    else:
        rc = lib.cimpc_plant_rollout_grad_feedback_limits(*base, 1e-9, 10, None, None, None, None, None, None, a["n_lim"], dp(lo), dp(hi))
    return rc, lib.cimpc_last_error(None).decode()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("what", sorted(LIMIT_REFUSALS))
def test_the_entries_refuse_the_limits_by_reason_without_a_device(entry, what):
    """What `cimpc_plant_rollout_feedback_limits` refuses of the limits, by the same reasons, under each entry's own name."""
    from contactimplicitmpc.jl_amd import plant
    change, reason = LIMIT_REFUSALS[what]
    a = dict(model=plant.model_dims("hopper_2D")[0], n_lim=1, u_lo=-1.0, u_hi=1.0)
    a.update(change)
    rc, why = _call(entry, a)
    assert rc == INVALID and why == f"{entry}: {reason}"


def test_the_tape_entry_refuses_limits_with_a_null_clamped_and_then_what_its_sibling_refuses():
    from contactimplicitmpc.jl_amd import plant
    good = dict(model=plant.model_dims("hopper_2D")[0], n_lim=1, u_lo=-1.0, u_hi=1.0)
    rc, why = _call("cimpc_plant_rollout_tape_feedback_limits", dict(good, clamped=False))
    assert rc == INVALID and why == "cimpc_plant_rollout_tape_feedback_limits: limits on a tape without clamped"
    # good limits and nothing else: the rollout's own check (no device either) refuses the rest
    rc, why = _call("cimpc_plant_rollout_tape_feedback_limits", good)
    assert rc == INVALID and why == "cimpc_plant_rollout_tape_feedback_limits: an argument that cimpc_plant_rollout_tape_feedback refuses"
    rc, why = _call("cimpc_plant_rollout_grad_feedback_limits", good)
    assert rc == INVALID and why == "cimpc_plant_rollout_grad_feedback_limits: an argument that cimpc_plant_rollout_grad_feedback refuses"


def test_python_takes_clamp_grad_only_as_a_bool_and_only_with_limits():
    from contactimplicitmpc.jl_amd import plant
    nq, nu, B, T = 4, 2, 3, 5
    K, x_ref = np.zeros((T, nu, 2 * nq)), np.zeros((T, 2 * nq))
    args = ("hopper_2D", np.zeros((B, nq)), np.zeros((B, nq)), np.zeros((T, nu)), 0.01, 0.5)
    assert plant.Feedback(K, x_ref).clamp_grad is False
    for call, kw in ((plant.rollout, dict(diff_sol=True)), (plant.rollout, {}), (plant.rollout_tape, {})):
        with pytest.raises(ValueError, match="clamp_grad=True needs control limits"):
            call(*args, feedback=plant.Feedback(K, x_ref, clamp_grad=True), **kw)
        for bad in (1, 0, "yes", None, 1.0):
            with pytest.raises(ValueError, match="clamp_grad must be a bool"):
                call(*args, feedback=plant.Feedback(K, x_ref, u_lo=[-1.0, -1.0], u_hi=[1.0, 1.0], clamp_grad=bad), **kw)


def test_the_default_still_refuses_limits_and_now_names_the_switch():
    from contactimplicitmpc.jl_amd import plant
    nq, nu, B, T = 4, 2, 3, 5
    K, x_ref = np.zeros((T, nu, 2 * nq)), np.zeros((T, 2 * nq))
    args = ("hopper_2D", np.zeros((B, nq)), np.zeros((B, nq)), np.zeros((T, nu)), 0.01, 0.5)
    limited = plant.Feedback(K, x_ref, u_lo=[-1.0, -np.inf], u_hi=[1.0, np.inf])
    for call, kw in ((plant.rollout, dict(diff_sol=True)), (plant.rollout_tape, {})):
        with pytest.raises(ValueError, match="derivative of the clamp") as info:
            call(*args, feedback=limited, **kw)
        assert "clamp_grad=True" in str(info.value)


def test_tape_gains_pass_the_limits_and_the_switch_to_their_feedback():
    from contactimplicitmpc.jl_amd import plant
    keep, B, nu, nq = 3, 2, 2, 4
    g = plant.TapeGains(K=np.ones((keep, B, nu, 2 * nq)), k=None, P0=np.zeros((B, 2 * nq, 2 * nq)), p0=None, dV=None, status=np.zeros(B), n_cut=np.zeros(B))
    q = np.random.default_rng(0).standard_normal((keep + 2, B, nq))
    plain, lim = g.feedback(q), g.feedback(q, u_lo=[-1.0, -2.0], u_hi=[1.0, 2.0], clamp_grad=True)
    assert plain.u_lo is None and plain.u_hi is None and plain.clamp_grad is False
    assert lim.u_lo == [-1.0, -2.0] and lim.u_hi == [1.0, 2.0] and lim.clamp_grad is True
    assert np.array_equal(lim.K, plain.K) and np.array_equal(lim.x_ref, plain.x_ref)
