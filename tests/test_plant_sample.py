"""The sampling policy (`cimpc_plant_sampler`, `plant.SamplingPolicy`) without a device: csrc/plant_sample.h
built with g++ against the NumPy restatements of `plant_sample_cases` exactly - Philox4x32-10 on its known answers, the deviate on a few
thousand counters with the edge words, its moments, the candidate law, eligibility, choice and both updates -; the same program under
AddressSanitizer and UBSan; `cimpc_plant_sample_noise` against the same restatement; every refusal that needs no device, each by its reason;
the exports, their ctypes signatures and their Julia calls, by text; and the Python class's own refusals before the library is called.
tests/README_plant_sample.md has the rest."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib
import plant_sample_cases as psc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "plant_sample_check.cpp")
INVALID = -1
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
NAMES = {"cimpc_plant_sampler_create": 30, "cimpc_plant_sampler_control": 14, "cimpc_plant_sampler_plan": 7, "cimpc_plant_sampler_raw_weights": 2,
         "cimpc_plant_sampler_reset": 2, "cimpc_plant_sampler_dims": 8, "cimpc_plant_sampler_destroy": 1, "cimpc_plant_sample_noise": 7}
JL_FUNCS = {name: name[len("cimpc_"):] for name in NAMES}
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip, "const int*": _lib._ip,
         "cimpc_plant_sampler": C.c_void_p, "const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts),
         "cimpc_plant_sampler*": C.POINTER(C.c_void_p), "unsigned long long": C.c_ulonglong, "unsigned int": C.c_uint}
JL_COMPAT = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*", "const int*"},
             "Ptr{Cvoid}": {"cimpc_plant_sampler"}, "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"},
             "Ref{Ptr{Cvoid}}": {"cimpc_plant_sampler*"}, "Ref{Cint}": {"int*"}, "Culonglong": {"unsigned long long"}, "Cuint": {"unsigned int"}}
hx = lambda x: float(x).hex()
nan, inf = float("nan"), float("inf")


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: {a.shape} against {b.shape}"
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{what} differs"
    if a.dtype.kind == "f":
        assert np.array_equal(np.signbit(a), np.signbit(b)), f"{what}: a sign of zero differs"


# ---- the header --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("sample") / "plant_sample_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", exe, SRC])
    return exe


def run(exe, mode, text):
    res = subprocess.run([exe, mode], input=text + "\n", capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    return res.stdout.strip().split("\n")


def doubles(line):
    return np.array([float.fromhex(v) for v in line.split()])


def ints(line):
    return np.array([int(v) for v in line.split()])


def check_philox(exe):
    text = f"{len(psc.KNOWN)} " + " ".join(" ".join(str(v) for v in ctr + key) for ctr, key, _ in psc.KNOWN)
    lines = run(exe, "philox", text)
    for (ctr, key, out), line in zip(psc.KNOWN, lines):
        assert [int(v, 16) for v in line.split()] == list(out), (ctr, key)
        assert [int(v) for v in psc.philox(*ctr, *key)] == list(out), "the NumPy restatement misses a known answer"


def counters(seed, n):
    """n random (seed, draw, b, c, e) and every combination of 0 and 0xffffffff in the counter words, under seeds 0, 2^32 - 1, above 2^32, 2^64 - 1."""
    rng = np.random.default_rng(seed)
    rows = [(int(s), int(d), int(b), int(c), int(e)) for s, d, b, c, e in zip(rng.integers(0, 2 ** 64, n, dtype=np.uint64), rng.integers(0, 2 ** 32, n),
                                                                                rng.integers(0, 2 ** 32, n), rng.integers(0, 2 ** 32, n), rng.integers(0, 2 ** 32, n))]
    edge = (0, 0xffffffff)
    for s in (0, 0xffffffff, (5 << 32) + 7, 2 ** 64 - 1):
        rows += [(s, d, b, c, e) for d in edge for b in edge for c in edge for e in edge]
    return rows


def check_deviate(exe, seed, n):
    rows = counters(seed, n)
    got = doubles(run(exe, "eps", f"{len(rows)} " + " ".join(" ".join(str(v) for v in r) for r in rows))[0])
    cols = [np.array(col, dtype=np.uint64) for col in zip(*rows)]
    _same(got, psc.eps(*cols), "the deviate")
    assert np.abs(got).max() <= 4.0 * math.sqrt(1.5)
    triples = ((0, 1, 0), (3, 2, 1), (2 ** 31 - 1, 2 ** 31 - 1, 5), (2 ** 31 - 1, 2, 1), (7, 3, 2))
    lines = run(exe, "draw", f"{len(triples)} " + " ".join(f"{s} {n} {i}" for s, n, i in triples))
    assert [int(v) for v in lines] == [psc.draw_of(*t) for t in triples]
    pairs = ((14, 3), (14, 1), (1, 1), (5, 5), (5, 7), (6, 2 ** 31 - 1), (2 ** 31 - 1, 1))
    lines = run(exe, "rows", f"{len(pairs)} " + " ".join(f"{H} {k}" for H, k in pairs))
    assert [int(v) for v in lines] == [psc.noise_rows(*p) for p in pairs]


def test_philox_meets_its_known_answers(host):
    check_philox(host)


def test_the_deviate_of_the_header_is_the_numpy_restatement_exactly(host):
    check_deviate(host, 11, 4000)


def test_the_moments_and_the_support_of_the_deviate():
    """65 536 consecutive e: |mean| < 0.02 and |variance - 1| < 0.03, five standard errors (1/256 for the mean, sqrt(1.85 / 65536) for the
    variance with excess kurtosis -0.15), and |eps| <= 4 sqrt(1.5) for every draw."""
    for seed, draw, b, c in ((0, 0, 0, 1), ((9 << 32) + 1, 77, 3, 2)):
        e = psc.eps(seed, draw, b, c, np.arange(65536))
        assert abs(e.mean()) < 0.02 and abs(e.var() - 1.0) < 0.03, (e.mean(), e.var())
        assert np.abs(e).max() <= 4.0 * math.sqrt(1.5)
        kurt = ((e - e.mean()) ** 4).mean() / e.var() ** 2 - 3.0
        print(f"seed {seed} draw {draw}: mean {e.mean():.5f} variance {e.var():.5f} excess kurtosis {kurt:.4f} max |eps| {np.abs(e).max():.4f}")


def test_the_host_entry_gives_the_restated_noise_and_rows_do_not_depend_on_B_or_N():
    from contactimplicitmpc.jl_amd import plant
    seed, draw = (3 << 32) + 12345, 0xfffffffe
    big = plant.sampling_noise(seed, draw, 5, 7, 4, 3)
    _same(big, psc.noise(seed, draw, 5, 7, 4, 3), "cimpc_plant_sample_noise")
    small = plant.sampling_noise(seed, draw, 2, 3, 4, 3)
    _same(small, big[:, :3, :2], "the rows of the robots and samples that remain")
    assert not np.array_equal(plant.sampling_noise(seed + 1, draw, 2, 3, 4, 3), small) and not np.array_equal(plant.sampling_noise(seed, draw + 1, 2, 3, 4, 3), small)
    for bad in (dict(B=0), dict(N=0), dict(n_rows=0), dict(nu=0), dict(seed=-1), dict(seed=2 ** 64), dict(draw=2 ** 32)):
        with pytest.raises(ValueError):
            plant.sampling_noise(**dict(dict(seed=1, draw=0, B=1, N=1, n_rows=1, nu=1), **bad))
    assert _lib.load().cimpc_plant_sample_noise(1, 0, 1, 1, 1, 1, None) == INVALID
    assert _lib.load().cimpc_last_error(None).decode() == "cimpc_plant_sample_noise: null eps"


# (H, B, N, nu, noise_hold, limits: 0 none, 1 shared, B per robot)
SHAPES = ((5, 2, 1, 1, 1, 0), (7, 3, 2, 2, 3, 1), (4, 2, 65, 12, 2, 2), (1, 1, 2, 2, 1, 0), (6, 3, 5, 2, 7, 3))


def _limits(rng, n_lim, nu, scale):
    if not n_lim:
        return None, None
    hi = scale * (0.5 + rng.random((n_lim, nu)))
    return -hi, hi


def _flat(*arrays):
    return " ".join(hx(v) for a in arrays if a is not None for v in np.ravel(a))


def check_candidates(exe, seed):
    rng = np.random.default_rng(seed)
    for H, B, N, nu, hold, n_lim in SHAPES:
        lo, hi = _limits(rng, n_lim, nu, 1.0)
        u_nom = psc.limit(rng.standard_normal((H, B, nu)), lo, hi)
        u_nom[0, 0, 0] = -0.0
        sigma = rng.random(nu)
        sigma[-1] = 0.0 if nu > 1 else sigma[-1]
        sd, draw = int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 32))
        got = doubles(run(exe, "cand", f"{H} {B} {N} {nu} {hold} {n_lim} {sd} {draw} " + _flat(u_nom, sigma, lo, hi))[0]).reshape(H, N, B, nu)
        want = psc.candidates(u_nom, sigma, psc.noise(sd, draw, B, N, psc.noise_rows(H, hold), nu), hold, lo, hi)
        _same(got, want, f"candidates {(H, B, N, nu, hold, n_lim)}")
        _same(got[:, 0], u_nom, "candidate 0 must be a copy of the plan to the bit")
        assert np.signbit(got[0, 0, 0, 0]), "-0.0 in the plan must stay -0.0 in candidate 0"
        if n_lim:
            assert np.all(got >= lo) and np.all(got <= hi)
            if N > 1:
                assert ((got[:, 1:] == lo) | (got[:, 1:] == hi)).any(), "no candidate entry sits on a bound: the limits do not bind"


def _update_case(rng, H, B, N, nu, n_lim, lam, J=None, conv=None):
    lo, hi = _limits(rng, n_lim, nu, 1.5)
    u_nom = psc.limit(rng.standard_normal((H, B, nu)), lo, hi)
    cand = psc.limit(u_nom[:, None] + 0.7 * rng.standard_normal((H, N, B, nu)), lo, hi)
    cand[:, 0] = u_nom
    J = 3.0 + rng.random((N, B)) if J is None else np.asarray(J, dtype=np.float64)
    conv = (rng.random((N, B)) < 0.8).astype(np.int32) if conv is None else np.asarray(conv, dtype=np.int32)
    return u_nom, cand, J, conv, lo, hi


def _run_update(exe, u_nom, cand, J, conv, lo, hi, lam):
    H, N, B, nu = cand.shape
    n_lim = 0 if lo is None else lo.shape[0]
    text = f"{H} {B} {N} {nu} {n_lim} {hx(lam)} " + _flat(u_nom, cand, J) + " " + " ".join(str(int(v)) for v in conv.ravel()) + " " + _flat(lo, hi)
    lines = run(exe, "update", text)
    return dict(choice=ints(lines[0]), n_eligible=ints(lines[1]), J_nom=doubles(lines[2]), J_best=doubles(lines[3]), weights=doubles(lines[4]).reshape(N, B),
                raw=doubles(lines[5]).reshape(N, B), u_new=doubles(lines[6]).reshape(H, B, nu))


def _check_update(exe, case, lam, what):
    u_nom, cand, J, conv, lo, hi = case
    got = _run_update(exe, u_nom, cand, J, conv, lo, hi, lam)
    want = psc.update(u_nom, cand, J, conv, lam, lo, hi)
    for k in got:
        _same(got[k], want[k], f"{what}: {k}")
    return got


def check_updates(exe, seed):
    rng = np.random.default_rng(seed)
    for H, B, N, nu, hold, n_lim in SHAPES:
        for lam in (0.0, 0.3):
            case = _update_case(rng, H, B, N, nu, n_lim, lam)
            got = _check_update(exe, case, lam, f"update {(H, B, N, nu, n_lim, lam)}")
            if lam == 0.0:
                ind = np.zeros((N, B))
                ind[got["choice"][got["choice"] >= 0], np.flatnonzero(got["choice"] >= 0)] = 1.0
                _same(got["weights"], ind, "with lam = 0 the weights are the indicator of the choice")
            if case[4] is not None:
                assert np.all(got["u_new"] >= case[4]) and np.all(got["u_new"] <= case[5])
    # the eligibility cases on H 3, B 5, N 4: robot 0 every candidate ineligible, 1 only candidate 0, 2 a tie, 3 NaN and +inf costs, 4 both kinds
    J = np.array([[2.0, 1.0, 4.0, nan, 2.0], [1.0, 0.5, 3.0, inf, 1.0], [1.5, 0.25, 3.0, 5.0, 3.0], [nan, 0.1, 3.5, -inf, 0.5]])
    conv = np.array([[0, 1, 1, 1, 1], [0, 0, 1, 1, 0], [0, 0, 1, 1, 1], [1, 0, 1, 1, 0]])
    for lam in (0.0, 0.8):
        case = _update_case(rng, 3, 5, 4, 2, 1, lam, J=J, conv=conv)
        got = _check_update(exe, case, lam, f"eligibility, lam {lam}")
        assert got["choice"].tolist() == [-1, 0, 1, 2, 0] and got["n_eligible"].tolist() == [0, 1, 4, 1, 2]
        _same(got["u_new"][:, 0], case[0][:, 0], "every candidate ineligible: the plan is kept")
        _same(got["u_new"][:, 1], case[0][:, 1], "only candidate 0 eligible: the plan is kept")
        assert not got["weights"][:, 0].any() and np.isnan(got["J_nom"][3]) and got["J_best"][3] == 5.0 and got["J_best"][0] == 2.0
        assert got["weights"][:, 3].tolist() == [0.0, 0.0, 1.0, 0.0], "NaN and infinite costs carry no weight"
        if lam > 0.0:
            assert got["weights"][1, 2] == got["weights"][2, 2] > got["weights"][0, 2] > 0.0 and got["weights"][1, 4] == 0.0


def test_the_candidate_law_of_the_header_is_the_numpy_restatement_exactly(host):
    check_candidates(host, 5)


def test_eligibility_choice_and_both_updates_are_the_numpy_restatement_exactly(host):
    check_updates(host, 6)


HEADER_REFUSALS = (
    (f"0 2 3 2 1 {hx(1.0)} {hx(1.0)} 1 {hx(0.0)} 1", "N below 1"),
    (f"65536 65536 1 2 1 {hx(1.0)} {hx(1.0)} 1 {hx(0.0)} 1", "N B H beyond an int"),
    (f"4 2 3 2 0 {hx(1.0)} {hx(1.0)} 1 {hx(0.0)} 1", "null sigma"),
    (f"4 2 3 2 1 {hx(1.0)} {hx(-1e-300)} 1 {hx(0.0)} 1", "a sigma entry that is negative or not finite"),
    (f"4 2 3 2 1 {hx(inf)} {hx(1.0)} 1 {hx(0.0)} 1", "a sigma entry that is negative or not finite"),
    (f"4 2 3 2 1 {hx(1.0)} {hx(nan)} 1 {hx(0.0)} 1", "a sigma entry that is negative or not finite"),
    (f"4 2 3 2 1 {hx(1.0)} {hx(1.0)} 0 {hx(0.0)} 1", "noise_hold below 1"),
    (f"4 2 3 2 1 {hx(1.0)} {hx(1.0)} 1 {hx(-0.5)} 1", "lam negative or not a number"),
    (f"4 2 3 2 1 {hx(1.0)} {hx(1.0)} 1 {hx(nan)} 1", "lam negative or not a number"),
    (f"4 2 3 2 1 {hx(1.0)} {hx(1.0)} 1 {hx(0.0)} 0", "n_iter below 1"),
    (f"4 2 3 2 1 {hx(0.0)} {hx(0.0)} 1 {hx(0.0)} 1", "ok"),
    (f"1 1 1 2 1 {hx(1.0)} {hx(1.0)} 2147483647 {hx(inf)} 1", "ok"),
)


@pytest.mark.parametrize("k", range(len(HEADER_REFUSALS)))
def test_the_headers_refusals_by_reason(host, k):
    text, reason = HEADER_REFUSALS[k]
    assert run(host, "refusal", text) == [reason]


def test_the_host_build_runs_clean_under_the_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "plant_sample_check_san")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, SRC], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr[-300:])
    check_philox(exe)
    check_deviate(exe, 12, 500)
    check_candidates(exe, 7)
    check_updates(exe, 8)
    for text, _ in HEADER_REFUSALS:
        run(exe, "refusal", text)


# ---- the refusals of the entries -----------------------------------------------------------------------------------------------------------------
def _create(**change):
    """cimpc_plant_sampler_create on a small stand-in problem (hopper_2D, B 2, H 3, L 2) with `change` applied -> (rc, reason, handle value)."""
    nq, nu, B, H, L = 4, 2, 2, 3, 2
    n = 2 * nq
    a = dict(model=2, B=B, H=H, L=L, n_iter=2, N=4, sigma=[0.1, 0.1], noise_hold=1, lam=0.0, seed=3, h=0.01, n_Q=1, n_x=1, n_lim=1, u_lo=None, u_hi=None,
             u0=np.zeros((H, B, nu)), null=None, mu=[0.5], n_mu=1, handle=True, n_terrain=0)
    a.update(change)
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib._dp)
    Q, Qf, R, xr, ur = np.eye(n), np.eye(n), np.eye(nu), np.zeros((max(a["L"], 0) + 1, a["n_x"], n)), np.zeros((max(a["L"], 1), a["n_x"], nu))
    p = dict(mu=arr(a["mu"]), Q=Q, Qf=Qf, R=R, x_ref=xr, u_ref=ur, sigma=arr(a["sigma"]), u0=arr(a["u0"]))
    opts = _lib.IpOpts()
    _lib.load().cimpc_default_ip_opts(C.byref(opts))
    po = C.byref(opts)
    if a["null"] == "opts":
        po = None
    elif a["null"]:
        p[a["null"]] = None
    lo, hi = arr(a["u_lo"]), arr(a["u_hi"])
    handle = C.c_void_p(0xdead)      # what a refusal must overwrite with NULL
    lib = _lib.load()
    rc = lib.cimpc_plant_sampler_create(a["model"], a["B"], a["H"], 0, a["n_terrain"], None, dp(p["mu"]), a["n_mu"], a["h"], po, dp(p["Q"]), dp(p["Qf"]), dp(p["R"]),
                                        a["n_Q"], 1, a["L"], a["n_x"], dp(p["x_ref"]), dp(p["u_ref"]), a["N"], dp(p["sigma"]), a["noise_hold"], a["lam"],
                                        a["n_iter"], a["seed"], a["n_lim"], dp(lo), dp(hi), dp(p["u0"]), C.byref(handle) if a["handle"] else None)
    return rc, lib.cimpc_last_error(None).decode(), handle.value


REFUSED = {
    "H 0": (dict(H=0), "H or L below 1"),
    "L 0": (dict(L=0), "H or L below 1"),
    "n_iter 0": (dict(n_iter=0), "n_iter below 1"),
    "N 0": (dict(N=0), "N below 1"),
    "N B H beyond an int": (dict(N=2 ** 30), "N B H beyond an int"),
    "null sigma": (dict(null="sigma"), "null sigma"),
    "a negative sigma": (dict(sigma=[0.1, -0.1]), "a sigma entry that is negative or not finite"),
    "an infinite sigma": (dict(sigma=[inf, 0.1]), "a sigma entry that is negative or not finite"),
    "noise_hold 0": (dict(noise_hold=0), "noise_hold below 1"),
    "a negative lam": (dict(lam=-1.0), "lam negative or not a number"),
    "a NaN lam": (dict(lam=nan), "lam negative or not a number"),
    "null u0": (dict(null="u0"), "null u0"),
    "null x_ref": (dict(null="x_ref"), "null x_ref"),
    "null opts": (dict(null="opts"), "null opts"),
    "null mu": (dict(null="mu"), "null mu"),
    "null Qf": (dict(null="Qf"), "null Qf"),
    "an unknown model": (dict(model=99), "an unknown model"),
    "B 0": (dict(B=0), "B below 1"),
    "n_Q 0": (dict(n_Q=0), "n_Q, n_R or n_x of the cost below 1"),
    "n_Q 2": (dict(n_Q=2), "n_Q of the cost neither 1 nor T"),
    "n_x 3": (dict(n_x=3), "n_x of the cost neither 1 nor B"),
    "h 0": (dict(h=0.0), "h not positive"),
    "u_lo alone": (dict(u_lo=[[-1.0, -1.0]]), "one of u_lo, u_hi without the other"),
    "n_lim 3": (dict(u_lo=[[-1.0, -1.0]], u_hi=[[1.0, 1.0]], n_lim=3), "n_lim neither 1 nor B"),
    "u_lo above u_hi": (dict(u_lo=[[2.0, -1.0]], u_hi=[[1.0, 1.0]]), "u_lo above u_hi"),
    "a NaN limit": (dict(u_lo=[[nan, -1.0]], u_hi=[[1.0, 1.0]]), "a NaN limit"),
    "a non-finite u0": (dict(u0=np.full((3, 2, 2), nan)), "a non-finite entry of u0"),
    "u0 outside the limits": (dict(u_lo=[[-1.0, -1.0]], u_hi=[[1.0, 1.0]], u0=np.full((3, 2, 2), 1.5)), "an entry of u0 outside the limits"),
    "n_mu 3": (dict(n_mu=3, mu=[0.5, 0.5, 0.5]), "an argument that cimpc_plant_rollout refuses for the B robots"),
    "terrains counted but not given": (dict(n_terrain=1), "an argument that cimpc_plant_rollout refuses for the B robots"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_create_refuses_by_reason_without_a_device_and_leaves_no_handle(what):
    change, reason = REFUSED[what]
    rc, why, handle = _create(**change)
    assert rc == INVALID
    assert why == "cimpc_plant_sampler_create: " + reason
    assert handle is None, "*handle must be NULL after a refusal"


def test_a_null_handle_is_refused_first_and_by_every_entry():
    lib = _lib.load()
    rc, why, _ = _create(handle=False, H=0)
    assert rc == INVALID and why == "cimpc_plant_sampler_create: null handle"
    some = np.zeros(8)
    somei = np.zeros(8, dtype=np.int32)
    D, I = some.ctypes.data_as(_lib._dp), somei.ctypes.data_as(_lib._ip)
    assert lib.cimpc_plant_sampler_control(None, 0, 0, D, D, D, D, D, D, I, I, D, D, I) == INVALID
    assert lib.cimpc_last_error(None).decode() == "cimpc_plant_sampler_control: null handle"
    assert not some.any() and not somei.any(), "a refused control wrote to an output"
    assert lib.cimpc_plant_sampler_plan(None, D, None, None, None, None, None) == INVALID
    assert lib.cimpc_last_error(None).decode() == "cimpc_plant_sampler_plan: null handle"
    assert lib.cimpc_plant_sampler_raw_weights(None, D) == INVALID
    assert lib.cimpc_last_error(None).decode() == "cimpc_plant_sampler_raw_weights: null handle"
    assert lib.cimpc_plant_sampler_reset(None, D) == INVALID
    assert lib.cimpc_last_error(None).decode() == "cimpc_plant_sampler_reset: null handle"
    assert lib.cimpc_plant_sampler_dims(None, I, I, I, I, I, I, I) == INVALID
    assert lib.cimpc_plant_sampler_destroy(None) == 0
    assert not some.any() and not somei.any()


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_the_exports_are_declared_and_bound(name):
    params = _prototype(name)
    assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(params) == NAMES[name]
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), name)


def test_the_source_is_built_and_states_its_rules_once():
    csrc = os.path.join(ROOT, "contactimplicitmpc", "jl_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "plant_sample.hip" in make and "plant_sample.h " in make
    src = open(os.path.join(csrc, "plant_sample.hip")).read()
    hdr = open(os.path.join(csrc, "plant_sample.h")).read()
    for name in NAMES:
        assert f'extern "C" int {name}(' in src
    for text in (src, hdr):
        assert "asm" not in text and "__builtin" not in text
    assert '#include "plant_sample.h"' in src and '#include "plant_mpc.h"' in hdr
    for rule in ("plant_sample_eps(", "plant_sample_candidate(", "plant_sample_update(", "plant_mpc_warm_start(", "plant_mpc_window(", "plant_candidates_cost_launch(",
                 "plant_step_chunks("):
        assert rule in src, rule
    assert "plant_linesearch_choice(" in hdr and "plant_feedback_limit(" in hdr and "0xD2511F53" in hdr and "0x1.3988e1409212ep+0" in hdr
    assert "plant_step_kernel" not in src and "plant_ls_cost_kernel<" not in src, "no new instantiation of an existing kernel"
    assert "__global__" in src and src.count("__global__") == 3      # begin, expand, update
    # a control step: no allocation, one synchronize
    control = src[src.index('extern "C" int cimpc_plant_sampler_control('):src.index('extern "C" int cimpc_plant_sampler_plan(')]
    assert "hipMalloc" not in control and control.count("hipStreamSynchronize") == 1 and control.count("up(") == 2      # q0 and q1: 2 B nq doubles


@pytest.mark.parametrize("name", sorted(NAMES))
def test_julia_calls_match_the_prototypes(name):
    fname = JL_FUNCS[name]
    assert f"function {fname}(" in JL, f"julia/CIMPCHip.jl has no {fname}"
    fn = JL[JL.index(f"function {fname}("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint", fn, flags=re.S)
    assert m, f"{fname} does not call {name}"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    params = _prototype(name)
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in JL_COMPAT[jt], f"argument {k}: Julia {jt} against C `{ct}`"
    doc = JL[:JL.index(f"function {fname}(")][-3000:]
    assert "unexecuted" in doc.lower(), "the docstring must say that the Julia call has not been run"


# ---- the Python class ----------------------------------------------------------------------------------------------------------------------------
def test_python_refuses_wrong_shapes_and_values_before_the_library_is_called(monkeypatch):
    from contactimplicitmpc.jl_amd import plant
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    nq, nu, B, H = 4, 2, 3, 5
    n = 2 * nq
    good = plant.TrackingReference(np.eye(n), np.eye(nu), x_ref=np.zeros((4, n)))
    a = dict(model="hopper_2D", B=B, H=H, h=0.01, mu=0.5, ref=good, u0=np.zeros((H, nu)), sigma=0.1)
    for change, match in ((dict(u0=np.zeros((H, nu + 1))), "u0 must be"), (dict(u0=np.zeros((H + 1, nu))), "u0 must be"), (dict(u0=np.zeros((H, 2, nu))), "u0 must be"),
                          (dict(u0=np.full((H, nu), np.nan)), "finite"), (dict(H=0), "B and H"), (dict(B=0), "B and H"), (dict(ref=None), "TrackingReference"),
                          (dict(h=0.0), "h must be"), (dict(mu=[0.5, 0.5]), "mu:"), (dict(n_iter=0), "n_iter"), (dict(n_samples=0), "n_samples"),
                          (dict(n_samples=2 ** 30), "n_samples"), (dict(sigma=[0.1, 0.1, 0.1]), "sigma must be"), (dict(sigma=np.zeros((2, 2))), "sigma must be"),
                          (dict(sigma=[0.1, -0.1]), "sigma must be finite"), (dict(sigma=np.inf), "sigma must be finite"), (dict(lam=-0.5), "lam"),
                          (dict(lam=np.nan), "lam"), (dict(noise_hold=0), "noise_hold"), (dict(seed=-1), "seed"), (dict(u_lo=[-1.0, -1.0]), "go together"),
                          (dict(u_lo=[2.0, 0.0], u_hi=[1.0, 1.0]), "must not exceed"),
                          (dict(ref=plant.TrackingReference(np.eye(3), np.eye(nu))), "TrackingCost"),
                          (dict(ref=plant.TrackingReference(np.eye(n), np.eye(nu), x_ref=np.zeros((4, 2, n)))), "robots")):
        kw = dict(a, **change)
        with pytest.raises(ValueError, match=match):
            plant.SamplingPolicy(kw.pop("model"), kw.pop("B"), kw.pop("H"), kw.pop("h"), kw.pop("mu"), kw.pop("ref"), kw.pop("u0"), **kw)
    with pytest.raises(TypeError):      # sigma has no default
        plant.SamplingPolicy("hopper_2D", B, H, 0.01, 0.5, good, np.zeros((H, nu)))


def test_control_refuses_wrong_states_before_the_library_is_called():
    """A policy whose handle is a stand-in: `control`, `reset` and `__call__` refuse from shapes and values alone."""
    from contactimplicitmpc.jl_amd import plant

    class Lib:
        def __getattr__(self, name):
            raise AssertionError("the library was called")
    pol = object.__new__(plant.SamplingPolicy)
    pol._handle, pol._lib, pol.B, pol.H, pol.h, pol.n_iter, pol.n_samples, pol._dims, pol._lo, pol._hi = object(), Lib(), 3, 5, 0.01, 1, 4, (4, 2, 1, 2), None, None
    pol.s, pol._fresh, pol._prev, pol.last = 0, True, None, None
    q = np.zeros((3, 4))
    for args, kw, match in (((np.zeros((3, 5)), q), {}, "q1 and v1"), ((q, np.zeros((2, 4))), {}, "q1 and v1"), ((q, q), dict(shift=-1), "shift"),
                            ((np.full((3, 4), np.inf), q), {}, "finite"), ((q, np.full((3, 4), np.nan)), {}, "finite")):
        with pytest.raises(ValueError, match=match):
            pol.control(*args, **kw)
    with pytest.raises(ValueError, match="start"):
        pol(q)
    with pytest.raises(ValueError, match="u0 must be"):
        pol.reset(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="negative"):
        pol.reset(s=-1)
    assert pol.s == 0 and pol._fresh, "a refusal changed the policy"
    pol._handle = None
    for call in (lambda: pol.control(q, q), pol.plan, pol.raw_weights, lambda: pol.plan_rollouts, pol.reset):
        with pytest.raises(ValueError, match="closed"):
            call()
    assert issubclass(plant.SamplingPolicy, plant._DevicePolicy) and issubclass(plant.ILQRPolicy, plant._DevicePolicy)
