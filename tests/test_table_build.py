"""The device table build without a device: `cimpc_set_linearization_batch`, `cimpc_linearize_knots` and `cimpc_get_table` as
declared, exported, bound and mirrored in Julia; their argument validation (which comes before any device call); the Python shape
checks; the `tables` keyword of `lcp_models.reference_problem`; and the one text every table is built by - `lin_table_build_knot` of
`contactimplicitmpc/jl_amd/csrc/lin_table_build.h`, built with g++ (tests/native/lin_table_build_check.cpp; also as a sanitized
stand-alone program) - against a NumPy statement of what the table means, one seeded knot per layout family, and against the tables
recorded bit for bit in tests/golden/lin_table_sha256.json (tests/table_build_cases.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, lcp_models, policy, solver
import table_build_cases as cases
from table_build_cases import LAYOUTS, knot as _knot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID = -1
NEW = {"cimpc_set_linearization_batch": 8, "cimpc_linearize_knots": 9, "cimpc_get_table": 3}
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "cimpc_handle": C.c_void_p,
         "const cimpc_terrain*": C.POINTER(_lib.Terrain)}


def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


# ---- the exports ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NEW))
def test_export_is_declared_and_bound(name):
    params = _prototype(name)
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(params) == NEW[name]
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), name)


def test_the_version_counts_the_new_entries():
    assert _lib.load().cimpc_version() >= 107


def test_julia_calls_match_the_prototypes():
    compat = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Terrain}": {"const cimpc_terrain*"},
              "Ptr{Cvoid}": {"cimpc_handle"}}
    for fn_name, name in (("set_linearization_batch!", "cimpc_set_linearization_batch"), ("linearize_knots!", "cimpc_linearize_knots"),
                          ("get_table", "cimpc_get_table")):
        fn = JL[JL.index("function " + fn_name + "("):]
        fn = fn[:fn.index("\nend\n") + 5]
        m = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint", fn, flags=re.S)
        if m:
            types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
        else:
            m = re.search(r"ccall\(\(:" + name + r",\s*LIB\),\s*Cint,\s*\(([^()]*)\)", fn)
            assert m, f"{fn_name} does not call {name}"
            types = [a.strip() for a in m.group(1).split(",")]
        params = _prototype(name)
        assert len(types) == len(params), f"{name}: {len(types)} Julia arguments, {len(params)} C parameters"
        for k, (jt, ct) in enumerate(zip(types, params)):
            assert ct in compat[jt], f"{name} argument {k}: Julia {jt} against C `{ct}`"
        assert not re.search(r"zeros\(\s*(Cint\s*,\s*)?\d", fn), f"literal array size in {fn_name}"
    assert "_lin_dims(hs)" in JL and "cimpc_query_sizes" in JL[JL.index("function get_table("):]


def test_a_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    a = np.zeros(64)
    p = a.ctypes.data_as(_lib._dp)
    assert lib.cimpc_set_linearization_batch(None, 1, 1, p, p, p, p, p) == INVALID
    assert lib.cimpc_linearize_knots(None, 0, 1, 1, 0, None, p, p, 1e-4) == INVALID
    assert lib.cimpc_get_table(None, 1, p) == INVALID


# ---- the Python mirrors -----------------------------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the shapes were checked")


def _solver_without_a_device(nq=11, nu=8, nw=2, nc=4, nb=8, H_ref=6):
    s = solver.CIMPCSolver.__new__(solver.CIMPCSolver)
    s.lib, s.h = _NoLibrary(), None
    s.nq, s.nu, s.nw, s.nc, s.nb, s.H_ref = nq, nu, nw, nc, nb, H_ref
    s.nz, s.nth = nq + 4 * nc + 2 * nb, 2 * nq + nu + nw + 2
    return s


def test_python_shapes_are_checked_before_the_library_is_called():
    s = _solver_without_a_device()
    nz, nth, N = s.nz, s.nth, 3
    good = dict(t0=1, z0=np.zeros((N, nz)), th0=np.zeros((N, nth)), r0=np.zeros((N, nz)), rz0=np.zeros((N, nz, nz)), rth0=np.zeros((N, nz, nth)))
    bad = [dict(z0=np.zeros((N, nz + 1))), dict(z0=np.zeros(nz)), dict(z0=np.zeros((0, nz))), dict(th0=np.zeros((N + 1, nth))), dict(r0=np.zeros((N, nz - 1))),
           dict(rz0=np.zeros((N, nz, nth))), dict(rth0=np.zeros((N, nth, nz))), dict(rz0=np.zeros((nz, nz))), dict(t0=0), dict(t0=5), dict(t0=7)]
    for over in bad:
        with pytest.raises(ValueError):
            s.set_linearization_batch(**{**good, **over})
    with pytest.raises(AssertionError):          # ... and a well-formed call does reach the library
        s.set_linearization_batch(**good)
    z, th = np.zeros((N, nz)), np.ones((N, nth))
    for args, kw in (((("quadruped", z[:, :-1], th, 1e-4)), {}), (("quadruped", z, th[:2], 1e-4), {}), (("quadruped", z[0], th[0], 1e-4), {}),
                     (("quadruped", z, th, 1e-4), dict(t0=5)), (("quadruped", z, th, 1e-4), dict(t0=0)),
                     (("flamingo", z, th, 1e-4), {}),                                     # another model's dimensions
                     (("quadruped", z, th, 1e-4), dict(terrain=["sine1_2D_lc", "sine1_2D_lc"]))):      # neither 1 nor N terrains
        with pytest.raises(ValueError):
            s.linearize_knots(*args, **kw)
    with pytest.raises(KeyError):
        s.linearize_knots("unicycle", z, th, 1e-4)
    with pytest.raises(AssertionError):
        s.linearize_knots("quadruped", z, th, 1e-4, t0=4)
    for t in (0, 7):
        with pytest.raises(ValueError):
            s.get_table(t)


def test_tables_keyword_leaves_the_tables_out_and_nothing_else():
    model = lcp_models.PushBot()
    gait = lcp_models.constant_reference(model, [0.1, 0.05], 3, 0.04)
    called = []

    def never(z, th, kappa):
        called.append(1)
        return model.linearize_batch(z, th, kappa)
    P0 = lcp_models.reference_problem(model, gait, 1e-4)
    P1 = lcp_models.reference_problem(model, gait, 1e-4, linearize=never, tables=False)
    assert not called and P1.r0 is None and P1.rz0 is None and P1.rth0 is None
    assert P0.r0 is not None and P1.model is model and (P1.H, P1.h, P1.kappa) == (P0.H, P0.h, P0.kappa)
    for f in ("q", "u", "w", "gamma", "b", "z", "theta"):
        assert np.array_equal(getattr(P0, f), getattr(P1, f)), f

    class Traj:
        H, h = P0.H, P0.h
        q, u, w, gamma, b, z, theta = P0.q, P0.u, P0.w, P0.gamma, P0.b, P0.z, P0.theta
    Q1 = lcp_models.reference_problem_from_traj(model, Traj, 1e-4, tables=False)
    assert Q1.r0 is None and Q1.rz0 is None and Q1.rth0 is None and np.array_equal(Q1.z, P0.z) and np.array_equal(Q1.theta, P0.theta)
    assert np.array_equal(lcp_models.reference_problem_from_traj(model, Traj, 1e-4, tables=True).r0, P0.r0)
    # a policy over the host path has nothing to upload from such a problem, and says so before it asks for a device
    w = np.tile(np.eye(model.nq), (3, 1, 1))
    with pytest.raises(ValueError, match="device_tables"):
        policy.CIMPCPolicy(P1, w, np.tile(np.eye(model.nu), (3, 1, 1)), mode=1)


# ---- the kernel's text on the host ------------------------------------------------------------------------------------------------------
# the layout families and their knots: tests/table_build_cases.py
OFFSETS = ("ldw", "gst", "oW", "oCAi", "oAi", "oDy1", "oDx", "oRx", "oRy1", "oRthDyn", "oRthRst", "oGs", "oK0", "oAiB", "oVec", "oTh0", "size")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("lin_table_build") / "lin_table_build_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"] if request.param == "sanitized" else []
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, os.path.join(HERE, "native", "lin_table_build_check.cpp")]
    if flags and subprocess.run(cmd, capture_output=True).returncode != 0:
        pytest.skip("this g++ has no static sanitizer runtime")
    subprocess.check_call(cmd)

    def run(dims, z0, th0, r0, rz0, rth0):
        vals = np.concatenate([z0, th0, r0, rz0.T.ravel(), rth0.T.ravel()])         # the matrices column-major
        out = subprocess.run([exe], input=" ".join(str(d) for d in dims) + " " + " ".join(float(v).hex() for v in vals), capture_output=True,
                             text=True, check=True).stdout.split("\n")
        if out[0] == "invalid":
            return None, None
        L = dict(zip(OFFSETS, (int(v) for v in out[0].split())))
        if out[1] == "singular":
            return L, None
        return L, np.array([float.fromhex(v) for v in out[1:1 + L["size"]]])
    return run


def _meaning(dims, z0, th0, r0, rz0, rth0):
    """What each block of the table means (lin_table.h), in NumPy: name -> matrix [row i, column k], or vector."""
    nx, ny, nth, G, nths, adj = dims
    Dx, Dy1, Rx, Ry1 = rz0[:nx, :nx], rz0[:nx, nx:nx + ny], rz0[nx:nx + ny, :nx], rz0[nx:nx + ny, nx:nx + ny]
    rthdyn, rthrst = rth0[:nx], rth0[nx:nx + ny]
    Ai = np.linalg.inv(Dx)
    CAi = Rx @ Ai
    CAiB = CAi @ Dy1
    W = Ry1 - CAiB
    np.fill_diagonal(W, 0.0)
    exact = dict(Dx=Dx, Dy1=Dy1, Rx=Rx, Ry1=Ry1, RthDyn=rthdyn, RthRst=rthrst, Th0=th0, RY2=np.array([rz0[nx + i, nx + ny + i] for i in range(ny)]),
                 RY1D=np.diag(Ry1).copy(), RDYN0=r0[:nx], RRST0=r0[nx:nx + ny], X0=z0[:nx], Y10=z0[nx:nx + ny], Y20=z0[nx + ny:])
    computed = dict(Ai=Ai, CAi=CAi, W=W, CAIBD=np.diag(CAiB).copy())
    if nths:
        computed["Gs"] = CAi @ rthdyn[:, :nths] - rthrst[:, :nths]
    if adj:
        computed["K0"] = Ai @ rthdyn[:, :nths]
        computed["AiB"] = Ai @ Dy1
    return exact, computed, np.linalg.cond(Dx)


def _blocks(dims, L, T):
    """The table taken apart by the printed layout -> (name -> block in the orientation of `_meaning`, entries no block owns)."""
    nx, ny, nth, G, nths, adj = dims
    owned = np.zeros(L["size"], dtype=bool)

    def strided(off, rows, cols, ld=G):              # element (i, k) at off + k * ld + i
        idx = off + np.arange(cols)[None, :] * ld + np.arange(rows)[:, None]
        assert not owned[idx].any(), "two blocks share an entry"
        owned[idx] = True
        return T[idx]
    out = dict(W=strided(L["oW"], ny, ny, L["ldw"]).T, CAi=strided(L["oCAi"], ny, nx), Ai=strided(L["oAi"], nx, nx), Dy1=strided(L["oDy1"], nx, ny),
               Dx=strided(L["oDx"], nx, nx), Rx=strided(L["oRx"], ny, nx), Ry1=strided(L["oRy1"], ny, ny), RthDyn=strided(L["oRthDyn"], nx, nth),
               RthRst=strided(L["oRthRst"], ny, nth))
    if nths:
        out["Gs"] = strided(L["oGs"], nths, ny, nths).T if L["gst"] else strided(L["oGs"], ny, nths)
    if adj:
        out["K0"] = strided(L["oK0"], nx, nths, nx)
        out["AiB"] = strided(L["oAiB"], ny, nx, ny).T
    for v, (name, n) in enumerate((("RY2", ny), ("RY1D", ny), ("CAIBD", ny), ("RDYN0", nx), ("RRST0", ny), ("X0", nx), ("Y10", ny), ("Y20", ny))):
        out[name] = strided(L["oVec"] + v * G, n, 1)[:, 0]
    out["Th0"] = strided(L["oTh0"], nth, 1)[:, 0]
    return out, T[~owned]


C_BOUND = 10.0 * 0.32      # ten times the largest ratio measured (docstring below)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_the_built_table_means_what_lin_table_h_says(harness, name):
    """Every block against NumPy: the copied blocks exactly, the padding exactly zero, the computed blocks (Ai = Dx^-1, CAi, W off the
    diagonal, diag CAiB, Gs, K0, AiB) within c * 2^-52 * cond_2(Dx) * max|entry of the block|.  Measured on the host (g++ -O2, both
    builds alike): the largest ratio deviation / (2^-52 cond max|entry|) over all blocks of a layout is 0.32 for pushbot mode 1, 0.23
    hopper_3D, 0.22 quadruped, 0.15 at 64 x 64, 0.12 the wall, 0.11 centroidal, 0.10 the wall's generic layout; c = 3.2 is ten times the
    largest, for the summation order of the BLAS behind NumPy."""
    dims, knot = LAYOUTS[name], _knot(name)
    L, T = harness(dims, *knot)
    assert T is not None and T.shape == (L["size"],)
    got, rest = _blocks(dims, L, T)
    assert np.array_equal(rest, np.zeros_like(rest)), "padding is not zero"
    exact, computed, cond = _meaning(dims, *knot)
    assert sorted(got) == sorted({**exact, **computed})
    for k, want in exact.items():
        assert np.array_equal(got[k], want), k
    assert np.array_equal(np.diag(got["W"]), np.zeros(dims[1]))
    worst = 0.0
    for k, want in computed.items():
        unit = 2.0 ** -52 * cond * np.abs(want).max()
        ratio = np.abs(got[k] - want).max() / unit
        worst = max(worst, ratio)
        print(f"{name} {k}: cond {cond:.3g}, max|entry| {np.abs(want).max():.3g}, deviation / (2^-52 cond max|entry|) = {ratio:.3g}")
        assert ratio <= C_BOUND, (name, k, ratio)
    print(f"{name}: largest ratio {worst:.3g}")


def test_a_singular_dx_is_refused_as_the_packer_refuses_it(harness):
    L, T = harness(LAYOUTS["quadruped"], *_knot("quadruped", singular=True))
    assert L is not None and T is None


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_the_built_table_is_the_recorded_one_bit_for_bit(harness, name):
    """Every knot of the layout - its own, the three that make the elimination exchange rows and skip zero multipliers, the singular
    one - against the SHA-256 recorded from the packer `cimpc_set_linearization` had of its own before it ran this text: the bits of
    the one remaining statement of the table's arithmetic, pinned without a GPU."""
    want = cases.recorded()[name]
    assert sorted(want["knots"]) == sorted(cases.KNOTS)
    for kn, k in cases.knots(name).items():
        L, T = harness(LAYOUTS[name], *k)
        assert L["size"] == want["size"], kn
        assert (T is None) == (kn == "singular"), kn
        assert cases.table_hash(T) == want["knots"][kn], f"{name}, knot {kn!r}"
