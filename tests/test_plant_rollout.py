"""`cimpc_plant_rollout` without a device: the export and its ctypes signature, argument validation (which comes before any device
call), the launch plan of `contactimplicitmpc/jl_amd/csrc/plant_rollout_plan.h` built with g++ (tests/native/plant_rollout_plan_check.cpp),
the host-side schedule of `plant.rollout` against `OpenLoopPolicy`, and the Julia binding's `plant_rollout` read as text."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, plant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID, NO_DEVICE = -1, -2


def _prototype():
    m = re.search(r"\bint\s+cimpc_plant_rollout\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, "cimpc_plant_rollout is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


def test_export_is_declared_and_bound():
    params = _prototype()
    res, args = _lib.SIGNATURES["cimpc_plant_rollout"]
    assert res is C.c_int and len(args) == len(params) == 25
    ctype = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip,
             "const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts)}
    assert [ctype[p] for p in params] == args
    assert hasattr(_lib.load(), "cimpc_plant_rollout")


# ---- validation: hopper_2D (nq 4, nu 2, nc 1, nb 2, nw 2), B = 2, T = 3 ---------------------------------------------------------------
def _call(**over):
    mid, nq, nu, nc, fd, nw = plant.model_dims(over.pop("model_name", "hopper_2D"))
    B, T = 2, 3
    a = dict(model=mid, B=B, T=T, steps_per_launch=0, n_terrain=0, terrain=None, q0=np.zeros((B, nq)), q1=np.zeros((B, nq)),
             u=np.zeros((2, B, nu)), K_u=2, n_u=B, hold_u=2, w=np.zeros((3, 1, nw)), K_w=3, n_w=1, hold_w=1, mu=np.array([0.5, 0.6]), n_mu=B,
             h=0.01, opts=_lib.IpOpts(**dataclasses.asdict(plant.SIM_OPTS)), q=np.zeros((T + 2, B, nq)), gamma=np.zeros((T, B, nc)),
             b=np.zeros((T, B, fd * nc)), status=np.zeros((T, B), dtype=np.int32), iters=np.zeros((T, B), dtype=np.int32))
    a.update(over)
    def arg(k, v):
        if k == "opts":
            return None if v is None else C.byref(v)
        if isinstance(v, np.ndarray):
            return v.ctypes.data_as(_lib._ip if v.dtype == np.int32 else _lib._dp)
        return v
    order = ["model", "B", "T", "steps_per_launch", "n_terrain", "terrain", "q0", "q1", "u", "K_u", "n_u", "hold_u", "w", "K_w", "n_w", "hold_w",
             "mu", "n_mu", "h", "opts", "q", "gamma", "b", "status", "iters"]
    vals = [arg(k, a[k]) for k in order]
    return _lib.load().cimpc_plant_rollout(*vals)


def _opts(**kw):
    o = _lib.IpOpts(**dataclasses.asdict(plant.SIM_OPTS))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _terrains(*names):
    from contactimplicitmpc.jl_amd import terrain
    return (_lib.Terrain * len(names))(*[terrain.get(n).to_c() for n in names])


BAD = {
    "null q0": dict(q0=None), "null q1": dict(q1=None), "null u": dict(u=None), "null mu": dict(mu=None), "null opts": dict(opts=None),
    "null q": dict(q=None), "null gamma": dict(gamma=None), "null b": dict(b=None), "null status": dict(status=None), "null iters": dict(iters=None),
    "B = 0": dict(B=0), "T = 0": dict(T=0), "T < 0": dict(T=-1), "K_u = 0": dict(K_u=0), "hold_u = 0": dict(hold_u=0),
    "steps_per_launch < 0": dict(steps_per_launch=-1), "h = 0": dict(h=0.0),
    "n_u neither 1 nor B": dict(n_u=3), "n_u = 0": dict(n_u=0), "n_w neither 1 nor B": dict(n_w=3), "n_mu neither 1 nor B": dict(n_mu=0),
    "K_w = 0 with w": dict(K_w=0), "hold_w = 0 with w": dict(hold_w=0),
    "unknown model": dict(model=9), "particle_2D without a terrain": dict(model=6),
    "terrain count without terrains": dict(n_terrain=1), "terrains without a count": dict(terrain=_terrains("sine1_2D_lc")),
    "terrain count neither 1 nor B": dict(n_terrain=3, terrain=_terrains("sine1_2D_lc", "sine1_2D_lc", "sine1_2D_lc")),
    "a 3-D terrain under a planar model": dict(n_terrain=1, terrain=_terrains("sine1_3D_lc")),
    "max_iter = 0": dict(opts=_opts(max_iter=0)), "max_ls < 0": dict(opts=_opts(max_ls=-1)), "r_tol = 0": dict(opts=_opts(r_tol=0.0)),
    "kappa_tol = 0": dict(opts=_opts(kappa_tol=0.0)), "ls_scale = 1": dict(opts=_opts(ls_scale=1.0)),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_invalid_arguments_are_refused_without_a_device(what):
    assert _call(**BAD[what]) == INVALID


def test_the_wall_takes_no_rough_terrain():
    assert _call(model_name="centroidal_quadruped_wall", n_terrain=1, terrain=_terrains("sine1_3D_lc")) == INVALID


def test_a_valid_call_needs_a_gfx950():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    assert _call() == NO_DEVICE
    assert _call(w=None, K_w=0, n_w=0, hold_w=0, n_mu=1, n_u=1, n_terrain=1, terrain=_terrains("sine1_2D_lc"), steps_per_launch=2) == NO_DEVICE
    with pytest.raises(_lib.CimpcError):
        plant.rollout("hopper_2D", np.zeros(4), np.zeros(4), np.zeros((2, 2)), 0.01, 0.5)


# ---- the launch plan ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("rollout_plan") / "plant_rollout_plan_check")
    # the sanitizer runtimes linked statically: the program then runs the same whatever else the loader brings in
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"] if request.param == "sanitized" else []
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, os.path.join(HERE, "native", "plant_rollout_plan_check.cpp")]
    if flags and subprocess.run(cmd, capture_output=True).returncode != 0:
        pytest.skip("this g++ has no static sanitizer runtime")
    subprocess.check_call(cmd)

    def run(queries):
        text = "".join(" ".join(str(v) for v in q) + "\n" for q in queries)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
        assert len(out) == len(queries)
        return [[int(v) for v in line.split()] for line in out]
    return run


def test_schedule_row_rule(plan):
    """test/simulator/open_loop.jl: N_sample = 3 over 4 controls gives (1-based) indices 1, 1, 1, 2, 2, 2, ...; past the last control
    the row stays the last one."""
    got = [r[0] for r in plan([("row", t, 3, 4) for t in range(20)])]
    assert got == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3] + [3] * 8
    pol = plant.OpenLoopPolicy([np.array([float(k)]) for k in range(4)], N_sample=3)
    assert [int(round(3 * pol(t + 1)[0])) for t in range(12)] == got[:12]
    assert [r[0] for r in plan([("row", t, 1, 1) for t in range(3)] + [("row", 5, 1, 7), ("row", 2 ** 31 - 1, 1, 2 ** 31 - 1)])] == [0, 0, 0, 5, 2 ** 31 - 2]


@pytest.mark.parametrize("T,chunk", [(1, 64), (3, 2), (64, 64), (65, 64), (7, 3)])
def test_chunks_are_contiguous_covering_and_bounded(plan, T, chunk):
    for spl in (chunk, 0) if chunk == 64 else (chunk,):          # 0: the default, 64
        n, *flat = plan([("chunks", T, spl)])[0]
        chunks = list(zip(flat[0::2], flat[1::2]))
        assert n == len(chunks) == -(-T // chunk)
        t = 0
        for t0, steps in chunks:
            assert t0 == t and 1 <= steps <= chunk
            t += steps
        assert t == T
    assert plan([("chunks", 7, 3)])[0] == [3, 0, 3, 3, 3, 6, 1]


# ---- plant.rollout on the host ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_robot", [False, True])
@pytest.mark.parametrize("N_sample,steps", [(1, None), (2, 7), (3, None), (2, 11)])
def test_host_schedule_is_the_open_loop_policy(per_robot, N_sample, steps):
    rng = np.random.default_rng(N_sample)
    K, B, nu = 4, 3, 2
    u = rng.standard_normal((K, B, nu) if per_robot else (K, nu))
    rows, applied = plant.open_loop_controls("hopper_2D", u, B, N_sample, steps)
    T = K * N_sample if steps is None else steps
    assert rows.shape == (K, B if per_robot else 1, nu) and rows.flags["C_CONTIGUOUS"] and applied.shape == (T, B, nu)
    pol = plant.OpenLoopPolicy(list(u), N_sample=N_sample)
    for t in range(min(T, K * N_sample)):                          # the policy itself runs out after K N_sample steps
        np.testing.assert_array_equal(applied[t], np.broadcast_to(pol(t + 1), (B, nu)))
    for t in range(K * N_sample, T):                               # ... the rollout holds the last control
        np.testing.assert_array_equal(applied[t], applied[K * N_sample - 1])


def test_host_shapes_are_checked_before_the_library_is_called():
    z = np.zeros
    for kw in (dict(u=z((3, 5))), dict(u=z((3, 2, 2))), dict(u=z((0, 2))), dict(q1=z((3, 5))), dict(v1=z((2, 4))), dict(mu=[0.5, 0.5]),
               dict(w=z((3, 3))), dict(w=z((3, 2, 2))), dict(N_sample=0), dict(w_hold=0), dict(steps=0)):
        a = dict(q1=z((3, 4)), v1=z((3, 4)), u=z((2, 2)), mu=0.5)
        a.update(kw)
        extra = {k: a.pop(k) for k in ("w", "N_sample", "w_hold", "steps") if k in a}
        with pytest.raises(ValueError):
            plant.rollout("hopper_2D", a["q1"], a["v1"], a["u"], 0.01, a["mu"], **extra)


# ---- the Julia binding ------------------------------------------------------------------------------------------------------------------
def _jl_plant_rollout():
    fn = JL[JL.index("function plant_rollout("):]
    return fn[:fn.index("\nend\n") + 5]


def test_julia_plant_rollout_matches_the_prototype():
    params = _prototype()
    fn = _jl_plant_rollout()
    m = re.search(r"@ccall LIB\.cimpc_plant_rollout\((.*?)\)::Cint", fn, flags=re.S)
    assert m, "plant_rollout does not call cimpc_plant_rollout"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    compat = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*"},
              "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"}}
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in compat[jt], f"argument {k}: Julia {jt} against C `{ct}`"


def test_julia_plant_rollout_is_sized_from_the_model_tables():
    fn = _jl_plant_rollout()
    assert not re.search(r"zeros\(\s*(Cint\s*,\s*)?\d", fn), "literal array size in plant_rollout"
    assert "_plant_dims(model)" in fn
    dims = JL[JL.index("function _plant_dims("):]
    dims = dims[:dims.index("\nend\n")]
    for table in ("PLANT_MODELS", "PLANT_ENV_MODELS", "PLANT_SPATIAL_MODELS"):
        assert f"haskey({table}, model)" in dims, table
    assert "error(" in dims
    # the Julia mirror of cimpc_terrain lists the header's fields in the header's order
    body = re.search(r"typedef struct cimpc_terrain\s*\{(.*?)\}\s*cimpc_terrain\s*;", HDR, flags=re.S).group(1)
    c_fields = [re.match(r"\w+\s+(\w+)", " ".join(s.split())).group(1) for s in body.split(";") if s.strip()]
    jl = re.search(r"struct Terrain[^\n]*\n(.*?)\nend", JL, flags=re.S).group(1)
    assert [d.split("::")[0].strip() for line in jl.split("\n") for d in line.split("#")[0].split(";") if "::" in d] == c_fields
