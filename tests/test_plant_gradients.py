"""Step gradients (`cimpc_plant_sensitivity`, `cimpc_plant_rollout_grad`, `plant.sensitivity`, `diff_sol=True`) without a device: the
rollout cases of tests/plant_gradient_cases.py held to their conditions on trajectories the CPU restatements make, argument
validation (which comes before any device call), the LDS plan of csrc/plant_sensitivity_plan.h built with g++, the exports and their
ctypes signatures, `StepGradients` on a hand-made array, and the Julia binding read as text."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, plant
import plant_gradient_cases as pgc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID, NO_DEVICE = -1, -2
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip,
         "const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts)}


# ---- the rollout cases, on CPU-made trajectories ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_rollout_case_is_differentiable_everywhere_on_the_cpu_trajectory(which):
    """Every step of the case converges on the CPU restatement, and at every step both float64 references (LAPACK, the kernel's
    elimination order) stay within 1e-6 of the longdouble solve: the GPU test may then leave no step out."""
    c = pgc.rollout_case(which)
    st, Z, TH = pgc.cpu_rollout(which)
    nq, nu, nc = pgc.dims(c["model"])[:3]
    assert st.all()
    refs = pgc.rollout_references(c, Z, TH, pgc.REG, 2 * nq + nu)
    for t in range(Z.shape[0]):
        for b in range(Z.shape[1]):
            r = refs[t, b]
            print(f"{which} t={t} b={b}: max gamma {Z[t, b, nq:nq + nc].max():.3g}, cond R {r['cond']:.2e}, d_lapack {r['d_lapack']:.2e}, "
                  f"d_order {r['d_order']:.2e}, max|dz| {float(np.abs(r['ld']).max()):.3g}")
            assert max(r["d_lapack"], r["d_order"]) <= pgc.REF_LIMIT
            assert np.isfinite(r["ld"].astype(float)).all()


def test_hopper_case_has_flight_and_hard_contact():
    st, Z, TH = pgc.cpu_rollout("hopper_2D")
    gamma = Z[:, :, 4]
    assert (gamma < 1e-6).any() and (gamma > 1.0).any()
    assert ((gamma > 1e-3) & (gamma < 1.0)).any()      # and the light contact in between


def test_particle_case_lands_and_slides():
    c = pgc.rollout_case("particle")
    st, Z, TH = pgc.cpu_rollout("particle")
    gamma, q2 = Z[:, 0, 3], Z[:, 0, :3]
    assert gamma[0] < 1e-6 and (gamma[-6:] > 1e-2).all()
    assert np.linalg.norm(q2[-1, :2] - q2[-6, :2]) > 1e-3      # it moves along the surface while in contact


def test_regularization_is_the_definition():
    """R differs from dr/dz in the 2 ny entries of the bilinear rows alone, and there it is max(y, reg)."""
    nq, ny = 3, 6
    rng = np.random.default_rng(0)
    rz = rng.standard_normal((15, 15))
    z = np.concatenate([rng.standard_normal(3), [1e-14, 0.5, 2e-9, 0.0, 1e-3, 0.3], [0.7, 1e-21, 0.4, 1e-9, 5e-10, 0.2]])
    R = pgc.regularized(rz, z, nq, ny, 1e-9)
    want = rz.copy()
    for t in range(ny):
        want[nq + ny + t, nq + t] = max(z[nq + ny + t], 1e-9)
        want[nq + ny + t, nq + ny + t] = max(z[nq + t], 1e-9)
    np.testing.assert_array_equal(R, want)
    assert R[nq + ny + 1, nq + 1] == 1e-9 and R[nq + ny + 1, nq + ny + 1] == 0.5 and R[nq + ny + 3, nq + 3] == 1e-9


def test_kernel_order_restatement_solves():
    rng = np.random.default_rng(1)
    M = rng.standard_normal((9, 9))[:, rng.permutation(9)]
    rhs = rng.standard_normal((9, 4))
    np.testing.assert_allclose(pgc.solve_kernel_order(M, rhs), np.linalg.solve(M, rhs), rtol=0, atol=1e-12)
    with pytest.raises(np.linalg.LinAlgError):
        pgc.solve_kernel_order(np.zeros((2, 2)), np.ones(2))


# ---- exports and signatures ----------------------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("cimpc_plant_sensitivity", 10), ("cimpc_plant_rollout_grad", 30)])
def test_exports_are_declared_and_bound(name, n_args):
    params = _prototype(name)
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(params) == n_args
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), name)


def test_rollout_grad_extends_the_rollout_prototype():
    assert _prototype("cimpc_plant_rollout_grad")[:25] == _prototype("cimpc_plant_rollout")
    assert _prototype("cimpc_plant_rollout_grad")[25:] == ["double", "int", "double*", "double*", "int*"]


# ---- validation: hopper_2D (nq 4, nu 2, nc 1, nb 2, nw 2: nz 12, ntheta 14, nr 7) -----------------------------------------------------------
def _arg(k, v):
    if k == "opts":
        return None if v is None else C.byref(v)
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(_lib._ip if v.dtype == np.int32 else _lib._dp)
    return v


def _terrains(*names):
    from contactimplicitmpc.jl_amd import terrain
    return (_lib.Terrain * len(names))(*[terrain.get(n).to_c() for n in names])


def _sens(**over):
    mid = plant.model_dims(over.pop("model_name", "hopper_2D"))[0]
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(over.pop("dims_of", "hopper_2D"))
    N = 2
    a = dict(model=mid, N=N, n_terrain=0, terrain=None, z=np.full((N, nz), 0.5), theta=np.full((N, nth), 0.5), reg=1e-9, n_cols=nth,
             dz=np.zeros((N, nth, nr)), status=np.zeros(N, dtype=np.int32))
    a.update(over)
    order = ["model", "N", "n_terrain", "terrain", "z", "theta", "reg", "n_cols", "dz", "status"]
    return _lib.load().cimpc_plant_sensitivity(*[_arg(k, a[k]) for k in order])


def _grad(**over):
    mid = plant.model_dims("hopper_2D")[0]
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims("hopper_2D")
    B, T = 2, 3
    a = dict(model=mid, B=B, T=T, steps_per_launch=0, n_terrain=0, terrain=None, q0=np.zeros((B, nq)), q1=np.zeros((B, nq)),
             u=np.zeros((2, B, nu)), K_u=2, n_u=B, hold_u=2, w=None, K_w=1, n_w=1, hold_w=1, mu=np.array([0.5, 0.6]), n_mu=B,
             h=0.01, opts=_lib.IpOpts(**dataclasses.asdict(plant.SIM_OPTS)), q=np.zeros((T + 2, B, nq)), gamma=np.zeros((T, B, nc)),
             b=np.zeros((T, B, nb)), status=np.zeros((T, B), dtype=np.int32), iters=np.zeros((T, B), dtype=np.int32),
             reg=1e-9, n_cols=2 * nq + nu, z=np.zeros((T, B, nz)), dz=np.zeros((T, B, 2 * nq + nu, nr)), grad_status=np.zeros((T, B), dtype=np.int32))
    a.update(over)
    order = ["model", "B", "T", "steps_per_launch", "n_terrain", "terrain", "q0", "q1", "u", "K_u", "n_u", "hold_u", "w", "K_w", "n_w", "hold_w",
             "mu", "n_mu", "h", "opts", "q", "gamma", "b", "status", "iters", "reg", "n_cols", "z", "dz", "grad_status"]
    return _lib.load().cimpc_plant_rollout_grad(*[_arg(k, a[k]) for k in order])


BAD_SENS = {
    "n_cols = 0": dict(n_cols=0), "n_cols = ntheta + 1": dict(n_cols=15), "n_cols < 0": dict(n_cols=-1),
    "reg < 0": dict(reg=-1e-9), "reg NaN": dict(reg=float("nan")), "reg Inf": dict(reg=float("inf")),
    "null dz": dict(dz=None), "null status": dict(status=None), "null z": dict(z=None), "null theta": dict(theta=None), "N = 0": dict(N=0),
    "terrain count neither 1 nor N": dict(n_terrain=3, terrain=_terrains("sine1_2D_lc", "sine1_2D_lc", "sine1_2D_lc")),
    "terrain count without terrains": dict(n_terrain=1), "terrains without a count": dict(terrain=_terrains("sine1_2D_lc")),
    "a 3-D terrain under a planar model": dict(n_terrain=1, terrain=_terrains("sine1_3D_lc")),
    "unknown model": dict(model=9), "particle_2D without a terrain": dict(model=6),
    "h = 0 at a knot": dict(theta=np.concatenate([np.full((2, 13), 0.5), [[0.5], [0.0]]], axis=1)),
}
BAD_GRAD = {
    "n_cols = 0": dict(n_cols=0), "n_cols = ntheta + 1": dict(n_cols=15), "reg < 0": dict(reg=-1.0), "reg NaN": dict(reg=float("nan")),
    "null dz": dict(dz=None), "null grad_status": dict(grad_status=None), "unknown model": dict(model=9),
    "terrain count neither 1 nor B": dict(n_terrain=3, terrain=_terrains("sine1_2D_lc", "sine1_2D_lc", "sine1_2D_lc")),
    # ... and what cimpc_plant_rollout refuses
    "null q": dict(q=None), "T = 0": dict(T=0), "n_u neither 1 nor B": dict(n_u=3), "h = 0": dict(h=0.0),
}


@pytest.mark.parametrize("what", sorted(BAD_SENS))
def test_sensitivity_refuses_invalid_arguments_without_a_device(what):
    assert _sens(**BAD_SENS[what]) == INVALID


@pytest.mark.parametrize("what", sorted(BAD_GRAD))
def test_rollout_grad_refuses_invalid_arguments_without_a_device(what):
    assert _grad(**BAD_GRAD[what]) == INVALID


def test_a_valid_call_needs_a_gfx950():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    assert _sens() == NO_DEVICE
    assert _sens(n_cols=1, reg=0.0, n_terrain=1, terrain=_terrains("sine1_2D_lc")) == NO_DEVICE
    assert _sens(model_name="centroidal_quadruped_wall", dims_of="centroidal_quadruped_wall") == NO_DEVICE      # the largest shape fits
    assert _grad() == NO_DEVICE
    assert _grad(z=None, n_cols=14, reg=0.0, steps_per_launch=1) == NO_DEVICE
    with pytest.raises(_lib.CimpcError):
        plant.sensitivity("hopper_2D", np.full(12, 0.5), np.full(14, 0.5), 1e-9)
    with pytest.raises(_lib.CimpcError):
        plant.rollout("hopper_2D", np.zeros(4), np.zeros(4), np.zeros((2, 2)), 0.01, 0.5, diff_sol=True)


def test_python_checks_shapes_and_columns_before_the_library_is_called():
    z, th = np.full((2, 12), 0.5), np.full((2, 14), 0.5)
    for kw in (dict(n_cols=0), dict(n_cols=15)):
        with pytest.raises(ValueError):
            plant.sensitivity("hopper_2D", z, th, 1e-9, **kw)
    with pytest.raises(ValueError):
        plant.sensitivity("hopper_2D", z, th[:1], 1e-9)
    for kw in (dict(grad_cols=0), dict(grad_cols=15), dict(grad_reg=-1.0), dict(grad_reg=float("nan"))):
        with pytest.raises(ValueError):
            plant.rollout("hopper_2D", np.zeros(4), np.zeros(4), np.zeros((2, 2)), 0.01, 0.5, diff_sol=True, **kw)
        with pytest.raises(ValueError):
            plant.plant_step("hopper_2D", np.zeros(4), np.zeros(4), np.zeros(2), 0.5, 0.01, diff_sol=True, **kw)


# ---- the LDS plan ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lds_plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("sens_plan") / "plant_sensitivity_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "native", "plant_sensitivity_plan_check.cpp")])

    def run(queries):
        text = "".join(f"{nz} {nc}\n" for nz, nc in queries)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
        assert len(out) == len(queries)
        return [[int(v) for v in line.split()] for line in out]
    return run


def test_every_model_fits_the_lds_and_a_larger_shape_is_refused(lds_plan):
    """The need is nz (nz + n_cols) + nz + 2 doubles next to the static arrays; every compiled model fits at every n_cols (so the
    entry points' refusal cannot be reached through a model id), and the first shapes over the budget are refused."""
    models = [m for t in (plant.MODELS, plant.TERRAIN_MODELS, plant.CENTROIDAL_ENV_MODELS, plant.SPATIAL_MODELS, plant.WALLED_MODELS) for m in t]
    shapes = [(pgc.dims(m)[5], pgc.dims(m)[6]) for m in models]
    for (nz, nth), (lds, static, cap, fits) in zip(shapes, lds_plan(shapes)):
        assert lds == (nz * (nz + nth) + nz + 2) * 8 and cap == 160 * 1024 and fits == 1
    assert (114, 53) in shapes
    (lds_w, static, cap, fits_w), (_, _, _, fits_117), (lds_118, _, _, fits_118), (_, _, _, fits_cols), (_, _, _, fits_0) = \
        lds_plan([(114, 53), (117, 53), (118, 53), (114, 66), (66, 0)])
    assert lds_w == 153232 and fits_w == 1 and fits_117 == 1
    assert lds_118 + static > cap and fits_118 == 0 and fits_cols == 0 and fits_0 == 0
    assert static >= (114 + 53) * 8 + C.sizeof(_lib.Terrain)      # z, theta and a terrain: the kernel's static arrays


# ---- StepGradients -------------------------------------------------------------------------------------------------------------------------
def test_step_gradients_slices_the_nine_blocks():
    nq, nu, nc, nb = 3, 2, 1, 4
    nr, ncols = nq + nc + nb, 2 * nq + nu + 1      # one more column (w1) than the nine blocks need
    T, B = 2, 3
    dz = np.arange(T * B * nr * ncols, dtype=float).reshape(T, B, nr, ncols)
    g = plant.StepGradients(dz=dz, z=np.zeros((T, B, 5)), status=np.ones((T, B), dtype=np.int32), nq=nq, nu=nu, nc=nc, nb=nb)
    rows = {"q3": slice(0, 3), "gamma1": slice(3, 4), "b1": slice(4, 8)}
    cols = {"q1": slice(0, 3), "q2": slice(3, 6), "u1": slice(6, 8)}
    for rn, rs in rows.items():
        for cn, cs in cols.items():
            blk = getattr(g, f"d{rn}_d{cn}")
            assert blk.shape == (T, B, rs.stop - rs.start, cs.stop - cs.start)
            np.testing.assert_array_equal(blk, dz[:, :, rs, cs])
            assert np.shares_memory(blk, dz)
    # entry [r, c] of an entry's block is d z[r] / d theta[c]
    assert g.dq3_dq2[1, 2, 0, 1] == dz[1, 2, 0, 4] and g.db1_du1[0, 1, 3, 0] == dz[0, 1, 7, 6]
    one = dataclasses.replace(g, dz=dz[0], z=g.z[0], status=g.status[0])      # a single step: leading axis (B,)
    assert one.dgamma1_dq1.shape == (B, 1, 3)
    few = dataclasses.replace(g, dz=dz[..., :4])                               # grad_cols = 4: q1 is there, q2 is not
    assert few.dq3_dq1.shape == (T, B, 3, 3)
    with pytest.raises(ValueError):
        few.dq3_dq2


def test_diff_sol_is_off_by_default():
    import inspect
    for fn in (plant.plant_step, plant.rollout, plant.simulate):
        p = inspect.signature(fn).parameters
        assert p["diff_sol"].default is False and p["grad_reg"].default is None and p["grad_cols"].default is None
    assert inspect.signature(plant.sensitivity).parameters["n_cols"].default is None


# ---- the Julia binding ---------------------------------------------------------------------------------------------------------------------
JL_COMPAT = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*"},
             "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"}}


@pytest.mark.parametrize("fn_name,symbol", [("plant_sensitivity", "cimpc_plant_sensitivity"), ("plant_rollout", "cimpc_plant_rollout_grad")])
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
    assert "_plant_dims(model)" in fn and not re.search(r"zeros\(\s*(Cint\s*,\s*)?\d", fn)
    if fn_name == "plant_rollout":
        assert "diff_sol::Bool = false" in fn and "kappa_tol * o[].gamma_reg" in fn
