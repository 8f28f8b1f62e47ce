"""`cimpc_plant_linearize` without a device: the θ-generic residuals of `contactimplicitmpc/jl_amd/csrc/plant_model.h` built with g++
(tests/native/plant_linearize_check.cpp; also as a sanitized stand-alone program) and evaluated as the kernel evaluates them - r,
dr/dz and dr/dθ against the torch linearization of every model and, on terrain, against the complex-step derivatives of the NumPy
restatements; the z-columns against the (Dual, double) Jacobian of the step kernel, bit for bit; the export, its ctypes signature and
its argument validation (which comes before any device call); the `linearize` keyword of `lcp_models.reference_problem`; the Julia
binding's `plant_linearize` read as text."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, lcp_models, plant
import plant_linearize_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
INVALID, NO_DEVICE = -1, -2


# ---- the header on the host -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("plant_linearize") / "plant_linearize_check")
    # the sanitizer runtimes linked statically: the program then runs the same whatever else the loader brings in
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"] if request.param == "sanitized" else []
    cmd = ["g++", "-O2", "-std=c++17", *flags, "-o", exe, os.path.join(HERE, "native", "plant_linearize_check.cpp")]
    if flags and subprocess.run(cmd, capture_output=True).returncode != 0:
        pytest.skip("this g++ has no static sanitizer runtime")
    subprocess.check_call(cmd)

    def run(mid, z, th, kappa, terrain=None):
        head = f"{mid} {kappa!r} " + ("0" if terrain is None else "1 " + cases.encode_terrain(terrain))
        out = subprocess.run([exe], input=head + " " + " ".join(repr(float(v)) for v in np.concatenate([z, th])), capture_output=True,
                             text=True, check=True).stdout.split("\n")
        if out[0] == "invalid":
            return None
        nz, nth = (int(v) for v in out[0].split())
        assert (nz, nth) == (z.shape[0], th.shape[0])
        a = [np.array(line.split(), dtype=float) for line in out[1:5]]
        return a[0], a[1].reshape(nz, nz), a[2].reshape(nz, nth), a[3].reshape(nz, nz)
    return run


@pytest.mark.parametrize("mid", sorted(cases.TORCH_MODELS))
def test_header_linearization_matches_torch(harness, mid):
    """r, dr/dz and dr/dθ of the (Dual, DualTh) evaluation against `ContactModel.linearize`, and the z-columns against the
    (Dual, double) Jacobian bit for bit."""
    z, th, (r0, rz0, rth0) = cases.torch_case(mid)
    r, Jz, Jth, Jold = harness(mid, z[0], th[0], cases.KAPPA)
    cases.assert_linearization((r, Jz, Jth), (r0[0], rz0[0], rth0[0]), cases.TORCH_MODELS[mid])
    assert np.array_equal(Jz, Jold), f"{cases.TORCH_MODELS[mid]}: dr/dz moves with θ on dual numbers"


def test_the_batched_torch_reference_is_the_single_knot_one():
    """`linearize_batch`, the reference of these tests, against `linearize` knot by knot (one model)."""
    z, th, (r0, rz0, rth0) = cases.torch_case(2)
    for k in range(z.shape[0]):
        cases.assert_linearization((r0[k], rz0[k], rth0[k]), lcp_models.Hopper2D().linearize(z[k], th[k], cases.KAPPA), f"hopper_2D knot {k}")


@pytest.mark.parametrize("model,mid,terrain", cases.TERRAIN_CASES)
def test_header_linearization_on_terrain_matches_the_restatements(harness, model, mid, terrain):
    """One terrain per residual family and particle_2D, against the complex-step derivatives of the restatements (which carry complex
    numbers, so no difference quotient is needed); the z-columns again bit for bit."""
    z, th, ref = cases.terrain_case(model, mid, terrain)
    r, Jz, Jth, Jold = harness(mid, z[0], th[0], cases.KAPPA, terrain)
    cases.assert_linearization((r, Jz, Jth), ref[0], f"{model} on {terrain}")
    assert np.array_equal(Jz, Jold)


def test_header_refuses_what_the_entry_refuses(harness):
    z, th = np.zeros(7), np.ones(10)
    assert harness(6, z, th, 0.0) is None                                   # particle_2D has no flat entry
    assert harness(3, np.zeros(66), np.ones(53), 0.0, "sine1_2D_lc") is None      # the centroidal models take no terrain


# ---- the export -----------------------------------------------------------------------------------------------------------------------
def _prototype():
    m = re.search(r"\bint\s+cimpc_plant_linearize\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, "cimpc_plant_linearize is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


def test_export_is_declared_and_bound():
    params = _prototype()
    res, args = _lib.SIGNATURES["cimpc_plant_linearize"]
    assert res is C.c_int and len(args) == len(params) == 10
    ctype = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "const cimpc_terrain*": C.POINTER(_lib.Terrain)}
    assert [ctype[p] for p in params] == args
    assert hasattr(_lib.load(), "cimpc_plant_linearize")


# validation: hopper_2D (nz 12, nθ 14), N = 2
def _call(**over):
    mid, nq, nu, nc, fd, nw = plant.model_dims(over.pop("model_name", "hopper_2D"))
    nz, nth, N = nq + 4 * nc + 2 * fd * nc, 2 * nq + nu + nw + 2, 2
    a = dict(model=mid, N=N, n_terrain=0, terrain=None, z=np.full((N, nz), 0.5), theta=np.full((N, nth), 0.5), kappa=1e-3, r0=np.zeros((N, nz)),
             rz0=np.zeros((N, nz, nz)), rth0=np.zeros((N, nth, nz)))
    a.update(over)
    arg = lambda v: v.ctypes.data_as(_lib._dp) if isinstance(v, np.ndarray) else v
    return _lib.load().cimpc_plant_linearize(*[arg(a[k]) for k in ("model", "N", "n_terrain", "terrain", "z", "theta", "kappa", "r0", "rz0", "rth0")])


def _terrains(*names):
    from contactimplicitmpc.jl_amd import terrain
    return (_lib.Terrain * len(names))(*[terrain.get(n).to_c() for n in names])


def _theta(h, knot):
    th = np.full((2, 14), 0.5)
    th[knot, -1] = h
    return th


BAD = {
    "unknown model": dict(model=9), "another unknown model": dict(model=11), "negative model": dict(model=-1), "N = 0": dict(N=0), "N < 0": dict(N=-1),
    "null z": dict(z=None), "null theta": dict(theta=None), "no output": dict(r0=None, rz0=None, rth0=None),
    "kappa < 0": dict(kappa=-1e-3), "kappa nan": dict(kappa=float("nan")), "kappa inf": dict(kappa=float("inf")),
    "h = 0 at the first knot": dict(theta=_theta(0.0, 0)), "h < 0 at the last knot": dict(theta=_theta(-0.01, 1)), "h nan": dict(theta=_theta(float("nan"), 1)),
    "particle_2D without a terrain": dict(model_name="particle_2D"),
    "terrain count without terrains": dict(n_terrain=1), "terrains without a count": dict(terrain=_terrains("sine1_2D_lc")),
    "terrain count neither 1 nor N": dict(n_terrain=3, terrain=_terrains("sine1_2D_lc", "sine1_2D_lc", "sine1_2D_lc")),
    "a 3-D terrain under a planar model": dict(n_terrain=1, terrain=_terrains("sine1_3D_lc")),
    "one bad terrain among N": dict(n_terrain=2, terrain=_terrains("sine1_2D_lc", "sine1_3D_lc")),
    "the wall on rough ground": dict(model_name="centroidal_quadruped_wall", n_terrain=1, terrain=_terrains("sine1_3D_lc")),
    "pushbot on rough ground": dict(model_name="pushbot", n_terrain=1, terrain=_terrains("sine1_2D_lc")),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_invalid_arguments_are_refused_without_a_device(what):
    assert _call(**BAD[what]) == INVALID


def test_a_valid_call_needs_a_gfx950():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    assert _call() == NO_DEVICE
    assert _call(rz0=None, rth0=None, kappa=0.0, n_terrain=2, terrain=_terrains("sine1_2D_lc", "flat_2D_lc")) == NO_DEVICE
    with pytest.raises(_lib.CimpcError):
        plant.linearize("hopper_2D", np.full(12, 0.5), np.full(14, 0.5), 1e-3)


def test_host_shapes_are_checked_before_the_library_is_called():
    for z, th in ((np.zeros(11), np.ones(14)), (np.zeros(12), np.ones(12)), (np.zeros((2, 12)), np.ones((3, 14))), (np.zeros((0, 12)), np.ones((0, 14)))):
        with pytest.raises(ValueError):
            plant.linearize("hopper_2D", z, th, 1e-3)
    with pytest.raises(ValueError):
        plant.linearize("hopper_2D", np.zeros((3, 12)), np.ones((3, 14)), 1e-3, terrain=["sine1_2D_lc", "sine1_2D_lc"])
    with pytest.raises(KeyError):
        plant.linearizer("unicycle")


# ---- lcp_models: the keyword ------------------------------------------------------------------------------------------------------------
def test_linearize_keyword_defaults_to_the_torch_path():
    model = lcp_models.PushBot()
    gait = lcp_models.constant_reference(model, [0.1, 0.05], 3, 0.04)
    fields = ("z", "theta", "r0", "rz0", "rth0")
    P0 = lcp_models.reference_problem(model, gait, 1e-4)
    P1 = lcp_models.reference_problem(model, gait, 1e-4, linearize=None)
    for f in fields:
        assert np.array_equal(getattr(P0, f), getattr(P1, f)), f
    seen = []

    def mine(z, th, kappa):
        seen.append((z.copy(), th.copy(), kappa))
        r0, rz0, rth0 = model.linearize_batch(z, th, kappa)
        return r0 + 1.0, rz0, rth0
    P2 = lcp_models.reference_problem(model, gait, 1e-4, linearize=mine)
    assert len(seen) == 1 and np.array_equal(seen[0][0], P0.z) and np.array_equal(seen[0][1], P0.theta) and seen[0][2] == 1e-4
    assert np.array_equal(P2.r0, P0.r0 + 1.0) and np.array_equal(P2.rz0, P0.rz0) and np.array_equal(P2.rth0, P0.rth0)

    class Traj:
        H, h = P0.H, P0.h
        q, u, w, gamma, b, z, theta = P0.q, P0.u, P0.w, P0.gamma, P0.b, P0.z, P0.theta
    Q0 = lcp_models.reference_problem_from_traj(model, Traj, 1e-4)
    Q2 = lcp_models.reference_problem_from_traj(model, Traj, 1e-4, linearize=mine)
    assert np.array_equal(Q0.r0, P0.r0) and np.array_equal(Q2.r0, P0.r0 + 1.0) and len(seen) == 2


# ---- the Julia binding ------------------------------------------------------------------------------------------------------------------
def test_julia_plant_linearize_matches_the_prototype():
    params = _prototype()
    fn = JL[JL.index("function plant_linearize("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\.cimpc_plant_linearize\((.*?)\)::Cint", fn, flags=re.S)
    assert m, "plant_linearize does not call cimpc_plant_linearize"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    compat = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Terrain}": {"const cimpc_terrain*"}}
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in compat[jt], f"argument {k}: Julia {jt} against C `{ct}`"
    assert not re.search(r"zeros\(\s*(Cint\s*,\s*)?\d", fn), "literal array size in plant_linearize"
    assert "_plant_dims(model)" in fn
