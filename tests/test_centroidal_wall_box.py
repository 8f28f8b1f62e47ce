"""centroidal_quadruped_box and centroidal_quadruped_wall on the CPU: the header residual (plant_residual_centroidal_env,
built with g++ by tests/native/plant_wall_box_check.cpp) against the NumPy restatement of tests/centroidal_wall_box_ref.py,
the shipped gaits against the restated dynamics, the lcp_models tables against finite differences, and the model ids.
The gaits are the reference's examples/centroidal_quadruped/reference/wall_stand_FL_4.jld2 and
examples/centroidal_quadruped_box/reference/step_over_box_v0.jld2, copied unchanged into tests/golden/gaits/."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from contactimplicitmpc.jl_amd import gait_io, lcp_models, plant
import centroidal_wall_box_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GAITS = {"centroidal_quadruped_wall": os.path.join(HERE, "golden", "gaits", "wall_stand_FL_4.jld2"),
         "centroidal_quadruped_box": os.path.join(HERE, "golden", "gaits", "step_over_box_v0.jld2")}
IDS = {"centroidal_quadruped_box": 7, "centroidal_quadruped_wall": 8}
# knots the trajectory optimiser solved; the files pad them with held copies of the first and last knot (the wall:
# stand_wall_FL.jl:276-283, N_first = 10, N_last = 20), which no model satisfies
SOLVED = {"centroidal_quadruped_wall": range(10, 30), "centroidal_quadruped_box": range(0, 49)}


def _points(name, n_random=3):
    """(z, θ) at random points and at three knots of the gait (z and θ as reference_problem packs them)."""
    m = lcp_models.MODELS[name]()
    rng = np.random.default_rng(IDS[name])
    pts = [(rng.uniform(0.1, 1.0, m.nz), rng.uniform(0.1, 1.0, m.nth)) for _ in range(n_random)]
    if name == "centroidal_quadruped_box":                     # feet on and around the step edge (x near 0.25)
        for z, _ in pts:
            z[6:18:3] = rng.uniform(0.2, 0.3, 4)
    g = gait_io.load_gait(GAITS[name])
    for t in (SOLVED[name][0], SOLVED[name][len(SOLVED[name]) // 2], g.H - 1):
        pts.append((m.pack_z(g.q[t + 2], g.gamma[t], g.b[t], g.psi[t], g.eta[t]),
                    m.pack_theta(g.q[t], g.q[t + 1], g.u[t], rng.uniform(-1, 1, 3), g.mu, g.h)))
    return pts


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("wb") / "plant_wall_box_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "plant_wall_box_check.cpp")])
    return lambda inp: subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")


@pytest.mark.parametrize("name", sorted(IDS))
def test_header_residual_and_jacobian_match_the_restatement(check_exe, name):
    P = ref.PLANTS[name]()
    d = P.dims
    for z, th in _points(name):
        kappa = 1e-3
        out = check_exe(f"{IDS[name]} {kappa} " + " ".join(repr(float(v)) for v in np.concatenate([z, th])))
        assert [int(v) for v in out[0].split()] == [d.nz, d.nth]
        r = np.array(out[1].split(), dtype=float)
        J = np.array(out[2].split(), dtype=float).reshape(d.nz, d.nz)
        np.testing.assert_allclose(r, P.residual(z, th, kappa), rtol=0, atol=1e-12)
        np.testing.assert_allclose(J, P.jacobian_z(z, th), rtol=0, atol=1e-12 * max(1.0, np.abs(J).max()))


def test_box_far_from_the_step_is_the_centroidal_residual_bit_for_bit(check_exe):
    """Every foot at x < 0.05: tanh(200 (x - 0.25)) rounds to -1, so e = e' = 0 exactly and the box residual and Jacobian are
    those of plant_residual on the centroidal model with the box's 0.5 kg feet, bit for bit."""
    rng = np.random.default_rng(3)
    P = ref.BoxPlant()
    for _ in range(3):
        z, th = rng.uniform(0.1, 1.0, P.dims.nz), rng.uniform(0.1, 1.0, P.dims.nth)
        z[6:18:3] = rng.uniform(-0.4, 0.049, 4)
        out = check_exe("7 1e-3 " + " ".join(repr(float(v)) for v in np.concatenate([z, th])))
        assert out[1] == out[3] and out[2] == out[4]


def test_wall_residual_is_the_lcp_model_residual():
    """The torch residual of lcp_models (what reference_problem differentiates) equals the NumPy restatement."""
    for name in IDS:
        m, P = lcp_models.MODELS[name](), ref.PLANTS[name]()
        for z, th in _points(name):
            r = m.residual(torch.as_tensor(z), torch.as_tensor(th), torch.tensor(1e-3, dtype=torch.float64)).numpy()
            np.testing.assert_allclose(r, P.residual(z, th, 1e-3), rtol=0, atol=1e-12)


def _dyn_max(model, g, knots):
    out = []
    for t in knots:
        z = model.pack_z(g.q[t + 2], g.gamma[t], g.b[t], g.psi[t], g.eta[t])
        th = model.pack_theta(g.q[t], g.q[t + 1], g.u[t], np.zeros(model.nw), g.mu, g.h)
        r = model.residual(torch.as_tensor(z), torch.as_tensor(th), torch.tensor(0.0, dtype=torch.float64)).numpy()
        out.append(np.abs(r[:model.nq]).max())
    return np.array(out)


class _Undamped:
    def joint_friction(self):
        return torch.zeros(18, dtype=torch.float64)


def test_gaits_satisfy_the_restated_dynamics():
    """Measured: the wall gait's solved knots satisfy the DAMPED wall model to 1.5e-7 (undamped: 0.99); the box gait's satisfy
    the UNDAMPED box model to 1.8e-5 (damped: 0.14) - the box gait was produced without the joint damping its model file
    defines, like centroidal_inplace_trot_v7.  The held padding knots satisfy neither."""
    gw, gb = gait_io.load_gait(GAITS["centroidal_quadruped_wall"]), gait_io.load_gait(GAITS["centroidal_quadruped_box"])
    assert (gw.H, gw.q.shape, gw.gamma.shape, gw.b.shape) == (50, (52, 18), (50, 8), (50, 32))
    assert (gb.H, gb.q.shape, gb.gamma.shape, gb.b.shape) == (99, (101, 18), (99, 4), (99, 16))
    W, Wu = lcp_models.CentroidalQuadrupedWall(), type("WU", (_Undamped, lcp_models.CentroidalQuadrupedWall), {})()
    Bx, Bu = lcp_models.CentroidalQuadrupedBox(), type("BU", (_Undamped, lcp_models.CentroidalQuadrupedBox), {})()
    kw, kb = SOLVED["centroidal_quadruped_wall"], SOLVED["centroidal_quadruped_box"]
    assert _dyn_max(W, gw, kw).max() < 2e-7
    assert _dyn_max(Wu, gw, kw).max() > 0.1
    assert _dyn_max(Bu, gb, kb).max() < 2e-5
    assert _dyn_max(Bx, gb, kb).max() > 0.1
    assert _dyn_max(W, gw, range(0, 10)).min() > 0.1 and _dyn_max(Bu, gb, range(49, 99)).min() > 0.1


@pytest.mark.parametrize("name", sorted(IDS))
def test_lcp_model_tables_match_finite_differences(name):
    m = lcp_models.MODELS[name]()
    g = gait_io.load_gait(GAITS[name])
    P = lcp_models.reference_problem(m, g, 1e-3)
    assert P.r0.shape == (g.H, m.nz) and P.rz0.shape == (g.H, m.nz, m.nz) and P.rth0.shape == (g.H, m.nz, m.nth)
    t = SOLVED[name][3]
    z, th = P.z[t], P.theta[t]
    f = lambda zz, tt: m.residual(torch.as_tensor(zz), torch.as_tensor(tt), torch.tensor(1e-3, dtype=torch.float64)).numpy()
    np.testing.assert_allclose(P.r0[t], f(z, th), rtol=0, atol=1e-14)
    eps = 1e-6
    Jz = np.stack([(f(z + eps * e, th) - f(z - eps * e, th)) / (2 * eps) for e in np.eye(m.nz)], 1)
    Jt = np.stack([(f(z, th + eps * e) - f(z, th - eps * e)) / (2 * eps) for e in np.eye(m.nth)], 1)
    assert np.abs(Jz - P.rz0[t]).max() < 1e-6 * max(1.0, np.abs(P.rz0[t]).max())
    assert np.abs(Jt - P.rth0[t]).max() < 1e-6 * max(1.0, np.abs(P.rth0[t]).max())


def test_model_ids_agree_across_header_host_and_julia():
    hdr = open(os.path.join(ROOT, "include", "cimpc.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
    ids = {n.lower(): int(v) for n, v in re.findall(r"#define CIMPC_PLANT_(\w+) (\d+)", hdr)}
    assert ids["centroidal_box"] == 7 and ids["centroidal_wall"] == 8
    m = re.search(r"const PLANT_ENV_MODELS = Dict\{Symbol,NTuple\{6,Int\}\}\((.*?)\)\n", jl, flags=re.S).group(1)
    table = {k: tuple(int(x) for x in v.split(",")) for k, v in re.findall(r":(\w+) => \(([^)]*)\)", m)}
    assert table == plant.CENTROIDAL_ENV_MODELS
    for name, mid in IDS.items():
        assert plant.model_dims(name)[0] == mid and name not in plant.MODELS
        lm = lcp_models.MODELS[name]()
        _, nq, nu, nc, fd, nw = plant.model_dims(name)
        assert (nq, nu, nc, fd * nc, nw) == (lm.nq, lm.nu, lm.nc, lm.nb, lm.nw)
