"""pushbot (src/dynamics/pushbot/model.jl) and walledcartpole (src/dynamics/walledcartpole/model.jl) on the CPU: the closed forms of
tests/walled_ref.py against the automatic derivatives of lcp_models' Lagrangians, the residual of csrc/plant_model.h built with g++
against both, the real problem tables of examples/pushbot/push_recovery.jl and examples/cartpole/cartpole.jl at their known answer,
the tables that name the models, and the CPU Newton solve that the device step is held to (tests/test_gpu_walled_models.py)."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from contactimplicitmpc.jl_amd import lcp_models, plant
import walled_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODELS = ("pushbot", "walledcartpole")
IDS = {"pushbot": 12, "walledcartpole": 13}
EXAMPLE = {"pushbot": (100, 0.04, 0.5), "walledcartpole": (50, 0.04, 0.35)}       # H, h of the example's reference; ϕ at q = 0


def _random_point(P, seed):
    """z, θ, κ: configurations in [-1, 1], every slack positive, μ in (0.1, 1), h in (0.01, 0.1), κ in (1e-4, 1e-2)."""
    d = P.dims
    rng = np.random.default_rng(seed)
    z, th = rng.uniform(0.1, 1.0, d.nz), rng.uniform(-1.0, 1.0, d.nth)
    z[:d.nq] = rng.uniform(-1.0, 1.0, d.nq)
    th[-2], th[-1] = rng.uniform(0.1, 1.0), rng.uniform(0.01, 0.1)
    return z, th, float(rng.uniform(1e-4, 1e-2))


@pytest.mark.parametrize("name", MODELS)
def test_closed_forms_match_the_lagrangians_derivatives(name):
    """D1L = -C and D2L = M v of walled_ref (closed forms) against torch.func on lcp_models' `lagrangian`: 16 random (q, v), 1e-12."""
    P, m = ref.PLANTS[name](), lcp_models.MODELS[name]()
    rng = np.random.default_rng(IDS[name])
    worst = 0.0
    for _ in range(16):
        q, v = rng.uniform(-1.0, 1.0, P.nq), rng.uniform(-1.0, 1.0, P.nq)
        d1, d2 = P.lagrangian_derivatives(q, v)
        t1, t2 = m.lagrangian_derivatives(torch.as_tensor(q), torch.as_tensor(v))
        worst = max(worst, np.abs(d1 - t1.numpy()).max(), np.abs(d2 - t2.numpy()).max())
        np.testing.assert_allclose(d1, t1.numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(d2, t2.numpy(), rtol=0, atol=1e-12)
    print(f"{name}: closed forms against autodiff, max difference {worst:.2e}")


@pytest.mark.parametrize("name", MODELS)
def test_residual_matches_the_torch_model(name):
    P, m = ref.PLANTS[name](), lcp_models.MODELS[name]()
    assert (m.nq, m.nu, m.nw, m.nc, m.nb, m.nz, m.nth) == (P.nq, P.nu, P.nw, 2, 4, P.dims.nz, P.dims.nth)
    for seed in range(16):
        z, th, kappa = _random_point(P, seed)
        r = m.residual(torch.as_tensor(z), torch.as_tensor(th), torch.tensor(kappa, dtype=torch.float64)).numpy()
        np.testing.assert_allclose(P.residual(z, th, kappa), r, rtol=0, atol=1e-12)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_header_matches_the_restatement(tmp_path):
    """plant_residual_walls on double and its dual-number Jacobian against walled_ref's residual and complex-step Jacobian at the
    points of the test above (the tolerances of tests/test_plant_model_header.py); every terrain but FLAT is refused."""
    exe = str(tmp_path / "walled_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "plant_walled_check.cpp")])
    for name in MODELS:
        P = ref.PLANTS[name]()
        d = P.dims
        for seed in range(16):
            z, th, kappa = _random_point(P, seed)
            inp = f"{IDS[name]} {kappa!r} " + " ".join(repr(float(v)) for v in (*z, *th))
            out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
            assert [int(v) for v in out[0].split()] == [d.nz, d.nth]
            r = np.array(out[1].split(), dtype=float)
            J = np.array(out[2].split(), dtype=float).reshape(d.nz, d.nz)
            np.testing.assert_allclose(r, P.residual(z, th, kappa), rtol=0, atol=1e-12)
            np.testing.assert_allclose(J, P.jacobian_z(z, th), rtol=0, atol=1e-12 * np.abs(J).max())
            assert [int(v) for v in out[3:10]] == [1, 0, 0, 0, 0, 0, 0]


@functools.lru_cache(maxsize=None)
def _problem(name, kappa):
    m = lcp_models.MODELS[name]()
    H, h, _ = EXAMPLE[name]
    return lcp_models.reference_problem(m, lcp_models.constant_reference(m, np.zeros(m.nq), H, h), kappa)


@pytest.mark.parametrize("name", MODELS)
def test_real_tables_at_the_examples_reference(name):
    """The examples' reference holds q = 0 with every force zero: s1 = ϕ(0), the upright pose is an equilibrium (r0[:nq] = 0), every
    other non-bilinear row is 0 and the bilinear rows are -κ; rz0 is the complex-step Jacobian of walled_ref to 1e-9."""
    kappa = 1e-4 if name == "pushbot" else 2e-4
    P, R = _problem(name, kappa), ref.PLANTS[name]()
    m = P.model
    H, h, gap = EXAMPLE[name]
    nq, nc, nb = m.nq, 2, 4
    assert (P.H, P.h, P.z.shape, P.theta.shape, P.r0.shape, P.rz0.shape, P.rth0.shape) == \
        (H, h, (H, m.nz), (H, m.nth), (H, m.nz), (H, m.nz, m.nz), (H, m.nz, m.nth))
    s1 = P.z[:, nq + 2 * nc + nb:nq + 3 * nc + nb]
    assert np.array_equal(s1, np.full((H, 2), gap))
    assert np.array_equal(P.theta[:, -2], np.full(H, m.mu_world)) and np.array_equal(P.theta[:, -1], np.full(H, h))
    nlin = nq + 2 * nc + nb
    assert np.array_equal(P.r0[:, :nlin], np.zeros((H, nlin)))
    assert np.array_equal(P.r0[:, nlin:], np.full((H, m.nz - nlin), -kappa))
    for t in (0, H - 1):
        np.testing.assert_allclose(P.rz0[t], R.jacobian_z(P.z[t], P.theta[t]), rtol=0, atol=1e-9)
    assert not lcp_models.get_stride(m, P.q).any()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ids_and_dimensions_agree_across_header_host_and_julia(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "cimpc.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
    ids = {n.lower(): int(v) for n, v in re.findall(r"#define CIMPC_PLANT_(\w+) (\d+)", hdr)}
    assert {k: ids[k] for k in MODELS} == IDS and 9 not in ids.values() and 11 not in ids.values()
    assert plant.WALLED_MODELS == {"pushbot": (12, 2, 2, 2, 2, 2), "walledcartpole": (13, 4, 1, 2, 2, 4)}
    t = re.search(r"const PLANT_WALLED_MODELS = Dict\{Symbol,NTuple\{6,Int\}\}\((.*?)\)\n", jl, flags=re.S).group(1)
    assert {k: tuple(int(x) for x in v.split(",")) for k, v in re.findall(r":(\w+) => \(([^)]*)\)", t)} == plant.WALLED_MODELS
    for fn in ("function plant_step(", "function _plant_dims("):
        body = jl[jl.index(fn):]
        assert "haskey(PLANT_WALLED_MODELS, model)" in body[:body.index("\nend\n")], fn
    exe = str(tmp_path / "by_id_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "plant_model_by_id_check.cpp")])
    out = subprocess.run([exe, "11", "12", "13", "14"], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [11, 0, 0, 0, 0, 0, 0]
    assert [int(v) for v in out[3].split()] == [14, 0, 0, 0, 0, 0, 0]
    for line, name in zip(out[1:3], MODELS):
        mid, nq, nu, nc, fd, nw = plant.model_dims(name)
        assert name not in plant.MODELS and [int(v) for v in line.split()] == [mid, 1, nq, nu, nc, fd * nc, nw]
        m = lcp_models.MODELS[name]()
        assert (m.nq, m.nu, m.nc, m.nf, m.nw) == (nq, nu, nc, fd, nw)


@pytest.mark.parametrize("disturbed", [False, True])
@pytest.mark.parametrize("name", MODELS)
def test_cpu_newton_solve_on_the_device_tests_inputs(name, disturbed):
    """The precondition of the device comparison: every one of the 64 states converges and at least 8 end in contact (γ > 1e-3), on
    both walls.  Observed with seed 0: pushbot 8 (undisturbed) and 9 in contact, walledcartpole 10 and 9, each 2 on the left wall; at
    most 13 iterations; the nearest γ on either side of the threshold are 5e-10 and 2.6e-2."""
    st, q2, gam, b, it = ref.cpu_step_case(name, disturbed)
    touching = gam > 1e-3
    print(f"{name} (w {'on' if disturbed else 'off'}): converged {st.sum()} / 64, in contact {touching.any(axis=1).sum()} "
          f"(left {touching[:, 0].sum()}, right {touching[:, 1].sum()}), iterations max {it.max()}")
    assert st.all() and len(st) == 64
    assert touching.any(axis=1).sum() >= 8
    assert touching[:, 0].any() and touching[:, 1].any()
