"""hopper_3D (src/dynamics/hopper_3D/model.jl) on the CPU: the residual of csrc/plant_model.h built with g++ against the NumPy
restatement (tests/hopper_3d_ref.py) and the torch model (lcp_models.Hopper3D); the rotation convention pinned by the reference's
own gait files (tests/golden/gaits/hopper_3D_gait_*.jld2); the tables that name the model."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import gait_io, lcp_models, plant, terrain
import hopper_3d_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GAIT = lambda name: os.path.join(HERE, "golden", "gaits", f"hopper_3D_{name}.jld2")


@functools.lru_cache(maxsize=None)
def _gait(name):
    return gait_io.load_joint_traj(GAIT(name))


def _random_point(seed):
    """z, θ with every slack positive, |p| up to 0.5 at q1 and q2, leg length and height of a hopper."""
    rng = np.random.default_rng(seed)
    z, th = rng.uniform(0.1, 1.0, 19), rng.uniform(0.1, 1.0, 22)
    for q in (z[0:7], th[0:7], th[7:14]):
        q[0:2] = rng.uniform(-0.5, 0.5, 2)
        p = rng.normal(size=3)
        q[3:6] = p / np.linalg.norm(p) * rng.uniform(0.0, 0.5)
    th[20], th[21] = 1.5, 0.01
    return z, th


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_header_matches_the_restatements(tmp_path):
    """Residual and dual-number Jacobian of plant_residual / plant_residual_terrain at random points, κ = 1e-3, on flat ground and
    three 3-D terrains: 1e-12 (x max|J| for J) against hopper_3d_ref, whose contact Jacobian is derived another way; the flat case
    also against torch's jacfwd / jacrev through lcp_models.Hopper3D."""
    exe = str(tmp_path / "hopper3d_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "plant_hopper3d_check.cpp")])
    kappa = 1e-3
    m = lcp_models.Hopper3D()
    for seed, name in enumerate(["flat_3D_lc", "sine2_3D_lc", "sine3_3D_lc", "quadratic_bowl_3D_lc", "sine2_3D_lc", "flat_3D_lc"]):
        z, th = _random_point(seed)
        assert max(np.linalg.norm(z[3:6]), np.linalg.norm(th[10:13])) <= 0.5 + 1e-12
        t = terrain.get(name)
        inp = f"{kappa} {t.kind} " + " ".join(repr(float(v)) for v in (*t.p, *z, *th))
        out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
        r_t, J_t, r_f, J_f = (np.array(line.split(), dtype=float) for line in out[:4])
        J_t, J_f = J_t.reshape(19, 19), J_f.reshape(19, 19)
        for P, r, J in ((ref.Hopper3DPlant(None if name == "flat_3D_lc" else name), r_t, J_t), (ref.Hopper3DPlant(), r_f, J_f)):
            np.testing.assert_allclose(r, P.residual(z, th, kappa), rtol=0, atol=1e-12)
            np.testing.assert_allclose(J, P.jacobian_z(z, th), rtol=0, atol=1e-12 * np.abs(J).max())
        r0, rz0, _ = m.linearize(z, th, kappa)
        np.testing.assert_allclose(r_f, r0, rtol=0, atol=1e-12)
        np.testing.assert_allclose(J_f, rz0, rtol=0, atol=1e-12 * np.abs(J_f).max())
        if name == "flat_3D_lc":
            assert np.array_equal(r_t, r_f) and np.array_equal(J_t, J_f)
    # a planar terrain is refused
    t = terrain.get("sine1_2D_lc")
    inp = f"{kappa} {t.kind} " + " ".join(repr(float(v)) for v in (*t.p, *z, *th))
    assert subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.strip() == "invalid"


def _gait_residuals(name, P):
    t = _gait(name)
    return np.abs(np.stack([P.residual(t.z[k], t.theta[k], 0.0) for k in range(t.H)]))


def test_in_place_gait_satisfies_the_residual():
    """test/simulator/hopper_3D.jl asserts |r|_inf < 1e-5 at every knot, κ = 0.  The standard rotation gives 7.6e-10, its transpose
    7.9e-6: the bound 1e-8 is what tells the two apart."""
    r = _gait_residuals("gait_in_place", ref.Hopper3DPlant())
    rt = _gait_residuals("gait_in_place", ref.Hopper3DTransposedPlant())
    print(f"gait_in_place: max |r| = {r.max():.3e} (transposed rotation: {rt.max():.3e})")
    assert r.shape == (92, 19) and r.max() < 1e-8
    assert rt.max() > 1e-8
    m = lcp_models.Hopper3D()
    t = _gait("gait_in_place")
    r0, _, _ = m.linearize_batch(t.z, t.theta, 0.0)
    assert np.abs(r0).max() < 1e-8


def test_forward_gait_pins_the_rotation_convention():
    """gait_forward.jld2 tilts about both axes: dynamics rows 0, 1 (position) and 3, 4 (orientation) hold to 2.0e-6 / 1.7e-5 with
    the standard rotation and to 9.5e-3 / 0.13 with its transpose.  (The slack part of this file's z is stale - |s1 - ϕ| up to
    1.1 - so only the dynamics rows are held.)"""
    r = _gait_residuals("gait_forward", ref.Hopper3DPlant())[:, [0, 1, 3, 4]]
    rt = _gait_residuals("gait_forward", ref.Hopper3DTransposedPlant())[:, [0, 1, 3, 4]]
    print(f"gait_forward rows 0-1 / 3-4: {r[:, :2].max():.3e} / {r[:, 2:].max():.3e} (transposed: {rt[:, :2].max():.3e} / {rt[:, 2:].max():.3e})")
    assert r.max() < 1e-4
    assert rt[:, :2].max() > 1e-3 and rt[:, 2:].max() > 1e-2


def test_model_dims_and_linearization_shapes():
    assert plant.model_dims("hopper_3D") == (10, 7, 3, 1, 4, 3)
    assert plant.SPATIAL_MODELS == {"hopper_3D": (10, 7, 3, 1, 4, 3)} and "hopper_3D" not in plant.MODELS
    m = lcp_models.MODELS["hopper_3D"]()
    assert isinstance(m, lcp_models.Hopper3D) and (m.space, m.nz, m.nth) == (3, 19, 22)
    z, th = _random_point(0)
    r0, rz0, rth0 = m.linearize(z, th, 1e-4)
    assert (r0.shape, rz0.shape, rth0.shape) == ((19,), (19, 19), (19, 22))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_id_10_is_the_hopper_and_id_9_is_unassigned(tmp_path):
    exe = str(tmp_path / "by_id_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "plant_model_by_id_check.cpp")])
    out = subprocess.run([exe, "9", "10", "11"], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [9, 0, 0, 0, 0, 0, 0]
    assert [int(v) for v in out[1].split()] == [10, 1, 7, 3, 1, 4, 3]
    assert [int(v) for v in out[2].split()] == [11, 0, 0, 0, 0, 0, 0]


def test_stride_and_real_problem_tables():
    """get_stride takes x and y (hopper_3D/model.jl:89-93); reference_problem_from_traj yields the tables of both gaits."""
    m = lcp_models.Hopper3D()
    for name, moving in (("gait_in_place", False), ("gait_forward", True)):
        t = _gait(name)
        s = lcp_models.get_stride(m, t.q)
        np.testing.assert_array_equal(s[:2], t.q[-2][:2] - t.q[0][:2])
        assert not s[2:].any() and (abs(s[0]) > 0.05 and abs(s[1]) > 0.05) == moving
        P = lcp_models.reference_problem_from_traj(m, t, 1e-4)
        assert (P.H, P.r0.shape, P.rz0.shape, P.rth0.shape) == (92, (92, 19), (92, 19, 19), (92, 19, 22))
    assert lcp_models.get_stride(lcp_models.Hopper2D(), np.arange(24.0).reshape(6, 4)).tolist() == [16.0, 0.0, 0.0, 0.0]
