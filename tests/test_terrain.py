"""Terrains of the device plant step on the CPU (contactimplicitmpc/jl_amd/terrain.py, the terrain residual of
contactimplicitmpc/jl_amd/csrc/plant_model.h built with g++ by tests/native/plant_terrain_check.cpp), against the NumPy
restatement of tests/terrain_ref.py - the analogue of the reference's test/simulator/environment.jl plus its two terrain
simulator tests (test/simulator/particle.jl)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import plant as pl
import terrain_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLANAR = ("slope1_2D_lc", "slope_smooth_2D_lc", "sine1_2D_lc", "sine2_2D_lc", "sine3_2D_lc", "piecewise1_2D_lc", "piecewise2_2D_lc",
          "stairs3_2D_lc")
SPATIAL = ("sine1_3D_lc", "sine2_3D_lc", "sine3_3D_lc", "quadratic_bowl_3D_lc")


def test_every_reference_environment_has_a_terrain():
    from contactimplicitmpc.jl_amd import terrain
    assert set(terrain.NAMES) == set(terrain_ref.SURFACES)
    with pytest.raises(KeyError):
        terrain.get("circular_bowl_3D_nc")


@pytest.mark.parametrize("name", PLANAR + ("flat_2D_lc",))
def test_planar_surfaces_and_gradients_match_the_formulas(name):
    from contactimplicitmpc.jl_amd import terrain
    T = terrain.get(name)
    s, g, _ = terrain_ref.SURFACES[name]
    x = np.concatenate([np.linspace(-1.0, 4.0, 1001), [0.4, 0.6, 1.9, 2.1, 0.125, 0.375, 0.625, 0.875]])
    np.testing.assert_allclose(T.surface(x), s(x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(T.gradient(x), g(x), rtol=0, atol=1e-12)
    if name != "stairs3_2D_lc":                      # its surf_grad is zero by definition (stairs.jl:22-24)
        e = 1e-6
        # 1e-6: a difference across a knot of the C1 piecewise table sees the jump of the second derivative (O(e))
        np.testing.assert_allclose(T.gradient(x), (T.surface(x + e) - T.surface(x - e)) / (2 * e), rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", SPATIAL + ("flat_3D_lc",))
def test_spatial_surfaces_and_gradients_match_the_formulas(name):
    from contactimplicitmpc.jl_amd import terrain
    T = terrain.get(name)
    s, g, _ = terrain_ref.SURFACES[name]
    rng = np.random.default_rng(0)
    x, y = rng.uniform(-2.0, 2.0, 500), rng.uniform(-2.0, 2.0, 500)
    np.testing.assert_allclose(T.surface(x, y), s(x, y) + 0.0 * x, rtol=0, atol=1e-13)
    gx, gy = g(x, y)
    G = T.gradient(x, y)
    np.testing.assert_allclose(G[:, 0], gx + 0.0 * x, rtol=0, atol=1e-12)
    np.testing.assert_allclose(G[:, 1], gy + 0.0 * y, rtol=0, atol=1e-12)
    e = 1e-6
    np.testing.assert_allclose(G[:, 0], (T.surface(x + e, y) - T.surface(x - e, y)) / (2 * e), rtol=0, atol=1e-7)
    np.testing.assert_allclose(G[:, 1], (T.surface(x, y + e) - T.surface(x, y - e)) / (2 * e), rtol=0, atol=1e-7)


def test_softplus_is_overflow_safe_and_equal_where_the_reference_is_finite():
    from contactimplicitmpc.jl_amd import terrain
    T = terrain.get("slope_smooth_2D_lc")
    with np.errstate(over="ignore"):
        x = np.array([20.0, 50.0, 1e3])
        assert np.all(np.isfinite(T.surface(x))) and np.all(np.isfinite(T.gradient(x)))
        np.testing.assert_allclose(T.surface(x), math.tan(math.radians(10.0)) * (x - 0.5), rtol=1e-15)
        np.testing.assert_allclose(T.surface(20.0), terrain_ref.SURFACES["slope_smooth_2D_lc"][0](20.0), rtol=1e-14)


@pytest.mark.parametrize("deg", [10.0, -10.0])
def test_piecewise_blends_are_c1_at_their_knots(deg):
    """generate_piecewise_terrain's @asserts (piecewise.jl:44-45, 62-63) and slope continuity at every knot of the table."""
    from contactimplicitmpc.jl_amd import terrain
    m = math.tan(math.radians(deg))
    a1, a2 = terrain.piecewise_blends(m)
    assert abs(terrain._poly(a1, 0.4)) < 1e-8 and abs(terrain._poly(a1, 0.6) - m * 0.1) < 1e-8
    assert abs(terrain._poly(a2, 1.4) - m * 1.4) < 1e-8 and abs(terrain._poly(a2, 1.6) - (1.5 * m - 0.025 * m)) < 1e-8
    assert abs(terrain._d_poly(a1, 0.4)) < 1e-8 and abs(terrain._d_poly(a1, 0.6) - m) < 1e-8
    assert abs(terrain._d_poly(a2, 1.4) - m) < 1e-8 and abs(terrain._d_poly(a2, 1.6) + 0.25 * m) < 1e-8
    T = terrain.get("piecewise1_2D_lc" if deg > 0 else "piecewise2_2D_lc")
    for k in (0.4, 0.6, 1.9, 2.1):
        e = 1e-12
        assert abs(T.surface(k - e) - T.surface(k)) < 1e-10
        assert abs(T.gradient(k - e) - T.gradient(k)) < 1e-9


def test_rotations_are_the_reference_rotations():
    for g in (-2.0, -0.3, 0.0, 0.17, 1.5):
        np.testing.assert_allclose(terrain_ref.rotation_2d(np.array(g)), terrain_ref.rotation_2d_atan(g), rtol=0, atol=1e-15)
        R = terrain_ref.rotation_2d(np.array(g))
        n = np.array([-g, 1.0]) / math.hypot(g, 1.0)
        np.testing.assert_allclose(R @ n, [0.0, 1.0], atol=1e-15)                  # world -> surface frame
    for gx, gy in ((0.0, 0.0), (0.3, -0.7), (-1.2, 0.4)):
        R = terrain_ref.rotation_3d(np.array(gx), np.array(gy))
        n = np.array([-gx, -gy, 1.0]) / math.sqrt(1 + gx * gx + gy * gy)
        np.testing.assert_allclose(R @ n, [0.0, 0.0, 1.0], atol=1e-15)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-15)


def _encode(T):
    c = T.to_c()
    head = [str(c.kind), str(c.n_pieces)]
    vals = list(c.p) + list(c.brk) + list(c.off) + [c.coef[i][k] for i in range(len(c.coef)) for k in range(4)]
    return " ".join(head + [repr(float(v)) for v in vals])


MODELS = {"quadruped": (0, PLANAR), "flamingo": (1, PLANAR), "hopper_2D": (2, PLANAR), "particle_2D": (6, PLANAR + ("flat_2D_lc",)),
          "particle": (5, SPATIAL)}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_terrain_residual_of_the_header_matches_the_restatement(tmp_path):
    """plant_residual_terrain and its dual-number Jacobian against terrain_ref (complex step) for every model that takes terrain
    and every surface, to 1e-12; on flat ground the terrain residual is the flat plant_residual bit for bit."""
    from contactimplicitmpc.jl_amd import terrain
    exe = str(tmp_path / "terrain_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "plant_terrain_check.cpp")])
    run = lambda inp: subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    for model, (mid, names) in MODELS.items():
        for name in names:
            P = terrain_ref.plant(model, name)
            d = P.dims
            rng = np.random.default_rng(mid)
            z, th, kappa = rng.uniform(0.1, 1.0, d.nz), rng.uniform(0.1, 1.0, d.nth), 1e-3
            z[0] = rng.uniform(-0.5, 2.5) if model != "particle" else rng.uniform(-1.0, 1.0)
            out = run(f"{mid} {kappa} {_encode(terrain.get(name))} " + " ".join(repr(float(v)) for v in np.concatenate([z, th])))
            assert [int(v) for v in out[0].split()] == [d.nz, d.nth]
            r = np.array(out[1].split(), dtype=float)
            J = np.array(out[2].split(), dtype=float).reshape(d.nz, d.nz)
            np.testing.assert_allclose(r, P.residual(z, th, kappa), rtol=0, atol=1e-12, err_msg=f"{model} {name}")
            np.testing.assert_allclose(J, P.jacobian_z(z, th), rtol=0, atol=1e-12 * max(1.0, np.abs(J).max()), err_msg=f"{model} {name}")
    for mid, P, flat in ((0, pl.QuadrupedPlant(), "flat_2D_lc"), (1, pl.FlamingoPlant(), "flat_2D_lc"), (2, pl.HopperPlant(), "flat_2D_lc"),
                         (5, pl.ParticlePlant(), "flat_3D_lc")):
        d = P.dims
        rng = np.random.default_rng(10 + mid)
        z, th = rng.uniform(0.1, 1.0, d.nz), rng.uniform(0.1, 1.0, d.nth)
        out = run(f"{mid} 1e-3 {_encode(terrain.get(flat))} " + " ".join(repr(float(v)) for v in np.concatenate([z, th])))
        assert out[1] == out[3] and out[2] == out[4], f"model {mid}: flat terrain residual differs from plant_residual"
    # models a terrain does not apply to
    for mid, name in ((3, "sine1_2D_lc"), (0, "quadratic_bowl_3D_lc"), (5, "sine1_2D_lc")):
        assert run(f"{mid} 1e-3 {_encode(terrain.get(name))}")[0] == "invalid"


def test_terrain_layout_matches_the_header(tmp_path):
    from contactimplicitmpc.jl_amd import _lib
    py = _lib.Terrain
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cimpc.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cimpc_terrain));']
    lines += [f'  printf("{f} %zu\\n", offsetof(cimpc_terrain, {f}));' for f, _ in py._fields_]
    lines += ['  printf("max %d\\n", CIMPC_TERRAIN_MAX_PIECES);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(py) and int(got["max"]) == _lib.MAX_TERRAIN_PIECES
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f


def test_reference_particle_in_quadratic_bowl_on_the_cpu_restatement():
    """test/simulator/particle.jl:129-155 (quadratic_bowl_3D_lc, μ 0.1, h 0.01, T 1000, q1 (1, 0.5, 2), v1 (0.1, 0, 0))."""
    ok, q, *_ = pl.simulate(terrain_ref.plant("particle", "quadratic_bowl_3D_lc"), lambda qq, t: np.zeros(3), np.array([1.0, 0.5, 2.0]),
                            np.array([0.1, 0.0, 0.0]), 1000, 0.01, mu=0.1)
    assert ok
    assert abs(q[-1][0]) < 0.05 and abs(q[-1][1]) < 0.05 and abs(q[-1][2]) < 1e-3


def test_reference_particle_2d_on_slope_on_the_cpu_restatement():
    """test/simulator/particle.jl:246-268 (particle_2D on slope1_2D_lc, μ 0.1, h 0.01, T 100, q1 (0, 1))."""
    ok, q, *_ = pl.simulate(terrain_ref.plant("particle_2D", "slope1_2D_lc"), lambda qq, t: np.zeros(2), np.array([0.0, 1.0]),
                            np.zeros(2), 100, 0.01, mu=0.1)
    assert ok and q[-1][0] < 0.0 and q[-1][1] < 0.0
