"""Step gradients on the device (csrc/plant_sensitivity.hip: `plant.sensitivity`, `diff_sol=True` on `plant_step` and `rollout`) against
the longdouble solve of the same definition (tests/plant_gradient_cases.py):

    dz = -R(z, θ; reg)⁻¹ ∂r/∂θ[:, :n_cols],   rows [q2; γ; b].

Bound, per entry (one knot's or one step's whole block): max|dev - ld| / max|ld| <= 100 x max(d_lapack, d_order, 2.2e-16), where
d_lapack is `numpy.linalg.solve`'s own distance to the longdouble solve and d_order that of a float64 restatement of the kernel's
elimination order - never a figure of the device.  No case and no step is left out, and a step whose float64 references are
themselves further than 1e-6 from the longdouble solve fails.

Measured on one MI355X (scripts/plant_gradients_ab.py, profiles/plant_gradients.json).  Synthetic knots (eleven flat models, six
terrain cases, reg 0 and 1e-9, all columns): device <= 1.1e-13, at most 0.05 of its bound; references <= 3.4e-14.  Rollouts, worst step:
hopper_2D 4.9e-14 (LAPACK up to 4.6e-8 off, cond 8.8e11), particle 3.6e-14, quadruped 1.7e-14 (LAPACK 6.6e-9, cond 1.9e12),
centroidal_quadruped_wall 3.2e-8 (d_order 3.2e-8, LAPACK 2.9e-8; bound 3.2e-6).  Cost of `rollout(diff_sol=True)` against the parent
build's `rollout()`: 1.056 x (quadruped, B = 256, T = 100), 1.116 x (centroidal_quadruped, B = 64, T = 60); the composition of
rollout + `plant.linearize` + host solve takes 1.49 x and 2.31 x the fused call.
"""
import dataclasses

import numpy as np
import pytest

import plant_gradient_cases as pgc
import plant_linearize_cases as plc

pytestmark = pytest.mark.gpu


def _check(what, dev, ref):
    """One entry against its references: print the figures, then hold the references to their limit and the device to its bound."""
    d = pgc.rel(dev, ref["ld"])
    print(f"{what}: device {d:.2e} (bound {ref['bound']:.2e}; d_lapack {ref['d_lapack']:.2e}, d_order {ref['d_order']:.2e}, cond R {ref['cond']:.1e})")
    assert max(ref["d_lapack"], ref["d_order"]) <= pgc.REF_LIMIT, f"{what}: the float64 references are themselves off"
    assert d <= ref["bound"], f"{what}: {d:.3e} > {ref['bound']:.3e}"
    return d


# ---- 1. the kernel alone at synthetic knots ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", pgc.REGS)
@pytest.mark.parametrize("name,mid", pgc.FLAT_CASES)
def test_sensitivity_matches_the_longdouble_solve_on_flat_ground(name, mid, reg):
    """N = 3 seeded knots, every column of θ.  nz = 12 (hopper_2D), 15, 18 and 20 (the walled models), 19, 43, 39, 66 (one past a
    wavefront of pivot rows) and 114 (the largest LDS)."""
    from contactimplicitmpc.jl_amd import plant
    z, th, refs = pgc.flat_case(mid, reg)
    dz, st = plant.sensitivity(name, z, th, reg, n_cols=th.shape[1])
    nr = pgc.dims(name)[7]
    assert dz.shape == (pgc.N_KNOTS, nr, th.shape[1]) and st.tolist() == [1] * pgc.N_KNOTS
    for k in range(pgc.N_KNOTS):
        _check(f"{name} reg={reg:g} knot {k}", dz[k], refs[k])


@pytest.mark.parametrize("reg", pgc.REGS)
@pytest.mark.parametrize("model,mid,terrain", plc.TERRAIN_CASES)
def test_sensitivity_matches_the_longdouble_solve_on_terrain(model, mid, terrain, reg):
    """The six terrain cases of the linearization tests, references from the complex step of the NumPy restatements."""
    from contactimplicitmpc.jl_amd import plant
    z, th, refs = pgc.terrain_case(model, mid, terrain, reg)
    dz, st = plant.sensitivity(model, z, th, reg, n_cols=th.shape[1], terrain=terrain)
    assert st.tolist() == [1] * pgc.N_KNOTS
    for k in range(pgc.N_KNOTS):
        _check(f"{model} on {terrain} reg={reg:g} knot {k}", dz[k], refs[k])


def test_fewer_columns_are_the_leading_columns():
    from contactimplicitmpc.jl_amd import plant
    z, th, _ = pgc.flat_case(3, pgc.REG)
    full, _ = plant.sensitivity("centroidal_quadruped", z, th, pgc.REG, n_cols=th.shape[1])
    for n_cols in (1, 7, None):
        part, st = plant.sensitivity("centroidal_quadruped", z, th, pgc.REG, n_cols=n_cols)
        assert st.all() and part.shape[2] == (48 if n_cols is None else n_cols)
        np.testing.assert_array_equal(part, full[:, :, :part.shape[2]])
    one, st1 = plant.sensitivity("centroidal_quadruped", z[1], th[1], pgc.REG, n_cols=th.shape[1])      # a single knot, unbatched
    assert st1 == 1
    np.testing.assert_array_equal(one, full[1])


# ---- 2. rollout gradients at the device's own z ----------------------------------------------------------------------------------------------
def _rollout(c, **kw):
    from contactimplicitmpc.jl_amd import plant
    return plant.rollout(c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"], terrain=c["terrain"], **kw)


def _thetas(c, q, u_applied):
    T, B = u_applied.shape[:2]
    return np.array([[pgc.step_theta(c, q, u_applied, t, b) for b in range(B)] for t in range(T)])


@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_rollout_gradients_match_the_longdouble_solve_at_the_devices_z(which):
    """Every (t, b) of the case against the longdouble reference built from the z the device returned and the θ of that step."""
    c = pgc.rollout_case(which)
    ok, q, ua, gam, b, st, it, G = _rollout(c, diff_sol=True)
    T, B = st.shape
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(c["model"])
    assert ok and G.status.tolist() == [[1] * B] * T and G.dz.shape == (T, B, nr, 2 * nq + nu) and G.z.shape == (T, B, nz)
    refs = pgc.rollout_references(c, G.z, _thetas(c, q, ua), pgc.REG, 2 * nq + nu)
    worst = 0.0
    for t in range(T):
        for r in range(B):
            worst = max(worst, _check(f"{which} t={t} b={r} (max gamma {gam[t, r].max():.3g})", G.dz[t, r], refs[t, r]))
    print(f"{which}: worst device distance {worst:.2e}")
    if which == "hopper_2D":
        assert (gam < 1e-6).any() and (gam > 1.0).any()      # the case is what it is meant to be on the device too


# ---- 3. identities, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hopper_2D", "particle"])
def test_diff_sol_changes_nothing_else_and_is_the_kernel_at_the_steps_z(which):
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case(which)
    plain = _rollout(c)
    *same, G = _rollout(c, diff_sol=True)
    assert len(plain) == 7 and len(same) == 7
    for a, w in zip(same[1:], plain[1:]):
        np.testing.assert_array_equal(a, w)
    ok, q, ua, gam, b, st, it = plain
    T, B = st.shape
    nq, nu, nc, nb = pgc.dims(c["model"])[:4]
    np.testing.assert_array_equal(G.z[:, :, :nq], q[2:])
    np.testing.assert_array_equal(G.z[:, :, nq:nq + nc], gam)
    np.testing.assert_array_equal(G.z[:, :, nq + nc:nq + nc + nb], b)
    # each dz[t, b] is plant.sensitivity on (z[t, b], θ[t, b])
    TH = _thetas(c, q, ua)
    ter = None if c["terrain"] is None else [c["terrain"]] * (T * B)
    dz, s = plant.sensitivity(c["model"], G.z.reshape(T * B, -1), TH.reshape(T * B, -1), pgc.REG, terrain=ter)
    assert s.all()
    np.testing.assert_array_equal(dz.reshape(G.dz.shape), G.dz)
    # every column of θ: the nine blocks are its leading columns
    *_, Gall = _rollout(c, diff_sol=True, grad_cols=TH.shape[2])
    np.testing.assert_array_equal(Gall.dz[..., :2 * nq + nu], G.dz)
    # robot b of the batch is its single-robot call
    for r in range(B):
        one = dict(c, q1=c["q1"][r:r + 1], v1=c["v1"][r:r + 1], u=c["u"][:, r:r + 1] if c["u"].shape[1] > 1 else c["u"], mu=c["mu"][r:r + 1])
        *_, G1 = _rollout(one, diff_sol=True)
        np.testing.assert_array_equal(G1.dz[:, 0], G.dz[:, r])
        np.testing.assert_array_equal(G1.z[:, 0], G.z[:, r])
    # a chunked rollout is the one-launch rollout
    *chunked, Gc = _rollout(c, diff_sol=True, steps_per_launch=1)
    for a, w in zip(chunked[1:], plain[1:]):
        np.testing.assert_array_equal(a, w)
    np.testing.assert_array_equal(Gc.dz, G.dz)
    np.testing.assert_array_equal(Gc.z, G.z)
    np.testing.assert_array_equal(Gc.status, G.status)


@pytest.mark.parametrize("which", ["hopper_2D", "particle"])
def test_plant_step_with_diff_sol_is_step_0_of_the_rollout(which):
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case(which)
    ok, q, ua, gam, b, st, it, G = _rollout(c, diff_sol=True)
    B = st.shape[1]
    for r in range(B):      # one friction coefficient per call
        sel = slice(r, r + 1)
        args = (c["model"], q[0, sel], q[1, sel], ua[0, sel], c["mu"][r], c["h"])
        q2, g1, b1, s1, i1, G1 = plant.plant_step(*args, terrain=c["terrain"], diff_sol=True)
        plain = plant.plant_step(*args, terrain=c["terrain"])
        assert len(plain) == 5
        for a, w in zip((q2, g1, b1, s1, i1), plain):
            np.testing.assert_array_equal(a, w)
        np.testing.assert_array_equal(q2, q[2, sel])
        assert G1.dz.shape == (1,) + G.dz.shape[2:] and G1.status.tolist() == [1]
        np.testing.assert_array_equal(G1.dz[0], G.dz[0, r])
        np.testing.assert_array_equal(G1.z[0], G.z[0, r])


def test_simulate_with_diff_sol_stacks_the_steps():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("particle")
    ok, q, ua, gam, b, st, it, G = _rollout(c, diff_sol=True)
    step = iter(range(c["T"]))

    def policy(q1):
        return ua[next(step)]
    out = plant.simulate(c["model"], policy, c["q1"], c["v1"], c["T"], c["h"], float(c["mu"][0]), terrain=c["terrain"], diff_sol=True)
    assert len(out) == 6
    np.testing.assert_array_equal(out[1], q)
    np.testing.assert_array_equal(out[5].dz, G.dz)
    np.testing.assert_array_equal(out[5].status, G.status)


# ---- 4. a known answer ---------------------------------------------------------------------------------------------------------------------
def test_particle_in_free_flight():
    """At 1 m with u = w = 0 the step is q3 = 2 q2 - q1 + h² g: dq3/dq2 = 2I, dq3/dq1 = -I.  The only deviation is through the idle contact,
    γ ~ κ/ϕ and reg, both <= 1e-8 in size; γ1 does not move."""
    from contactimplicitmpc.jl_amd import plant
    q1 = np.array([[0.1, -0.2, 1.0]])
    q2, g, b, st, it, G = plant.plant_step("particle", q1 - 0.01 * np.array([[0.3, 0.1, 0.0]]), q1, np.zeros((1, 3)), 0.5, 0.01, diff_sol=True)
    assert st.all() and G.status.all() and g.max() < 1e-7
    for name, want in (("dq3_dq2", 2.0 * np.eye(3)), ("dq3_dq1", -np.eye(3)), ("dgamma1_dq1", 0.0), ("dgamma1_dq2", 0.0), ("dgamma1_du1", 0.0)):
        got = getattr(G, name)[0]
        print(f"{name}: max deviation {np.abs(got - want).max():.3e}")
        np.testing.assert_allclose(got, np.broadcast_to(want, got.shape), rtol=0, atol=1e-6)
    np.testing.assert_allclose(G.dq3_du1[0], np.eye(3) * 0.01, rtol=0, atol=1e-6)      # dq3/du1 = h/m I (h = 0.01, m = 1; u1 an impulse)


# ---- 5. reg is honoured ----------------------------------------------------------------------------------------------------------------------
def test_reg_is_honoured():
    """Knots with an idle pair (γ = 1e-12 at knot 0, s2 = 1e-5 at knot 1): reg = 1e-9 and reg = 1e-3 give different blocks, each its own
    longdouble reference's."""
    from contactimplicitmpc.jl_amd import plant
    name, (nq, nu, nc, nb, nw, nz, nth, nr) = "hopper_2D", pgc.dims("hopper_2D")
    z, th, _ = pgc.flat_case(2, pgc.REG)
    z = z.copy()
    z[0, nq] = 1e-12
    z[1, nz - 1] = 1e-5
    out = {}
    for reg in (1e-9, 1e-3):
        dz, st = plant.sensitivity(name, z, th, reg, n_cols=nth)
        assert st.all()
        for k in range(pgc.N_KNOTS):
            _check(f"reg={reg:g} knot {k}", dz[k], pgc.knot_references(name, None, z[k], th[k], reg, nth))
        out[reg] = dz
    for k in (0, 1):      # the longdouble references differ by 2.8e-2 (of 9.6) and 3.0e-4 (of 4.6) there
        assert np.abs(out[1e-9][k] - out[1e-3][k]).max() > 1e-5 * np.abs(out[1e-9][k]).max()
    np.testing.assert_array_equal(out[1e-9][2], out[1e-3][2])      # no pair of knot 2 is under either reg


# ---- 6. and 7. status 0 ------------------------------------------------------------------------------------------------------------------------
def test_an_unconverged_step_has_zero_gradients_and_loses_nothing_else():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    good = _rollout(c, diff_sol=True)
    ok, q, ua, gam, b, st, it, G = _rollout(c, diff_sol=True, opts=dataclasses.replace(plant.SIM_OPTS, max_iter=1))      # returns: the call itself is OK
    assert not ok and (st == 0).all() and (it == 1).all()
    np.testing.assert_array_equal(G.status, 0)
    np.testing.assert_array_equal(G.dz, 0.0)
    assert np.isfinite(G.z).all()
    again = _rollout(c, diff_sol=True)
    for a, w in zip(again[1:7], good[1:7]):
        np.testing.assert_array_equal(a, w)
    np.testing.assert_array_equal(again[7].dz, good[7].dz)
    assert again[7].status.all()


@pytest.mark.parametrize("damage", ["zero row", "NaN"])
def test_a_singular_knot_is_refused_alone(damage):
    """γ_1 = s1_1 = 0 with reg = 0 makes the first bilinear row of R zero: the last pivot is an exact zero.  A NaN in z reaches a pivot
    or a result.  Either way that knot alone has status 0 and a zero block; its neighbours are what they are without it."""
    from contactimplicitmpc.jl_amd import plant
    name, (nq, nu, nc, nb, nw, nz, nth, nr) = "quadruped", pgc.dims("quadruped")
    z, th, _ = pgc.flat_case(0, 0.0)
    clean, st = plant.sensitivity(name, z, th, 0.0, n_cols=nth)
    assert st.all()
    z = z.copy()
    if damage == "zero row":
        z[1, nq] = z[1, nq + 2 * nc + nb] = 0.0
    else:
        z[1, 3] = np.nan
    dz, st = plant.sensitivity(name, z, th, 0.0, n_cols=nth)
    assert st.tolist() == [1, 0, 1]
    np.testing.assert_array_equal(dz[1], 0.0)
    np.testing.assert_array_equal(dz[[0, 2]], clean[[0, 2]])
    if damage == "zero row":      # the same knot is differentiable as soon as reg > 0
        dz, st = plant.sensitivity(name, z, th, pgc.REG, n_cols=nth)
        assert st.all() and np.isfinite(dz).all()
