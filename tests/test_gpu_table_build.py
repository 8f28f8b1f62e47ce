"""The solver's linearization tables built on the device (`cimpc_linearize_knots`, `cimpc_set_linearization_batch`:
lin_table_build_kernel behind plant_linearize_kernel) against the host path `cimpc_set_linearization`, table by table and bit for
bit (`cimpc_get_table`): every layout family, a range inside the table, terrain, a singular knot, the sweep that consumes the
tables, and re-linearization in flight under `CIMPCPolicy`.  Both paths run one text (csrc/lin_table_build.h), one on the GPU and one
on the CPU; what that text computes is held by the recorded tables of tests/golden/lin_table_sha256.json, which the last test reads
back from a handle.  Handles are small (H_ref <= 6, B = 1, N = 3 knots) except the two policies, which carry the quadruped gait's
60 knots."""
import os

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import CIMPCSolver, InteriorPointOptions, NewtonOptions, _lib, gait_io, lcp_models, plant
from contactimplicitmpc.jl_amd.policy import CIMPCPolicy
import plant_linearize_cases as cases
import table_build_cases

pytestmark = pytest.mark.gpu

GAIT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaits")
# layout family -> (plant model, mode, source of the knots: a gait file, a joint-trajectory file, or the seed of plant_linearize_cases.inputs)
FAMILIES = {
    "quadruped mode 0 (16 lanes, adjoint, Gs by row)": ("quadruped", 0, ("gait", "quadruped_gait2.jld2")),
    "hopper_3D mode 0 (nx > ny)": ("hopper_3D", 0, ("traj", "hopper_3D_gait_in_place.jld2")),
    "centroidal_quadruped mode 0 (32 lanes)": ("centroidal_quadruped", 0, ("gait", "centroidal_inplace_trot_v7.jld2")),
    "pushbot mode 1 (column form)": ("pushbot", 1, ("seed", 12)),         # seed 12: the host path accepts every knot (asserted below)
    "centroidal_quadruped_wall mode 0 (64 lanes)": ("centroidal_quadruped_wall", 0, ("gait", "wall_stand_FL_4.jld2")),
    "centroidal_quadruped_wall mode 1 (run-time dimensions)": ("centroidal_quadruped_wall", 1, ("gait", "wall_stand_FL_4.jld2")),
}
KAPPA = 1e-4


def _knots(name, source, lo=0, n=3):
    model = lcp_models.MODELS[name]()
    kind, what = source
    if kind == "gait":
        P = lcp_models.reference_problem(model, gait_io.load_gait(os.path.join(GAIT_DIR, what)), KAPPA, tables=False)
        z, th = P.z, P.theta
    elif kind == "traj":
        t = gait_io.load_joint_traj(os.path.join(GAIT_DIR, what))
        z, th = t.z, t.theta
    else:
        z, th = cases.inputs(what, model.nz, model.nth, lo + n)
    return model, np.ascontiguousarray(z[lo:lo + n]), np.ascontiguousarray(th[lo:lo + n])


def _handle(model, mode, H_ref, H=None, kappa=KAPPA):
    return CIMPCSolver(model.nq, model.nu, model.nw, model.nc, model.nb, H_ref, H or H_ref, B=1, mode=mode,
                       ip_opts=InteriorPointOptions(kappa_tol=kappa), newton_opts=NewtonOptions(kappa=kappa))


def _host_path(s, t0, z, th, triple):
    r0, rz0, rth0 = triple
    for k in range(z.shape[0]):
        s.set_linearization(t0 + k, z[k], th[k], r0[k], rz0[k], rth0[k])


def _tables(s, knots):
    return [s.get_table(t) for t in knots]


# ---- 1. bit identity across layouts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_device_built_tables_are_the_host_packers_bit_for_bit(family):
    name, mode, source = FAMILIES[family]
    model, z, th = _knots(name, source)
    triple = plant.linearize(name, z, th, KAPPA)
    A, B, Cc = (_handle(model, mode, 3) for _ in range(3))
    try:
        _host_path(A, 1, z, th, triple)               # raises if the host path refuses a knot
        B.linearize_knots(name, z, th, KAPPA)
        Cc.set_linearization_batch(1, z, th, *triple)
        size = A.query_sizes()[0]
        for t in (1, 2, 3):
            a, b, c = A.get_table(t), B.get_table(t), Cc.get_table(t)
            assert a.shape == (size,) and np.isfinite(a).all() and np.count_nonzero(a) > model.nq * model.nq
            assert np.array_equal(a, b), f"{family}: linearize_knots, knot {t}: {np.count_nonzero(a != b)} of {size} entries differ"
            assert np.array_equal(a, c), f"{family}: set_linearization_batch, knot {t}: {np.count_nonzero(a != c)} of {size} entries differ"
    finally:
        for s in (A, B, Cc):
            s.close()


def test_dimensions_whose_workspace_passes_64_kb_of_lds():
    """nx = 40, ny = 56 on the run-time-dimension layout: [Dx | I], CAi and CAiB take 67 KB, past the default limit of a kernel's
    dynamic LDS - the launch that raises it.  Seeded tables with a dominant diagonal in Dx; batch against the host packer."""
    class Dims:
        nq, nu, nw, nc, nb = 40, 2, 2, 8, 40
    A, Cc = _handle(Dims, 0, 3), _handle(Dims, 0, 3)
    try:
        nz, nth, nx = A.nz, A.nth, Dims.nq
        rng = np.random.default_rng(5)
        z, th, r0 = rng.normal(size=(3, nz)), rng.uniform(0.1, 1.0, (3, nth)), rng.normal(size=(3, nz))
        rz0, rth0 = rng.normal(size=(3, nz, nz)), rng.normal(size=(3, nz, nth))
        rz0[:, :nx, :nx] += 4.0 * np.eye(nx)
        _host_path(A, 1, z, th, (r0, rz0, rth0))
        Cc.set_linearization_batch(1, z, th, r0, rz0, rth0)
        for t in (1, 2, 3):
            assert np.array_equal(A.get_table(t), Cc.get_table(t)), f"knot {t}"
    finally:
        A.close(); Cc.close()


# ---- 2. a range inside the table ------------------------------------------------------------------------------------------------------
def test_a_range_inside_the_table_leaves_the_other_knots_alone():
    model, z, th = _knots("quadruped", ("gait", "quadruped_gait2.jld2"), 0, 8)
    triple = plant.linearize("quadruped", z, th, KAPPA)
    A, B = _handle(model, 0, 6), _handle(model, 0, 6)
    try:
        for s in (A, B):
            _host_path(s, 1, z[:6], th[:6], [a[:6] for a in triple])
        before = _tables(B, range(1, 7))
        _host_path(A, 3, z[6:8], th[6:8], [a[6:8] for a in triple])      # knots 3-4 take the gait's knots 7-8
        B.linearize_knots("quadruped", z[6:8], th[6:8], KAPPA, t0=3)
        after, want = _tables(B, range(1, 7)), _tables(A, range(1, 7))
        for k in (0, 1, 4, 5):
            assert np.array_equal(after[k], before[k]), f"knot {k + 1} changed"
        for k in (2, 3):
            assert np.array_equal(after[k], want[k]) and not np.array_equal(after[k], before[k]), f"knot {k + 1}"
        with pytest.raises(_lib.CimpcError):          # past the end of the table: refused by the library as well
            B._check(B.lib.cimpc_linearize_knots(B.h, 0, 6, 2, 0, None, z[6:8].ctypes.data_as(_lib._dp), th[6:8].ctypes.data_as(_lib._dp), KAPPA), "linearize_knots")
        assert all(np.array_equal(a, b) for a, b in zip(_tables(B, range(1, 7)), after))
    finally:
        A.close(); B.close()


# ---- 3. terrain -----------------------------------------------------------------------------------------------------------------------
def test_a_terrain_per_knot():
    names = ["sine1_2D_lc", "piecewise1_2D_lc", "flat_2D_lc"]
    model = lcp_models.Quadruped()
    z, th = cases.inputs(100, 43, 34, 3)
    z[:, 0] = [0.3, 0.55, 1.7]                       # over the sine, inside piecewise1's first blend, anywhere (tests/test_gpu_plant_linearize.py)
    triple = plant.linearize("quadruped", z, th, KAPPA, terrain=names)
    flat = plant.linearize("quadruped", z, th, KAPPA)
    assert not np.array_equal(triple[1][0], flat[1][0])
    A, B = _handle(model, 0, 3), _handle(model, 0, 3)
    try:
        _host_path(A, 1, z, th, triple)
        B.linearize_knots("quadruped", z, th, KAPPA, terrain=names)
        for t in (1, 2, 3):
            assert np.array_equal(A.get_table(t), B.get_table(t)), f"knot {t} on {names[t - 1]}"
        B.linearize_knots("quadruped", z, th, KAPPA, terrain="sine1_2D_lc")          # one terrain shared by the knots
        _host_path(A, 1, z, th, plant.linearize("quadruped", z, th, KAPPA, terrain="sine1_2D_lc"))
        for t in (1, 2, 3):
            assert np.array_equal(A.get_table(t), B.get_table(t)), f"knot {t} on the shared terrain"
    finally:
        A.close(); B.close()


# ---- 4. a singular knot ---------------------------------------------------------------------------------------------------------------
def test_a_singular_knot_fails_the_whole_call_and_changes_nothing():
    model, z, th = _knots("quadruped", ("gait", "quadruped_gait2.jld2"), 0, 6)
    r0, rz0, rth0 = plant.linearize("quadruped", z, th, KAPPA)
    A, Cc = _handle(model, 0, 6), _handle(model, 0, 6)
    try:
        _host_path(A, 1, z, th, (r0, rz0, rth0))
        Cc.set_linearization_batch(1, z, th, r0, rz0, rth0)
        before = _tables(Cc, range(1, 7))
        t0 = 2
        bad = rz0[3:6].copy()                          # the gait's knots 4-6 into knots 2-4, the second one singular
        bad[1][:, 0] = 0.0                             # dr/d q2[0]
        with pytest.raises(_lib.CimpcError) as e:
            Cc.set_linearization_batch(t0, z[3:6], th[3:6], r0[3:6], bad, rth0[3:6])
        assert "(-1)" in str(e.value) and f"knot {t0 + 1}" in str(e.value) and "singular" in str(e.value), str(e.value)
        assert all(np.array_equal(a, b) for a, b in zip(_tables(Cc, range(1, 7)), before)), "a table changed"
        with pytest.raises(_lib.CimpcError, match="singular"):          # the host path refuses the same knot, and only that one
            A.set_linearization(t0 + 1, z[4], th[4], r0[4], bad[1], rth0[4])
        A.set_linearization(t0, z[3], th[3], r0[3], bad[0], rth0[3])
        A.set_linearization(t0 + 2, z[5], th[5], r0[5], bad[2], rth0[5])
    finally:
        A.close(); Cc.close()


# ---- 5. consumed right ----------------------------------------------------------------------------------------------------------------
def test_the_sweep_reads_device_built_tables_as_it_reads_the_host_packers():
    """B3 `implicit_dynamics` on the quadruped gait2 tables at κ = 1e-4, H = 6 (test/controller/implicit_dynamics.jl): the sweep alone,
    every output equal on the three handles."""
    model, z, th = _knots("quadruped", ("gait", "quadruped_gait2.jld2"), 0, 6)
    triple = plant.linearize("quadruped", z, th, KAPPA)
    P = lcp_models.reference_problem(model, gait_io.load_gait(os.path.join(GAIT_DIR, "quadruped_gait2.jld2")), KAPPA, tables=False)
    r = lcp_models.make_rollout(P, 6, 0, seed=0, perturb=1e-3)
    q = r["q"].copy()
    q[0], q[1] = r["q0"], r["q1"]
    theta = r["theta"].copy()
    theta[0, :model.nq], theta[0, model.nq:2 * model.nq], theta[1, :model.nq] = q[0], q[1], q[1]
    window = (np.arange(8) % 6 + 1)[None]
    hs = [_handle(model, 0, 6, kappa=2e-4) for _ in range(3)]
    try:
        _host_path(hs[0], 1, z, th, triple)
        hs[1].linearize_knots("quadruped", z, th, KAPPA)
        hs[2].set_linearization_batch(1, z, th, *triple)
        outs = []
        for s in hs:
            s.set_window(window)
            outs.append(s.implicit_dynamics(q[None], theta[None], want_z=True))
        assert outs[0]["status"].all() and np.abs(outs[0]["d"]).max() < 1e-2
        for o in outs[1:]:
            for k in outs[0]:
                assert np.array_equal(outs[0][k], o[k]), k
    finally:
        for s in hs:
            s.close()


# ---- 6. in flight ---------------------------------------------------------------------------------------------------------------------
def test_relinearization_in_flight_under_the_policy(monkeypatch):
    """Two policies over the quadruped gait (H_mpc 10, N_sample 5, κ_mpc 2e-4), tables from the device and from the host path, on the
    one-ended KKT kernels (reproducible to the bit): three solves (one cold, two warm), four knots re-linearized with θ carrying
    μ_world, two more warm solves - u1 and the Newton iteration counts equal at every solve.  Control: a second host-path policy."""
    for k in ("CIMPC_KKT_DUO", "CIMPC_KKT_TWISTED", "CIMPC_ASYNC_KKT_TW"):
        monkeypatch.setenv(k, "0")
    from oracle import synth
    from oracle.dims import Dims, QUADRUPED
    kappa, H_mpc, N_sample = 2e-4, 10, 5
    model = lcp_models.Quadruped()
    gait = gait_io.load_gait(os.path.join(GAIT_DIR, "quadruped_gait2.jld2"))
    P_host = lcp_models.reference_problem(model, gait, kappa, linearize=plant.linearizer("quadruped"))
    P_dev = lcp_models.reference_problem(model, gait, kappa, tables=False)
    assert P_dev.r0 is None
    obj = synth.make_objective(Dims(**QUADRUPED, mode=0), H_mpc, kind="quadruped")
    kw = dict(H_mpc=H_mpc, N_sample=N_sample, kappa_mpc=kappa, B=1, n_opts=NewtonOptions(kappa=kappa, r_tol=3e-4, max_iter=5),
              ip_opts=InteriorPointOptions(kappa_tol=kappa, r_tol=1e-8))
    with pytest.raises(ValueError, match="device_tables"):
        CIMPCPolicy(P_dev, obj.q, obj.u, **kw)
    pols = [CIMPCPolicy(P_host, obj.q, obj.u, **kw), CIMPCPolicy(P_host, obj.q, obj.u, **kw), CIMPCPolicy(P_dev, obj.q, obj.u, device_tables=True, **kw)]
    try:
        for t in (1, 30, 60):
            assert np.array_equal(pols[0].solver.get_table(t), pols[2].solver.get_table(t)), f"knot {t} at construction"
        rng = np.random.default_rng(0)

        def solve(step):
            q1 = P_host.q[1 + step] + 1e-3 * rng.uniform(-1.0, 1.0, model.nq)
            us = []
            for p in pols:
                u = [p(q1[None]).copy() for _ in range(N_sample)]          # one solve, then N_sample - 1 held steps
                assert all(np.array_equal(u[0], v) for v in u)
                us.append(u[0])
            iters = [p.newton_iters[-1] for p in pols]
            print(f"solve {step}: Newton iterations {[int(i[0]) for i in iters]}, max |u1| {np.abs(us[0]).max():.4g}")
            assert len(pols[0].newton_iters) == step + 1
            assert np.array_equal(us[0], us[1]) and np.array_equal(iters[0], iters[1]), f"solve {step}: the two host-path policies differ"
            assert np.array_equal(us[0], us[2]) and np.array_equal(iters[0], iters[2]), f"solve {step}: device tables differ from the host path"
            assert np.abs(us[0]).max() > 0
        for step in range(3):
            solve(step)
        t0, z, th = 5, P_host.z[4:8], P_host.theta[4:8].copy()
        th[:, -2] = model.mu_world
        assert not np.array_equal(th, P_host.theta[4:8])
        before = pols[2].solver.get_table(t0)
        pols[2].relinearize(z, th, t0=t0)
        triple = plant.linearize("quadruped", z, th, kappa)
        for p in pols[:2]:
            _host_path(p.solver, t0, z, th, triple)
        for t in range(t0, t0 + 4):
            assert np.array_equal(pols[0].solver.get_table(t), pols[2].solver.get_table(t)), f"knot {t} after relinearize"
        assert not np.array_equal(before, pols[2].solver.get_table(t0))
        for step in range(3, 5):
            solve(step)
        pols[2].relinearize()                          # the defaults: the problem's own z and θ, every knot
        assert np.array_equal(pols[2].solver.get_table(t0), before)
        for t in (1, 60):
            assert np.array_equal(pols[2].solver.get_table(t), pols[0].solver.get_table(t))
    finally:
        for p in pols:
            p.close()


# ---- 7. the recorded tables -----------------------------------------------------------------------------------------------------------
# layout of tests/table_build_cases.py -> the handle that has it: (model, mode)
RECORDED_HANDLES = {"quadruped": ("quadruped", 0), "hopper_3D": ("hopper_3D", 0), "centroidal": ("centroidal_quadruped", 0),
                    "pushbot mode 1": ("pushbot", 1), "wall": ("centroidal_quadruped_wall", 0), "wall generic": ("centroidal_quadruped_wall", 1)}


@pytest.mark.parametrize("layout", sorted(RECORDED_HANDLES))
def test_set_linearization_puts_the_recorded_tables_into_a_handle(layout):
    """A handle of one knot (H_ref = H = 1, B = 1) takes the layout's recorded knots one after the other: the table read back has the
    recorded size and SHA-256; the singular knot is refused and leaves the table set before it."""
    name, mode = RECORDED_HANDLES[layout]
    want = table_build_cases.recorded()[layout]
    s = _handle(lcp_models.MODELS[name](), mode, 1)
    try:
        assert s.query_sizes()[0] == want["size"]
        before = None
        for kn, knot in table_build_cases.knots(layout).items():
            if kn == "singular":
                assert before is not None
                with pytest.raises(_lib.CimpcError, match="singular"):
                    s.set_linearization(1, *knot)
                assert table_build_cases.table_hash(s.get_table(1)) == before, "the refused knot changed the table"
            else:
                s.set_linearization(1, *knot)
                before = table_build_cases.table_hash(s.get_table(1))
                assert before == want["knots"][kn], f"{layout}, knot {kn!r}"
    finally:
        s.close()
