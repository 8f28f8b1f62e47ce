"""Cases and references shared by tests/test_plant_linearize.py (the header on the host) and tests/test_gpu_plant_linearize.py (the
kernel): the inputs of tests/test_plant_model_header.py (seeded uniform(0.1, 1) z and θ, κ = 1e-3), the torch linearization of
contactimplicitmpc/jl_amd/lcp_models.py, and the complex-step derivatives of the NumPy restatements on terrain
(tests/terrain_ref.py, tests/hopper_3d_ref.py).  Every reference is computed once per process."""
import functools

import numpy as np

KAPPA = 1e-3
# CIMPC_PLANT_* id -> the torch model of lcp_models.MODELS (flat ground); particle_2D (6) has no flat entry and no torch model
TORCH_MODELS = {0: "quadruped", 1: "flamingo", 2: "hopper_2D", 3: "centroidal_quadruped", 4: "centroidal_quadruped_undamped", 5: "particle",
                7: "centroidal_quadruped_box", 8: "centroidal_quadruped_wall", 10: "hopper_3D", 12: "pushbot", 13: "walledcartpole"}
# one terrain case per residual family, and particle_2D: (plant model name, id, terrain name)
TERRAIN_CASES = (("quadruped", 0, "sine1_2D_lc"), ("quadruped", 0, "piecewise1_2D_lc"), ("hopper_2D", 2, "slope1_2D_lc"),
                 ("particle", 5, "quadratic_bowl_3D_lc"), ("hopper_3D", 10, "sine2_3D_lc"), ("particle_2D", 6, "slope1_2D_lc"))


def inputs(mid: int, nz: int, nth: int, N: int = 1):
    """N knots of seeded uniform(0.1, 1) z and θ; knot 0 is the input of tests/test_plant_model_header.py for this id."""
    rng = np.random.default_rng(mid)
    z, th = np.empty((N, nz)), np.empty((N, nth))
    for k in range(N):
        z[k], th[k] = rng.uniform(0.1, 1.0, nz), rng.uniform(0.1, 1.0, nth)
    return z, th


@functools.lru_cache(maxsize=None)
def torch_case(mid: int, N: int = 3):
    """(z, θ, (r0, rz0, rθ0) of `linearize_batch`) of model id `mid` at N knots."""
    from contactimplicitmpc.jl_amd import lcp_models
    model = lcp_models.MODELS[TORCH_MODELS[mid]]()
    z, th = inputs(mid, model.nz, model.nth, N)
    return z, th, model.linearize_batch(z, th, KAPPA)


def encode_terrain(name: str) -> str:
    """A terrain as tests/native/plant_linearize_check.cpp reads it: kind n_pieces p[4] brk[8] off[8] coef[8][4]."""
    from contactimplicitmpc.jl_amd import terrain
    c = terrain.get(name).to_c()
    vals = list(c.p) + list(c.brk) + list(c.off) + [c.coef[i][k] for i in range(len(c.coef)) for k in range(4)]
    return " ".join([str(c.kind), str(c.n_pieces)] + [repr(float(v)) for v in vals])


def restatement(model: str, terrain: str):
    if model == "hopper_3D":
        import hopper_3d_ref
        return hopper_3d_ref.Hopper3DPlant(terrain)
    import terrain_ref
    return terrain_ref.plant(model, terrain)


def complex_step(P, z, th, kappa):
    """(r, dr/dz, dr/dθ) of a restatement that carries complex numbers: all nz + nθ directions in one batched evaluation, exact to round-off."""
    nz, n, eps = z.shape[0], z.shape[0] + th.shape[0], 1e-30
    X = np.tile(np.concatenate([z, th]).astype(complex), (n, 1)) + 1j * eps * np.eye(n)
    J = (P.residual(X[:, :nz], X[:, nz:], 0.0).imag / eps).T
    return P.residual(z, th, kappa), J[:, :nz], J[:, nz:]


@functools.lru_cache(maxsize=None)
def terrain_case(model: str, mid: int, terrain: str, N: int = 1):
    """(z, θ, [(r, rz, rθ) of the restatement per knot]) of `model` on `terrain`: the inputs of tests/test_terrain.py (x drawn over the
    terrain's features)."""
    P = restatement(model, terrain)
    z, th = inputs(100 + mid, P.dims.nz, P.dims.nth, N)
    rng = np.random.default_rng(200 + mid)
    z[:, 0] = rng.uniform(-1.0, 1.0, N) if model in ("particle", "hopper_3D") else rng.uniform(-0.5, 2.5, N)
    return z, th, [complex_step(P, z[k], th[k], KAPPA) for k in range(N)]


def assert_linearization(got, want, what=""):
    """The project's tolerance for this comparison (tests/test_plant_model_header.py, tests/test_terrain.py): 1e-12 max(1, max|r|) on r,
    1e-12 x the largest |entry| on each matrix.  Dual arithmetic, torch.func and the complex step are each exact to round-off
    (~1e-15 relative), three orders inside it."""
    for name, g, w in zip(("r0", "rz0", "rth0"), got, want):
        scale = max(1.0, np.abs(w).max()) if name == "r0" else np.abs(w).max()
        err = np.abs(np.asarray(g) - np.asarray(w)).max()
        print(f"{what} {name}: max|entry| {np.abs(w).max():.3g}, max deviation {err:.3g} (bound {1e-12 * scale:.3g})")
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-12 * scale, err_msg=f"{what} {name}")
