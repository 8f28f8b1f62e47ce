"""Layouts and knots shared by tests/test_table_build.py (the table build on the host) and tests/test_gpu_table_build.py (the tables
a handle holds): the layout families, each one's seeded knot with a dominant diagonal in Dx, three further knots per layout whose Dx
makes the Gauss-Jordan step exchange rows and skip zero multipliers, and the tables recorded for all of them
(tests/golden/lin_table_sha256.json)."""
import hashlib
import json
import os

import numpy as np

# (nx, ny, nth, G, nths, adj) of the layout families: quadruped mode 0 (16 lanes, adjoint, Gs stored by row), hopper_3D mode 0 (nx > ny),
# centroidal_quadruped mode 0 (32 lanes, ldw = G + 1), pushbot mode 1 (column form), the wall mode 0 (64 lanes), the wall as the
# run-time-dimension kernel takes it (nths = 0, adj = 0), and the bound of that kernel, nx = ny = 64
LAYOUTS = {"quadruped": (11, 16, 34, 16, 30, 1), "hopper_3D": (7, 6, 22, 16, 17, 1), "centroidal": (18, 24, 53, 32, 48, 1),
           "pushbot mode 1": (2, 8, 10, 16, 6, 0), "wall": (18, 48, 53, 64, 48, 1), "wall generic": (18, 48, 53, 64, 0, 0),
           "64 x 64": (64, 64, 140, 64, 0, 0)}
# the knots recorded per layout, in the order of `knots`
KNOTS = ("own", "random", "sparse 1", "sparse 2", "singular")
RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lin_table_sha256.json")


def knot(name, singular=False):
    """(z0, th0, r0, rz0, rth0) of layout `name`: seeded normal entries, Dx with 3 added on its diagonal (no row is exchanged);
    `singular`: column 0 of Dx is zero."""
    nx, ny, nth, G, nths, adj = LAYOUTS[name]
    rng = np.random.default_rng(sorted(LAYOUTS).index(name))
    nz = nx + 2 * ny
    rz0 = rng.normal(size=(nz, nz))
    rz0[:nx, :nx] += 3.0 * np.eye(nx)
    if singular:
        rz0[:nx, 0] = 0.0
    return rng.normal(size=nz), rng.uniform(0.1, 1.0, nth), rng.normal(size=nz), rz0, rng.normal(size=(nz, nth))


def pivoting_knots(name):
    """Three knots that make the elimination exchange rows: Dx plain normal with nothing added to its diagonal; then twice a sparse Dx,
    about 60 % of its entries exactly zero (multipliers that are skipped) and in every column one entry of magnitude 4 to 5 on a
    permuted diagonal (the pivot is rarely the row it is looked for from)."""
    nx, ny, nth, G, nths, adj = LAYOUTS[name]
    nz = nx + 2 * ny
    out = []
    for j in range(3):
        rng = np.random.default_rng([1000 + sorted(LAYOUTS).index(name), j])
        rz0 = rng.normal(size=(nz, nz))
        if j > 0:
            Dx = rz0[:nx, :nx] * (rng.uniform(size=(nx, nx)) < 0.4)
            Dx[rng.permutation(nx), np.arange(nx)] = rng.choice([-1.0, 1.0], nx) * rng.uniform(4.0, 5.0, nx)
            rz0[:nx, :nx] = Dx
        out.append((rng.normal(size=nz), rng.uniform(0.1, 1.0, nth), rng.normal(size=nz), rz0, rng.normal(size=(nz, nth))))
    return out


def knots(name):
    """The five knots of layout `name` by the names in KNOTS."""
    return dict(zip(KNOTS, [knot(name), *pivoting_knots(name), knot(name, singular=True)]))


def table_hash(T):
    """SHA-256 of a table as little-endian float64 bytes; "singular" for a refused knot (None)."""
    return "singular" if T is None else hashlib.sha256(np.ascontiguousarray(T, dtype="<f8").tobytes()).hexdigest()


def recorded():
    """layout -> {"size": doubles per table, "knots": {knot name: hash}}, recorded from the packer `cimpc_set_linearization` had
    before it ran the shared build."""
    with open(RECORDED) as f:
        return json.load(f)
