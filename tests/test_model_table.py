"""`contactimplicitmpc/jl_amd/csrc/model_table.h` - the models the library is compiled for, each stated once, and the lookups the
dispatchers share - is plain C++: built here with g++ (tests/native/model_table_check.cpp).  The rows are held against the dimension
dicts of trajectory.py (which test_reference_shapes.py pins to the reference), the lookup rules against this file's own copy of the
rows, and csrc/ is searched for dimension lists that bypass the table."""
import os
import re
import shutil
import subprocess

import pytest

from contactimplicitmpc.jl_amd import trajectory as tr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "contactimplicitmpc", "jl_amd", "csrc")
FIELDS = ("nq", "nu", "nw", "nc", "nb")
ROWS = {name: tuple(d[k] for k in FIELDS) for name, d in dict(
    pushbot=tr.PUSHBOT, hopper=tr.HOPPER_2D, quadruped=tr.QUADRUPED, flamingo=tr.FLAMINGO, centroidal=tr.CENTROIDAL,
    hopper3d=tr.HOPPER_3D, walledcartpole=tr.WALLEDCARTPOLE, particle=tr.PARTICLE, particle2d=tr.PARTICLE_2D,
    centroidal_wall=tr.CENTROIDAL_WALL).items()}
ASYNC = {"pushbot", "hopper", "quadruped", "flamingo", "centroidal"}     # rows with a single-launch instantiation
LANES = {"centroidal": 32, "centroidal_wall": 64}                       # every other row: 16 lanes per problem
PAIRS = {(2, 2), (4, 2), (11, 8), (9, 6), (18, 12), (7, 3), (4, 1), (3, 3)}   # the (nq, nu) list the horizon-level kernels were compiled for


def _expected(dims, mode, H):
    """(sweep, callback, async) of five dimensions by the rules of ip_dispatch.hip, from this file's rows"""
    name = next((n for n, r in ROWS.items() if r == tuple(dims)), None)
    if name is None:
        return ["none"] * 3
    narrow = LANES.get(name, 16) <= 32
    return [name if narrow or mode == tr.MODE_CONFIGURATION else "none",
            name if narrow else "none",
            name if name in ASYNC and mode == tr.MODE_CONFIGURATION and H <= 96 else "none"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("model_table") / "model_table_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "native", "model_table_check.cpp")])

    def run(queries=()):
        text = "".join(" ".join(str(v) for v in q) + "\n" for q in queries)
        return [line.split() for line in subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    return run


def test_rows_are_the_reference_models(check):
    out = check()
    rows = [r for r in out if r[0] == "row"]
    assert len(rows) == len(ROWS) == 10 and {r[1] for r in rows} == set(ROWS)
    for _, name, *v in rows:
        v = [int(x) for x in v]
        assert tuple(v[:5]) == ROWS[name], name
        assert v[5] == LANES.get(name, 16), name
        assert v[6] == int(name in ASYNC), name
    assert {(int(r[1]), int(r[2])) for r in out if r[0] == "pair"} == PAIRS == {r[:2] for r in ROWS.values()}


def test_lookup_rules(check):
    queries = []
    for dims in ROWS.values():
        variants = [dims] + [dims[:k] + (dims[k] + s,) + dims[k + 1:] for k in range(5) for s in (1, -1)]     # the row and its near-misses
        queries += [(*v, mode, H) for v in variants for mode in (tr.MODE_CONFIGURATION, tr.MODE_CONFIGURATIONFORCE) for H in (96, 97)]
    got = [r for r in check(queries) if r[0] not in ("row", "pair")]
    assert len(got) == len(queries)
    for q, g in zip(queries, got):
        assert g == _expected(q[:5], q[5], q[6]), (q, g)
    # today no near-miss is another row, and the wall model has no compiled sweep in :configurationforce mode
    assert sum(g[0] != "none" for g in got) == 2 * (2 * 9 + 1)
    wall = queries.index((*ROWS["centroidal_wall"], tr.MODE_CONFIGURATIONFORCE, 96))
    assert got[wall] == ["none", "none", "none"]
    assert got[queries.index((*ROWS["centroidal_wall"], tr.MODE_CONFIGURATION, 96))] == ["centroidal_wall", "none", "none"]
    assert got[queries.index((*ROWS["quadruped"], tr.MODE_CONFIGURATION, 96))] == ["quadruped"] * 3
    assert got[queries.index((*ROWS["quadruped"], tr.MODE_CONFIGURATION, 97))] == ["quadruped", "quadruped", "none"]


def test_no_model_dimensions_outside_the_table():
    """the five-number rows are written in model_table.h alone, and the lists it replaced are gone"""
    tuples = re.compile("|".join(r"(?<![\w.])" + r"\s*,\s*".join(str(v) for v in r) + r"(?![\w.])" for r in ROWS.values()))
    lists = re.compile(r"#\s*define\s+(CIMPC_NQNU|CIMPC_MODELS|CIMPC_MODELS64|CIMPC_IS64)\b")
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".h", ".hip", ".cpp")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            hits += [f"{name}:{n}: {line.strip()}" for n, line in enumerate(f, 1)
                     if lists.search(line) or (name != "model_table.h" and tuples.search(line))]
    assert not hits, hits
