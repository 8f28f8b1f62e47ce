"""`plant_model_by_id` of `contactimplicitmpc/jl_amd/csrc/plant_model.h`, the one id -> model function of the device plant and of
the native harnesses: built here with g++ (tests/native/plant_model_by_id_check.cpp) and compared with the tables of plant.py."""
import os
import shutil
import subprocess

import pytest

from contactimplicitmpc.jl_amd import plant

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plant_model_by_id_matches_model_dims(tmp_path):
    exe = str(tmp_path / "by_id_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "plant_model_by_id_check.cpp")])
    want = {}
    for name in (*plant.MODELS, *plant.TERRAIN_MODELS, *plant.CENTROIDAL_ENV_MODELS):
        mid, nq, nu, nc, fd, nw = plant.model_dims(name)
        want[mid] = (nq, nu, nc, fd * nc, nw)
    assert sorted(want) == list(range(9))
    ids = list(range(-1, 10))
    out = subprocess.run([exe] + [str(i) for i in ids], capture_output=True, text=True, check=True).stdout.split("\n")
    for i, line in zip(ids, out):
        got = [int(v) for v in line.split()]
        assert got[0] == i
        if i in want:
            assert got[1] == 1 and tuple(got[2:]) == want[i], (i, got)
        else:
            assert got[1] == 0, (i, got)
