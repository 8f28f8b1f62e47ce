"""`plant_instance` and `plant_visit_instance` of `contactimplicitmpc/jl_amd/csrc/plant_ground.h`, the one place that maps a plant model
to the kernel instantiation it runs on: built here with g++ (tests/native/plant_ground_check.cpp).  Every model fits the instance it
is given, flat and on terrain, for the step kernel and for the linearization / sensitivity kernels, and the choice is the table
written out below - the launch chains the three kernels had before the header."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FLAT, TERRAIN, ENV, WALLS = range(4)
SHARED = {False: (66, 53, FLAT), True: (66, 53, TERRAIN)}          # by on_terrain
# id -> instance, or a function of (on_terrain, for_step)
TABLE = {
    **{i: (lambda ter, step: SHARED[ter]) for i in range(7)},      # quadruped, flamingo, hopper_2D, centroidal (2), particle, particle_2D
    7: (66, 53, ENV),                                              # centroidal_quadruped_box
    8: (114, 53, ENV),                                             # centroidal_quadruped_wall
    10: lambda ter, step: (19, 22, TERRAIN) if ter or not step else (66, 53, FLAT),      # hopper_3D: the step kernel keeps it on FLAT
    12: (20, 15, WALLS),                                           # pushbot
    13: (20, 15, WALLS),                                           # walledcartpole
}
NO_MODEL = (-1, 9, 11, 14)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plant_instance_fits_and_matches_the_launch_table(tmp_path):
    exe = str(tmp_path / "plant_ground_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "plant_ground_check.cpp")])
    ids = sorted((*TABLE, *NO_MODEL))
    assert set(range(9)) <= set(ids)
    out = subprocess.run([exe] + [str(i) for i in ids], capture_output=True, text=True, check=True).stdout
    print(out)
    rows = [[int(v) for v in line.split()] for line in out.splitlines()]
    seen, instances = set(), set()
    for row in rows:
        i, found = row[:2]
        if i in NO_MODEL:
            assert row == [i, 0], row                              # an id with no model is refused
            seen.add(i)
            continue
        assert found == 1, row
        ter, step, nz, nth, NZ, NTH, ground, visited = row[2:]
        assert nz <= NZ and nth <= NTH, row                         # the model fits: the kernel's `nz > NZ || nth > NTH` never fires
        want = TABLE[i](bool(ter), bool(step)) if callable(TABLE[i]) else TABLE[i]
        assert (NZ, NTH, ground) == want, row
        assert visited == 1, row                                   # the visitor hands over the instance plant_instance names
        seen.add((i, ter, step))
        instances.add((NZ, NTH, ground))
    assert seen == set(NO_MODEL) | {(i, t, s) for i in TABLE for t in (0, 1) for s in (0, 1)}
    assert instances == {(20, 15, WALLS), (19, 22, TERRAIN), (66, 53, ENV), (114, 53, ENV), (66, 53, TERRAIN), (66, 53, FLAT)}
    # the step kernel's exception: a flat hopper_3D on the shared FLAT instantiation, everything else of hopper_3D on its own size
    hopper = {(r[2], r[3]): tuple(r[6:9]) for r in rows if r[0] == 10}
    assert hopper == {(0, 1): (66, 53, FLAT), (1, 1): (19, 22, TERRAIN), (0, 0): (19, 22, TERRAIN), (1, 0): (19, 22, TERRAIN)}
