"""How the plant entries stage their arrays, without a device (csrc/plant_staging.h): the header built with g++ and
its check program run - regions that tile their buffer, the copier driven with memcpy over heap buffers of exactly the layout's need, the
layouts of `cimpc_plant_tape_linesearch` and `cimpc_plant_rollout_segments` against offsets worked out by hand, the refusal helpers'
strings - and the same program once more under AddressSanitizer and UBSan, where a copy that ran past its region would abort."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "contactimplicitmpc", "jl_amd", "csrc")
SRC = os.path.join(HERE, "native", "plant_staging_check.cpp")
ENTRIES = ("plant_riccati.hip", "plant_linesearch.hip", "plant_ilqr.hip", "plant_mpc.hip", "plant_sample.hip", "plant_shooting.hip")


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    word, count = r.stdout.split()
    assert word == "ok" and int(count) > 1000, r.stdout


def test_the_header_builds_without_hip_and_its_check_passes(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    out = str(tmp_path / "plant_staging_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-o", out, SRC])
    _run(out)


def test_the_check_under_the_sanitizers(tmp_path):
    """Skips only where g++ or the sanitizers' runtimes are missing, which a trivial program shows; a failed build of the program itself
    fails the test."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    flags = ["-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes")
    out = str(tmp_path / "plant_staging_check_san")
    subprocess.check_call(["g++", *flags, "-o", out, SRC])
    _run(out)


def test_the_entries_stage_through_the_header_alone():
    """No entry lays a buffer out or copies an array by an extent of its own: no offset chain, no copy lambda, no device scope written
    out, and none of the structs and twins that the header and the workspace state once."""
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "plant_staging.h " in make
    hdr = open(os.path.join(CSRC, "plant_staging.h")).read()
    assert "#include <hip" not in hdr and "hipStream_t" not in hdr and "__device__" not in hdr, "the header includes no HIP"
    for name in ENTRIES:
        src = open(os.path.join(CSRC, name)).read()
        for gone in ("auto next = ", "auto up = ", "auto down = ", "auto finite = ", "std::pair<const char*, const void*>", "hipSetDevice", "hipGetDevice(",
                     "std::lock_guard", "LineSearchWs", "ShootingWs", "RiccatiWs", "IlqrWs", "shoot_cost_of", "mpc_on_device", "smp_on_device",
                     "mpc_refuse", "smp_refuse", "plant_shoot_restore_kernel", "set_global_error"):
            if gone == "std::lock_guard" and name == "plant_shooting.hip":
                continue      # cimpc_plant_rollout_segments runs on the caller's device: it takes the mutex and selects nothing
            assert gone not in src, f"{name} still spells out {gone}"
    for name in ("plant_tangent.hip", "plant_adjoint.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert "PlantDeviceScope" in src and "hipSetDevice" not in src
    shooting = open(os.path.join(CSRC, "plant_shooting.hip")).read()
    assert shooting.count("std::lock_guard") == 1 and "plant_restore_launch(" in shooting
    assert open(os.path.join(CSRC, "plant_linesearch.hip")).read().count("__global__") == 4      # expand, cost, gather, restore: the one restore kernel
