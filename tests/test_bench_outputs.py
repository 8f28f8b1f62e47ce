"""`bench.py --dump-outputs DIR` writes what the last timed step returned, so that two builds can be compared output for output,
and a plain run (no `--full`) is only the headline: set up, warm up, the timed steps, the outputs, the line.

CPU part: `bench.dump_outputs` on stand-in results - float64 files, every rollout in global order, and above the size limit the same
fixed seeded sample of rollouts from every array.  GPU part (`-m gpu`): a plain run of a small batch end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("latency_b1", "mpc_loop_b1", "real_problem", "centroidal_payload_h60", "cpu_baseline", "multi_gpu")
NAMES = ("u1", "newton_iters", "r_norm", "sweeps", "traj_q", "traj_u", "traj_gamma", "traj_b", "traj_nu", "rollout_index")


class _StandIn:
    """the two things dump_outputs asks of a solver: the trajectory download (shapes of CIMPCSolver.trajectory)"""
    def __init__(self, B, H=4, nq=3, nu=2, nc=2, nb=2):
        rng = np.random.default_rng(5)
        self.traj = dict(q=rng.normal(size=(B, H + 2, nq)), u=rng.normal(size=(B, H, nu)), gamma=rng.normal(size=(B, H, nc)),
                         b=rng.normal(size=(B, H, nb)), nu=rng.normal(size=(B, H, nq)))

    def trajectory(self):
        return {k: v.copy() for k, v in self.traj.items()}


def _gathered(B, nu=2):
    return dict(u1=np.arange(B * nu, dtype=np.float64).reshape(B, nu), newton_iters=np.arange(B, dtype=np.int64) % 5,
                r_norm=np.linspace(0, 1, B), sweeps=np.arange(B, dtype=np.int64))


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_dump_writes_every_rollout_in_float64(tmp_path):
    import bench
    B = 7
    s = _StandIn(B)
    bench.dump_outputs(str(tmp_path), s, _gathered(B), B, "cpu", 0)
    got = _load(tmp_path)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in NAMES)
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["rollout_index"], np.arange(B))
    np.testing.assert_array_equal(got["u1"], _gathered(B)["u1"])
    np.testing.assert_array_equal(got["newton_iters"], _gathered(B)["newton_iters"])
    for k, v in s.traj.items():
        np.testing.assert_array_equal(got["traj_" + k], v)


def test_dump_above_the_limit_is_the_same_seeded_sample_everywhere(tmp_path, monkeypatch):
    import bench
    B = 200
    s = _StandIn(B)
    per_row = sum(a.nbytes for a in list(_gathered(B).values()) + list(s.traj.values())) / B + 8
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", int(per_row * 50))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), s, _gathered(B), B, "cpu", 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    rows = a["rollout_index"].astype(np.int64)
    assert len(rows) == 50 and np.all(np.diff(rows) > 0) and rows[-1] < B
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_LIMIT_BYTES
    for n in NAMES:
        np.testing.assert_array_equal(a[n], b[n])                    # the same sample from run to run
    np.testing.assert_array_equal(a["u1"], _gathered(B)["u1"][rows])  # and the same rows in every array
    np.testing.assert_array_equal(a["traj_q"], s.traj["q"][rows])


def test_dump_on_a_rank_other_than_0_writes_nothing(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path / "x"), _StandIn(3), _gathered(3), 3, "cpu", 1)
    assert not os.path.exists(tmp_path / "x")


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run of 16 rollouts: ONE line with the headline fields, `steps` timed steps, none of the --full legs, and the dumped
    arrays agree with the line and with each other (u1 is core.traj.u[1] of every rollout)."""
    B, steps = 16, 3
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--rollouts", str(B),
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    o = json.loads(lines[0])
    assert o["unit"] == "MPC steps/s" and o["higher_is_better"] is True and o["dtype"] == "f64" and o["steps"] == steps
    assert o["value"] > 0 and o["ms_per_step"] > 0
    assert abs(o["value"] - B * 1e3 / o["ms_per_step"]) < 1e-6 * o["value"]
    assert not [k for k in FULL_ONLY if k in o], "a plain run ran --full legs"
    got = _load(tmp_path)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["u1"].shape == (B, 8) and got["traj_q"].shape == (B, 42, 11) and got["traj_u"].shape == (B, 40, 8)
    np.testing.assert_array_equal(got["rollout_index"], np.arange(B))
    np.testing.assert_array_equal(got["u1"], got["traj_u"][:, 0])
    assert int((got["r_norm"] < 3e-4).sum()) == o["solver_iters"]["converged_rollouts"]
    assert np.all(np.isfinite(got["traj_q"])) and np.all(np.isfinite(got["u1"]))
