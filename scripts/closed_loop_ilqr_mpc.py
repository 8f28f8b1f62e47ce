#!/usr/bin/env python3
"""iLQR-MPC through contact in closed loop (`plant.ILQRPolicy`, `cimpc_plant_mpc`): the three hoppers of
`plant_gradient_cases.rollout_case("hopper_2D")` are asked to carry the body 5 cm along over S = 20 control steps and run on a TRUE plant the
planner does not know - one friction coefficient (0.5) where the planner believes (0.8, 0.3, 0.05), and an `ImpulseDisturbance` at simulator
step 6 - through `plant.simulate`.  Printed per robot: the executed trajectory's `TrackingCost` under MPC (re-planned at every step from the
measured state, the plan shifted by one) and under open-loop replay of the step-0 plan, under the same impulse.  The scene is
`plant_mpc_cases.scene`; tests/test_gpu_plant_mpc.py asserts the ordering on it.
usage: python scripts/closed_loop_ilqr_mpc.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from contactimplicitmpc.jl_amd import plant  # noqa: E402
import plant_mpc_cases as pmc  # noqa: E402


def main():
    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    c, ref, u0, kw = pmc.scene(plant)
    H = pmc.SCENE_STEPS
    first_plan, steps = [], []
    with plant.ILQRPolicy(c["model"], c["q1"].shape[0], H, c["h"], c["mu"], ref, u0, **kw) as pol:
        pol.start(c["q1"] - c["h"] * c["v1"])

        def mpc(q):
            u = pol(q)
            if not first_plan:
                first_plan.append(pol.plan()[0])
            steps.append(dict(s=pol.s, n_done=pol.last.n_done, accepted=pol.last.accepted.sum(axis=0).tolist(), converged=pol.last.converged.tolist()))
            return u
        q_mpc, u_mpc = pmc.run_scene(plant, mpc)
    q_open, u_open = pmc.run_scene(plant, pmc.replay(first_plan[0]))
    J_mpc, J_open = pmc.executed_cost(ref, q_mpc, u_mpc), pmc.executed_cost(ref, q_open, u_open)
    print(json.dumps({"scene": {"model": c["model"], "B": 3, "H": H, "S": H, "planner_mu": c["mu"].tolist(), "true_mu": pmc.SCENE_TRUE_MU,
                                "impulse": {"w": pmc.SCENE_IMPULSE[0].tolist(), "simulator_step": pmc.SCENE_IMPULSE[1]}, "policy": {k: v for k, v in kw.items()}},
                      "executed_cost_mpc": J_mpc.tolist(), "executed_cost_open_loop_replay_of_the_step_0_plan": J_open.tolist(),
                      "mpc_below_open_loop": (J_mpc < J_open).tolist(), "final_x_mpc": q_mpc[-1, :, 0].tolist(), "final_x_open_loop": q_open[-1, :, 0].tolist(),
                      "goal_x": ref.x_ref[-1, 0].tolist(), "steps": steps}))


if __name__ == "__main__":
    main()
