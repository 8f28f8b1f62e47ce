#!/usr/bin/env python3
"""Sampling MPC through contact in closed loop (`plant.SamplingPolicy`, `cimpc_plant_sampler`) on the scene of
scripts/closed_loop_ilqr_mpc.py (`plant_mpc_cases.scene`): the three hoppers are asked to carry the body 5 cm along over S = 20 control steps
and run on a TRUE plant the planner does not know - one friction coefficient (0.5) where the planner believes (0.8, 0.3, 0.05), and an
`ImpulseDisturbance` at simulator step 6 - through `plant.simulate`.  Printed per robot: the executed trajectory's `TrackingCost` under the
policy (re-planned at every step from the measured state, the plan shifted by one) and under open-loop replay of the step-0 plan, under the
same impulse.  The policy's settings are `plant_sample_cases.SCENE_SAMPLING`, fixed before the first run and not tuned afterwards.
usage: python scripts/closed_loop_sampling_mpc.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from contactimplicitmpc.jl_amd import plant  # noqa: E402
import plant_mpc_cases as pmc  # noqa: E402
import plant_sample_cases as psc  # noqa: E402


def main():
    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    c, ref, u0, _ = pmc.scene(plant)
    H = pmc.SCENE_STEPS
    st = dict(psc.SCENE_SAMPLING)
    st["sigma"] = np.full(2, st.pop("sigma_fraction") * np.abs(c["u"]).max())
    first_plan, steps = [], []
    with plant.SamplingPolicy(c["model"], c["q1"].shape[0], H, c["h"], c["mu"], ref, u0, **st) as pol:
        pol.start(c["q1"] - c["h"] * c["v1"])

        def mpc(q):
            u = pol(q)
            if not first_plan:
                first_plan.append(pol.plan()[0])
            steps.append(dict(s=pol.s, choice=pol.last.choice[-1].tolist(), n_eligible=pol.last.n_eligible[-1].tolist(), J_nom=pol.last.J_nom[-1].tolist(),
                              J_best=pol.last.J_best[-1].tolist()))
            return u
        q_mpc, u_mpc = pmc.run_scene(plant, mpc)
    q_open, u_open = pmc.run_scene(plant, pmc.replay(first_plan[0]))
    J_mpc, J_open = pmc.executed_cost(ref, q_mpc, u_mpc), pmc.executed_cost(ref, q_open, u_open)
    print(json.dumps({"scene": {"model": c["model"], "B": 3, "H": H, "S": H, "planner_mu": c["mu"].tolist(), "true_mu": pmc.SCENE_TRUE_MU,
                                "impulse": {"w": pmc.SCENE_IMPULSE[0].tolist(), "simulator_step": pmc.SCENE_IMPULSE[1]},
                                "policy": {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in st.items()}},
                      "executed_cost_sampling": J_mpc.tolist(), "executed_cost_open_loop_replay_of_the_step_0_plan": J_open.tolist(),
                      "sampling_below_open_loop": (J_mpc < J_open).tolist(), "final_x_sampling": q_mpc[-1, :, 0].tolist(), "final_x_open_loop": q_open[-1, :, 0].tolist(),
                      "goal_x": ref.x_ref[-1, 0].tolist(), "steps": steps}))


if __name__ == "__main__":
    main()
