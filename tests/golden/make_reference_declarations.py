"""Generates tests/golden/reference_declarations.json from a checkout of the reference package:

    python tests/golden/make_reference_declarations.py <ContactImplicitMPC.jl checkout>

What julia/CIMPCHip.jl was written against, as data: the type parameters of `Newton` (src/controller/newton.jl:17), whether
`solver::LS` is a field and the solver is built by `eval(opts.solver)(jac.R)`, the argument names of `newton_solve!`
(newton.jl:169-177) and whether the policy calls it with the warm-start keyword (src/controller/policy.jl).  The JSON is the
committed fixture of tests/test_julia_binding.py::test_reference_declarations_are_what_the_binding_was_written_against."""
import json
import os
import re
import sys


def reference_declarations(newton_src, policy_src):
    m = re.search(r"mutable struct Newton\{([^}]*)\}", newton_src)
    sig = newton_src[newton_src.index("function newton_solve!("):]
    sig = sig[:sig.index("where T")]
    return {
        "newton_type_parameters": [x.strip() for x in m.group(1).split(",")],
        "solver_field_is_LS": bool(re.search(r"^\s*solver::LS\s*$", newton_src, flags=re.M)),
        "solver_built_by_eval_opts_solver": bool(re.search(r"solver = eval\(opts\.solver\)\(jac\.R\)", newton_src)),
        "newton_solve_argument_names": re.findall(r"^\s*(\w+)::", sig, flags=re.M),
        "policy_calls_newton_solve_with_warm_start": bool(re.search(
            r"newton_solve!\(p\.newton, p\.s, p\.q0, q1,\s*p\.window, p\.im_traj, p\.traj, warm_start = t > 1\)", policy_src)),
    }


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ctrl = os.path.join(sys.argv[1], "src", "controller")
    out = reference_declarations(open(os.path.join(ctrl, "newton.jl")).read(), open(os.path.join(ctrl, "policy.jl")).read())
    json.dump(out, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_declarations.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))
