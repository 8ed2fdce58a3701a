"""Writes tests/golden/pose_graph_cov.json: per case of tests/pose_graph_cov_reference.py (the noisy graphs of tests/pose_graph_cases.py, n70
consistent, and the Cauchy graph with two disabled closures) the error of the numpy restatement of the device's conjugate gradients against
the dense inverse, max |C^_ab - C_ab| / sqrt(C_aa C_bb) over the entries of every queried block, at the defaults (cg_tol 1e-10, 1000
iterations) and at the reference optimum.  The GPU tests allow the device 8 x that plus 1e-13 (pose_graph_cov_reference.device_bound).

    python tests/golden/make_golden_pose_graph_cov.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pose_graph_cov_reference as CR      # noqa: E402


def main():
    out = {}
    for name, form in CR.CASES + [(CR.ROBUST_CASE, "noisy")]:
        err, its, res = CR.restatement_error(name, form)
        g = CR.case_graph(name, form)[0]
        cost, dof, vf = CR.variance_factor(g)
        out[CR.case_id(name, form)] = dict(error=err, cg_iterations_max=its, cg_residual_max=res, dof=dof, variance_factor=vf)
        print(CR.case_id(name, form), out[CR.case_id(name, form)])
    with open(CR.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
