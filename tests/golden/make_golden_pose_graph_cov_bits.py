"""The bits the pose-graph covariances and the operator product give, recorded as a fixture: tests/golden/pose_graph_cov_bits.json.

    python tests/golden/make_golden_pose_graph_cov_bits.py [--out tests/golden/pose_graph_cov_bits.json]      (RGBD360_LIB: the build to record from)

Record BEFORE the conjugate-gradient kernels change (k_pg_cg_*, csrc/pose_graph.h): tests/test_pose_graph_cov_gpu.py recomputes every case with
compute() below and demands these bits.  Per covariance case a SHA-256 of the cov bytes, cg_iterations, cg_residual as hex and every result
field, floats as hex; the graphs are those of tests/pose_graph_cases.py, optimised at cases.OPT first:
  n70/noisy             marginals of 0 (fixed: a zero block that never reaches the device), 1, 35, 69; relative (0, 69), (34, 35), (5, 5)
  variant/consistent    marginals of 1, 150 (fixed), 299, 300 (isolated); relative (149, 151), (300, 1)
  n300/noisy            17 marginals: one full batch of 16 and a batch of one
  n300/noisy, capped    the same 17 with cg_max_iters = 3: every column ends at the cap, the bits of an unfinished x and the flags
Per apply case (n70/noisy, variant/consistent at the start poses) a SHA-256 of y = (H + lambda diag H) x at lambda = 1e-3 and 0: the
edge product and the damped gather on their own.  Every case is computed twice in the process and nothing is written if the two differ.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_graph_cases as cases      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pose_graph_cov_bits.json")
VERTS17 = [int(v) for v in np.linspace(1, 299, 17).astype(int)]      # those of test_lock_step_is_query_by_query
# (key, graph, marginals, relative pairs, covariance parameters)
COV_CASES = (
    ("n70/noisy", ("n70", "noisy"), [0, 1, 35, 69], [(0, 69), (34, 35), (5, 5)], {}),
    ("variant/consistent", ("variant", "consistent"), [1, 150, 299, 300], [(149, 151), (300, 1)], {}),
    ("n300/noisy", ("n300", "noisy"), VERTS17, [], {}),
    ("n300/noisy/capped", ("n300", "noisy"), VERTS17, [], dict(cg_max_iters=3)),
)
APPLY_CASES = (("n70", "noisy"), ("variant", "consistent"))
APPLY_LAMBDAS = (1e-3, 0.0)


def _hex(v):
    return float(v).hex() if isinstance(v, (float, np.floating)) else int(v)


def record(cov, res):
    """What one covariance call is held to."""
    out = dict(cov_sha256=hashlib.sha256(np.ascontiguousarray(cov).tobytes()).hexdigest(),
               cg_iterations=[int(k) for k in res["cg_iterations"]], cg_residual=[float(r).hex() for r in res["cg_residual"]])
    out["result"] = {k: _hex(v) for k, v in res.items() if k not in ("cg_iterations", "cg_residual", "message")}
    return out


def _graph(reg, name, form):
    from rgbd360_amd.pose_graph import PoseGraph
    c = cases.case(name, form)
    g = PoseGraph(reg)
    g.add_vertices(c["poses"], fixed=c["fixed"])
    g.add_edges(c["ei"], c["ej"], c["Z"], c["Om"])
    return g


def compute(reg):
    """{"cov": {key: {"marginals": record, "relative": record}}, "apply": {"name/form": {lambda as hex: sha256 of y}}}."""
    out = dict(cov={}, apply={})
    for key, (name, form), verts, pairs, params in COV_CASES:
        with _graph(reg, name, form) as g:
            g.optimize(**cases.OPT)
            rec = dict(marginals=record(*g.marginals(verts, **params)))
            if pairs:
                rec["relative"] = record(*g.relative_covariances([p[0] for p in pairs], [p[1] for p in pairs], **params))
            out["cov"][key] = rec
    for name, form in APPLY_CASES:
        with _graph(reg, name, form) as g:
            x = np.random.default_rng(11).normal(size=(g.n_vertices, 6))
            out["apply"]["%s/%s" % (name, form)] = {float(lam).hex(): hashlib.sha256(g.apply(x, lam).tobytes()).hexdigest() for lam in APPLY_LAMBDAS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from rgbd360_amd.register import RegisterPhotoICP
    reg = RegisterPhotoICP(device=0)
    first, second = compute(reg), compute(reg)
    reg.close()
    if first != second:
        raise SystemExit("two runs in one process differ: nothing written")
    for k, v in first["cov"].items():
        m = v["marginals"]
        print(k, "status", m["result"]["status"], "iterations", m["cg_iterations"], m["cov_sha256"][:16])
    for k, v in first["apply"].items():
        print("apply", k, {lam: h[:16] for lam, h in v.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
