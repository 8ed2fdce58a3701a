"""The bits the device pose-graph optimiser produces, recorded as a fixture: tests/golden/pose_graph_bits.json.

    python tests/golden/make_golden_pose_graph_bits.py [--out tests/golden/pose_graph_bits.json]      (RGBD360_LIB: the build to record from)

Uses only add_vertices / add_edges / optimize / poses / trace, so it runs on a library from before the robust and switchable edges
(csrc/pose_graph.h).  Record BEFORE k_pg_edges changes: tests/test_pose_graph_robust_gpu.py recomputes every case with compute() below and
demands these bits of a graph whose edges are all quadratic and enabled.  Per graph of tests/pose_graph_cases.py (n70/noisy,
variant/consistent, n300/noisy) at cases.OPT: a SHA-256 of the float32 pose bytes, the result fields and every trace record, floats as hex.
Every case is computed twice in the process and nothing is written if the two differ.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_graph_cases as cases      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pose_graph_bits.json")
CASES = (("n70", "noisy"), ("variant", "consistent"), ("n300", "noisy"))


def _hex(d):
    return {k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in d.items()}


def record(g):
    """What one optimised graph is held to: g is a rgbd360_amd.pose_graph.PoseGraph ready to run."""
    res = g.optimize(**cases.OPT)
    return dict(poses_sha256=hashlib.sha256(g.poses().tobytes()).hexdigest(), result=_hex(res), trace=[_hex(t) for t in g.trace()])


def compute(reg, configure=None):
    """{"name/form": record}; configure(graph), when given, is called on every built graph before it runs."""
    from rgbd360_amd.pose_graph import PoseGraph
    out = {}
    for name, form in CASES:
        c = cases.case(name, form)
        with PoseGraph(reg) as g:
            g.add_vertices(c["poses"], fixed=c["fixed"])
            g.add_edges(c["ei"], c["ej"], c["Z"], c["Om"])
            if configure is not None:
                configure(g)
            out["%s/%s" % (name, form)] = record(g)
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
    for k, v in first.items():
        print(k, "iterations", v["result"]["iterations"], "status", v["result"]["status"], v["poses_sha256"][:16])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
