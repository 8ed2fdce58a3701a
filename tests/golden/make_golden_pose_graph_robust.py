"""The optima of the numpy reference on the corrupted graphs of tests/pose_graph_robust_reference.py, stored so that the GPU tests do not
spend a minute of every run in numpy: tests/golden/pose_graph_robust_optima.npz.

    python tests/golden/make_golden_pose_graph_robust.py

Keys "<name>/<kind>" for the five combinations the GPU tests hold the device to (dense solve, pose_graph_robust_reference.OPT) and
"<name>/clean" for the optimum of the graph without the wrong edges; values [N,4,4] float64.  tests/test_pose_graph_robust_cpu.py
recomputes every one of them and compares.  No library call, no device.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_graph_robust_reference as RR      # noqa: E402


def main():
    out = {}
    for name, kind in RR.COMBOS:
        out["%s/%s" % (name, RR.KIND_NAMES[kind])] = RR.optimum(name, kind)[0]
    for name in ("n70", "n300"):
        out["%s/clean" % name] = RR.clean_optimum(name)[0]
    np.savez_compressed(RR.STORED, **out)
    print("wrote", RR.STORED, os.path.getsize(RR.STORED), "bytes")


if __name__ == "__main__":
    main()
