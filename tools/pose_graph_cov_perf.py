"""The pose-graph covariance batch on the device (rgbd360_graph_marginals, csrc/pose_graph_cov.h) against the single-right-hand-side solver.

    python tools/pose_graph_cov_perf.py [--sizes 1000,10000] [--reps 20] [--rounds 5] [--out profiles/pose_graph_cov_perf.txt]

Per size N: the chain-plus-10 %-closure graph of tools/pose_graph_perf.py, optimised once at the defaults; 16 vertices spread over the chain.
  lock step   the wall time of whole rgbd360_graph_marginals calls of those 16 queries (96 right-hand sides in one batch, cg_max_iters
              launches enqueued blindly, one synchronisation), `rounds` times in one process, with the iteration counts they report;
  kernels     HIP-event averages over `reps` launches of the batch's kernels (rgbd360_graph_time_cov_kernels), the edge product in both work
              mappings: one thread per (edge, column), and one thread per (edge, query) holding W for six columns;
  baseline    the same 96 right-hand sides solved one after another by the single-right-hand-side kernels of rgbd360_graph_optimize, from
              their HIP-event averages (rgbd360_graph_time_kernels): per column, its iterations x (edge product + gather + update +
              direction) + the remaining launches of cg_max_iters x the launch that returns on the state word.  A column's iteration count
              is taken as its query's (the largest of its six).
The lock-step form ships only if it is not slower than the baseline on every size; the tool prints the verdict and changes nothing.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_graph_perf import make_graph                    # noqa: E402
from rgbd360_amd.pose_graph import PoseGraph              # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP         # noqa: E402

KERNELS = ("k_pgc_init", "k_pg_cg_edge<per column>", "k_pg_cg_edge<per query>", "k_pg_cg_gather", "k_pg_cg_update", "k_pg_cg_dir", "k_pgc_finish",
           "a launch returning on the stop words")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("rgbd360_graph_marginals, 16 queries = 96 right-hand sides in lock step: whole calls in milliseconds (wall clock, %d rounds), kernels as "
        "HIP-event averages over %d launches in microseconds" % (a.rounds, a.reps))
    reg = RegisterPhotoICP()
    verdicts = []
    for n in [int(s) for s in a.sizes.split(",")]:
        poses, i, j, Z, Om = make_graph(n, np.random.default_rng(n))
        with PoseGraph(reg) as g:
            g.add_vertices(poses, fixed=[0])
            g.add_edges(i, j, Z, Om)
            opt = g.optimize()
            verts = np.linspace(1, n - 1, 16).astype(np.int32)
            p = g.cov_params()
            say("N = %d vertices, E = %d edges; optimised: status %d, %d iterations, cost %.6g; cg_max_iters %d, cg_tol %g"
                % (g.n_vertices, g.n_edges, opt["status"], opt["iterations"], opt["chi2_final"], p.cg_max_iters, p.cg_tol))
            ms, res = [], None
            for r in range(a.rounds + 1):      # the first call allocates the batch's memory: not counted
                t0 = time.perf_counter()
                cov, res = g.marginals(verts)
                if r:
                    ms.append((time.perf_counter() - t0) * 1e3)
            its = res["cg_iterations"].astype(np.int64)
            say("  lock step: %s ms; median %.2f; status %d, %d queries not converged, iterations per query %s, largest residual %.3g"
                % (" ".join("%.2f" % m for m in ms), float(np.median(ms)), res["status"], res["n_not_converged"], its.tolist(), res["cg_residual_max"]))
            us = g.time_cov_kernels(verts, a.reps)
            say("  kernels: " + ", ".join("%s %.1f" % (k, v) for k, v in zip(KERNELS, us)))
            say("  work mapping of the edge product: per column %.1f us, per query %.1f us" % (us[1], us[2]))
            single = g.time_kernels(a.reps)
            step = float(single[2:6].sum())
            base_ms = float((6 * (its * step + (p.cg_max_iters - its) * 4.0 * float(single[9]))).sum()) / 1e3
            say("  single right-hand side: edge %.1f, gather %.1f, update %.1f, direction %.1f us = %.1f us per iteration; a returning launch %.1f us"
                % (single[2], single[3], single[4], single[5], step, single[9]))
            ok = float(np.median(ms)) <= base_ms
            verdicts.append(ok)
            say("  baseline, 96 right-hand sides one after another: %.1f ms; lock step %.2f ms: %.1f x; not slower: %s"
                % (base_ms, float(np.median(ms)), base_ms / float(np.median(ms)), "met" if ok else "NOT met"))
    say("ship condition (not slower than the baseline on every size): %s" % ("met" if all(verdicts) else "NOT met"))
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
