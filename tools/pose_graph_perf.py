"""The pose-graph optimiser's kernels and whole calls on the device (rgbd360_graph_*, csrc/pose_graph.h).

    python tools/pose_graph_perf.py [--sizes 1000,10000,100000] [--reps 20] [--rounds 3] [--out profiles/pose_graph_perf.txt]
    python tools/pose_graph_perf.py --robust [--parent-tree <a built checkout of the parent commit>] [--sizes 10000,100000] [--rounds 9] [--out ...]

Per size N: a chain of N vertices (0.1 m steps) with N / 10 random closures, noisy relative poses (0.02 m, 0.01 rad), information of order
1e4, started from the chained odometry, vertex 0 fixed.  HIP-event averages over `reps` launches of every kernel of one Levenberg-Marquardt
iteration (rgbd360_graph_time_kernels), a launch that returns at once on the state word, and the wall time of whole rgbd360_graph_optimize
calls at the defaults (10 iterations, cg_tol 1e-8, 400 conjugate-gradient iterations per solve) with their iteration counts, `rounds`
times in one process.  No rate is part of any acceptance; the block-Jacobi iteration count grows with the graph's diameter.

--robust: what the robust and switchable edges cost a graph that does not use them.  Per size, `rounds` repetitions of the HIP-event average
of k_pg_edges<linearise> and of the wall time of a whole optimize call, with every edge RGBD360_GRAPH_ROBUST_NONE and with every closure
Cauchy (delta 6); median and interquartile range of each.  With --parent-tree the same two figures are first measured in a child process
of this run: that checkout's own tools/pose_graph_perf.py (same graphs, reps and rounds) on its own library, its report parsed.  The
all-NONE kernel time may exceed the parent's median by no more than the parent's own interquartile range; the tool prints the verdict and
changes nothing else.
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd.pose_graph import PoseGraph              # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP         # noqa: E402

KERNELS = ("k_pg_edges<linearise>", "k_pg_assemble", "k_pg_cg_edge", "k_pg_cg_gather", "k_pg_cg_update", "k_pg_cg_dir", "k_pg_trial",
           "k_pg_edges<chi2>", "k_pg_decide", "a launch returning on the state word")


def rodrigues(w):
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -w[..., 2], w[..., 1], w[..., 2], -w[..., 0], -w[..., 1], w[..., 0]
    th = np.maximum(th, 1e-12)
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def rigid(Rm, t):
    T = np.zeros(Rm.shape[:-2] + (4, 4))
    T[..., :3, :3], T[..., :3, 3], T[..., 3, 3] = Rm, t, 1.0
    return T


def inv(T):
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    return rigid(Rt, -(Rt @ T[..., :3, 3:4])[..., 0])


def make_graph(n, rng):
    steps = rigid(rodrigues(rng.normal(0, 0.06, (n - 1, 3))), np.array([0.1, 0, 0]) + rng.normal(0, 0.02, (n - 1, 3)))
    gt = [np.eye(4)]
    for s in steps:
        gt.append(gt[-1] @ s)
    gt = np.stack(gt)
    i = np.concatenate([np.arange(n - 1), rng.integers(0, n, n // 10)])
    j = np.concatenate([np.arange(1, n), rng.integers(0, n, n // 10)])
    keep = i != j
    i, j = i[keep], j[keep]
    noise = rigid(rodrigues(rng.normal(0, 0.01, (len(i), 3))), rng.normal(0, 0.02, (len(i), 3)))
    Z = (noise @ inv(gt[i]) @ gt[j]).astype(np.float32)
    Q = np.linalg.qr(rng.normal(size=(len(i), 6, 6)))[0]
    Om = ((Q * rng.uniform(0.5e4, 2e4, (len(i), 1, 6))) @ np.swapaxes(Q, -1, -2)).astype(np.float32)
    start = [np.eye(4)]
    for k in range(n - 1):
        start.append(start[-1] @ Z[k].astype(np.float64))
    return np.stack(start).astype(np.float32), i.astype(np.int32), j.astype(np.int32), Z, Om


def robust_column(g, poses, first_closure, rounds, reps, cauchy):
    """[rounds] k_pg_edges<linearise> microseconds and [rounds] optimize milliseconds; cauchy: None (the settings are not touched: the
    only choice on a library without them), False (every edge NONE, set explicitly) or True (every closure Cauchy, delta 6)."""
    if cauchy is not None:
        n = g.n_edges - first_closure
        g.set_edge_robust(0, np.zeros(g.n_edges, np.int32))
        if cauchy and n:
            g.set_edge_robust(first_closure, np.full(n, 2, np.int32), 6.0)
    us, ms, last = [], [], None
    for _ in range(rounds):
        us.append(float(g.time_kernels(reps)[0]))
    for _ in range(rounds):
        g.set_poses(0, poses)
        t0 = time.perf_counter()
        last = g.optimize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return us, ms, last


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return float(med), float(q3 - q1)


def robust_main(a, say):
    sizes = [int(s) for s in a.sizes.split(",")]
    say("rgbd360_graph_* with and without robust edges: k_pg_edges<linearise> as HIP-event averages over %d launches in microseconds, whole optimize "
        "calls at the defaults in milliseconds; median (interquartile range) over %d repetitions" % (a.reps, a.rounds))
    parent = None
    if a.parent_tree:      # before this process opens the device: one process on it at a time
        tool = os.path.join(os.path.abspath(a.parent_tree), "tools", "pose_graph_perf.py")
        env = {k: v for k, v in os.environ.items() if k != "RGBD360_LIB"}
        text = subprocess.run([sys.executable, tool, "--sizes", a.sizes, "--reps", str(a.reps), "--rounds", str(a.rounds)], env=env, check=True,
                              capture_output=True, text=True).stdout
        parent, cur = {}, None
        for line in text.splitlines():
            m = re.match(r"N = (\d+) vertices", line)
            if m:
                cur = parent.setdefault(m.group(1), dict(us=[], ms=[]))
            m = re.match(r"  round \d+: k_pg_edges<linearise> ([0-9.]+),", line)
            if m:
                cur["us"].append(float(m.group(1)))
            m = re.match(r"  optimize round \d+: ([0-9.]+) ms, status \d+, (\d+) iterations .* chi2 \S+ -> (\S+)$", line)
            if m:
                cur["ms"].append(float(m.group(1)))
                cur.update(iterations=int(m.group(2)), chi2_final=m.group(3))
    reg = RegisterPhotoICP()
    for n in sizes:
        poses, i, j, Z, Om = make_graph(n, np.random.default_rng(n))
        with PoseGraph(reg) as g:
            g.add_vertices(poses, fixed=[0])
            g.add_edges(i, j, Z, Om)
            say("N = %d vertices, E = %d edges (%d closures)" % (g.n_vertices, g.n_edges, g.n_edges - (n - 1)))
            rows = []
            if parent:
                rows.append(("parent commit", parent[str(n)]["us"], parent[str(n)]["ms"], parent[str(n)]))
            for label, cauchy in (("all edges NONE", False), ("closures Cauchy, delta 6", True)):
                us, ms, res = robust_column(g, poses, n - 1, a.rounds, a.reps, cauchy)
                rows.append((label, us, ms, res))
            for label, us, ms, res in rows:
                say("  %-26s k_pg_edges<linearise> %.1f (%.1f) us; optimize %.1f (%.1f) ms, %d iterations, cost -> %.6g"
                    % ((label + ":",) + quartiles(us) + quartiles(ms) + (res["iterations"], float(res["chi2_final"]))))
            if parent:
                (p_med, p_iqr), (n_med, _) = quartiles(rows[0][1]), quartiles(rows[1][1])
                say("  all-NONE kernel against the parent: %+.1f us, allowed +%.1f us (the parent's interquartile range): %s"
                    % (n_med - p_med, p_iqr, "met" if n_med - p_med <= p_iqr else "NOT met"))
                say("  all-NONE optimize ends like the parent's (iterations, cost to the 6 digits of its report): %s"
                    % (rows[1][3]["iterations"] == rows[0][3]["iterations"] and "%.6g" % rows[1][3]["chi2_final"] == rows[0][3]["chi2_final"]))
    reg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--robust", action="store_true", help="the cost of the robust edges, used and unused (see above)")
    ap.add_argument("--parent-tree", default="", help="--robust: a built checkout of the parent commit, measured first in a child process")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if a.robust:
        robust_main(a, say)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    say("rgbd360_graph_*: HIP-event averages over %d launches in microseconds, whole calls in milliseconds, %d rounds in one process" % (a.reps, a.rounds))
    reg = RegisterPhotoICP()
    for n in [int(s) for s in a.sizes.split(",")]:
        poses, i, j, Z, Om = make_graph(n, np.random.default_rng(n))
        with PoseGraph(reg) as g:
            g.add_vertices(poses, fixed=[0])
            g.add_edges(i, j, Z, Om)
            say("N = %d vertices, E = %d edges" % (g.n_vertices, g.n_edges))
            for r in range(a.rounds):
                us = g.time_kernels(a.reps)
                say("  round %d: " % r + ", ".join("%s %.1f" % (k, v) for k, v in zip(KERNELS, us)))
            for r in range(a.rounds):
                g.set_poses(0, poses)
                t0 = time.perf_counter()
                res = g.optimize()
                ms = (time.perf_counter() - t0) * 1e3
                tr = g.trace()
                say("  optimize round %d: %.1f ms, status %d, %d iterations (%d accepted), %d conjugate-gradient iterations (%s per solve), chi2 %.6g -> %.6g"
                    % (r, ms, res["status"], res["iterations"], res["accepted"], res["cg_iterations"], "/".join(str(t["cg_iterations"]) for t in tr),
                       res["chi2_initial"], res["chi2_final"]))
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
