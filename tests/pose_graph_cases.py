"""The graphs of the pose-graph tests (tests/test_pose_graph_cpu.py, tests/test_pose_graph_gpu.py): the smallest that reach every code
path of csrc/pose_graph.h, each in a consistent and a noisy form.  Built once per process and never modified."""
import functools

import numpy as np

import pose_graph_reference as R

NAMES = ("n2", "ring5", "n70", "n300", "variant")      # optimised; "far" (n70's topology around |t| = 90 m) is for the per-edge checks only
FORMS = ("consistent", "noisy")


def _trajectory(rng, n, offset):
    """n float64 poses of a wandering walk (0.1 m and a few degrees per step: keyframes of an indoor sequence) starting at `offset`."""
    T = [np.eye(4)]
    T[0][:3, 3] = offset
    T[0] = R.se3_exp(np.concatenate([np.zeros(3), rng.uniform(-0.5, 0.5, 3)])) @ T[0]
    for _ in range(n - 1):
        step = np.concatenate([[0.1, 0.0, 0.0] + rng.normal(0, 0.02, 3), rng.normal(0, 0.06, 3)])
        T.append(T[-1] @ R.se3_exp(step))
    return np.stack(T)


def _topology(name, rng):
    """(n, fixed indices, [(i, j)], isolated count)."""
    if name == "n2":
        return 2, [0], [(0, 1)]
    if name == "ring5":
        return 5, [0], [(k, k + 1) for k in range(4)] + [(4, 0)]
    if name in ("n70", "far"):      # more than one wave: 69 + 12 = 81 edges
        e = [(k, k + 1) for k in range(69)]
        while len(e) < 81:
            i, j = sorted(rng.choice(70, 2, replace=False).tolist())
            if j - i > 1 and (i, j) not in e:
                e.append((i, j))
        return 70, [0], e
    # more than one 256-thread workgroup, several partial rows, one long CSR row: 299 + 40 + 100 = 439 edges
    e = [(k, k + 1) for k in range(299)]
    while len(e) < 339:
        i, j = sorted(rng.choice(300, 2, replace=False).tolist())
        if j - i > 1 and (i, j) not in e:
            e.append((i, j))
    e += [(0, int(v)) for v in rng.choice(np.arange(2, 300), 100, replace=False)]
    if name == "n300":
        return 300, [0], e
    # two fixed vertices, an isolated vertex (300), a duplicated edge, and every third closure stored with from > to
    e = [(j, i) if (k >= 299 and k % 3 == 0) else (i, j) for k, (i, j) in enumerate(e)]
    e.append(e[310])
    return 301, [0, 150], e


@functools.lru_cache(maxsize=None)
def case(name, form):
    """dict: gt [N,4,4] float64, poses [N,4,4] float32 (the start), fixed [N] bool, ei, ej, Z [E,4,4] float32, Om [E,6,6] float32 or None,
    extent (max |t| of the ground truth)."""
    rng = np.random.default_rng({"n2": 2, "ring5": 5, "n70": 70, "far": 71, "n300": 300, "variant": 301}[name] + (1000 if form == "noisy" else 0))
    n, fixed_idx, edges = _topology(name, np.random.default_rng(7))
    gt = _trajectory(rng, n, [60.0, -50.0, 20.0] if name == "far" else [1.0, 2.0, 0.5])
    fixed = np.zeros(n, bool)
    fixed[fixed_idx] = True
    ei = np.array([e[0] for e in edges], np.int32)
    ej = np.array([e[1] for e in edges], np.int32)
    rel = np.stack([R.rigid_inv(gt[i]) @ gt[j] for i, j in edges])      # frame j in frame i
    if form == "consistent":
        Z = rel.astype(np.float32)
        Om = None
        start = gt.copy()
        for v in range(n):
            if not fixed[v]:
                d = np.concatenate([rng.uniform(-0.1, 0.1, 3) / np.sqrt(3), rng.uniform(-0.05, 0.05, 3) / np.sqrt(3)])
                start[v] = R.se3_exp(d) @ gt[v]
    else:
        Z = np.stack([R.se3_exp(np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.01, 3)])) @ z for z in rel]).astype(np.float32)
        Om = []
        for _ in edges:
            Q, _r = np.linalg.qr(rng.normal(size=(6, 6)))
            Om.append((Q * rng.uniform(0.5e4, 2e4, 6)) @ Q.T)
        Om = np.stack(Om).astype(np.float32)
        start = gt.copy()      # chained odometry from vertex 0 along the edges k -> k + 1; the other fixed vertices keep the truth
        for k in range(n - 1):
            chain = [e for e, (i, j) in enumerate(edges) if (i, j) == (k, k + 1)]
            if chain and not fixed[k + 1]:
                start[k + 1] = start[k] @ Z[chain[0]].astype(np.float64)
    out = dict(name=name, form=form, gt=gt, poses=start.astype(np.float32), fixed=fixed, ei=ei, ej=ej, Z=Z, Om=Om,
               extent=float(np.abs(gt[:, :3, 3]).max()))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def reference_graph(c):
    return R.Graph(c["poses"], c["fixed"], c["ei"], c["ej"], c["Z"], c["Om"])


OPT = dict(max_iters=40, cg_tol=1e-8, cg_max_iters=400, tol_update=1e-10)      # the optimiser settings of the tests


@functools.lru_cache(maxsize=None)
def reference_optimum(name, form, solver="dense"):
    """(poses [N,4,4] float64, result, trace) of the numpy reference at the test settings."""
    T, res, trace = R.optimize(reference_graph(case(name, form)), solver=solver, **OPT)
    T.setflags(write=False)
    return T, res, trace


def truth_bound(c):
    """How far a pose entry of the optimum of a CONSISTENT graph may lie from the ground truth.  Every Z entry carries a relative float32
    rounding of 2^-24: per edge a rotation error below 2^-23 rad and a translation error below 2^-24 |t_edge|.  Along a path of L edges
    these add up to at most L 2^-23 rad, which moves a position by at most that times the lever arm (the extent of the trajectory), and the
    closures only average them.  With L <= N: N 2^-23 (1 + extent), the rounding of the fixed poses included."""
    return len(c["gt"]) * 2.0 ** -23 * (1.0 + c["extent"])


def chi2_floor(ref):
    """Per edge, what float64 rounding alone does to r^T Omega r: r carries an absolute error of about eps x 10^2 operations at the
    magnitude of the poses (the model behind the 1e-9 bound on r, without its margin of 10^3), which moves the term by 2 |Omega r| times
    that.  It matters only where chi2 is itself zero up to rounding -- a tree started from its own chained odometry -- and a relative bound
    says nothing; everywhere else it is far below 1e-10 chi2."""
    eps_r = 100 * 2.0 ** -52 * max(1.0, float(np.abs(ref.T[:, :3, 3]).max()))
    r = ref.linearize()[0]
    return np.array([2.0 * np.linalg.norm(ref.Om[e] @ r[e]) * eps_r for e in range(len(r))])
