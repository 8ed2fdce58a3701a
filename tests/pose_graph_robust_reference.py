"""Robust and switchable edges of rgbd360_graph_* (include/rgbd360_hip.h) restated in float64 numpy on top of
tests/pose_graph_reference.py: the rho / w table, a Graph whose cost is the sum of rho over the enabled edges and whose normal equations
carry the first-order weight w (no second-derivative term), and the corrupted graphs the tests share.  pose_graph_reference.optimize
drives a RobustGraph unchanged.  Nothing in this file calls the library."""
import functools
import os

import numpy as np

import pose_graph_cases as cases
import pose_graph_reference as R

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3
KINDS = (HUBER, CAUCHY, GEMAN_MCCLURE)
KIND_NAMES = {NONE: "none", HUBER: "huber", CAUCHY: "cauchy", GEMAN_MCCLURE: "geman_mcclure"}


def rho_w(kind, delta, s):
    """(rho(s), w(s) = d rho / d s) of one edge, s = r^T Omega r.  Whenever not s > 0 every kind gives (s, 1)."""
    s = float(s)
    if kind == NONE or not s > 0.0:
        return s, 1.0
    d2 = float(delta) * float(delta)
    if kind == HUBER:
        if s <= d2:
            return s, 1.0
        q = np.sqrt(s)
        return 2.0 * delta * q - d2, delta / q
    if kind == CAUCHY:
        u = s / d2
        return d2 * np.log1p(u), 1.0 / (1.0 + u)
    if kind == GEMAN_MCCLURE:
        t = d2 / (d2 + s)
        return s * t, t * t
    raise ValueError("kind %r" % (kind,))


class RobustGraph(R.Graph):
    """pose_graph_reference.Graph with per edge a kind, a delta and an enabled flag.  A disabled edge adds nothing to cost, H or g and
    does not count toward a vertex's degree: a free vertex whose edges are all disabled is treated as fixed (and counted isolated)."""

    def __init__(self, poses, fixed, ei, ej, Z, Om=None, kinds=None, deltas=None, enabled=None):
        super().__init__(poses, fixed, ei, ej, Z, Om)
        E = len(self.ei)
        self.kinds = np.zeros(E, np.int64) if kinds is None else np.broadcast_to(np.asarray(kinds, np.int64), (E,)).copy()
        self.deltas = np.ones(E) if deltas is None else np.broadcast_to(np.asarray(deltas, np.float64), (E,)).copy()
        self.enabled = np.ones(E, bool) if enabled is None else np.broadcast_to(np.asarray(enabled, bool), (E,)).copy()
        deg = np.zeros(self.n, np.int64)
        np.add.at(deg, self.ei[self.enabled], 1)
        np.add.at(deg, self.ej[self.enabled], 1)
        self.isolated = (deg == 0) & ~self.user_fixed
        self.fixed = self.user_fixed | (deg == 0)
        self.free = np.flatnonzero(~self.fixed)
        self.slot = -np.ones(self.n, np.int64)
        self.slot[self.free] = np.arange(len(self.free))

    def edge_weights(self, T=None):
        """(cost, s [E], rho [E], w [E]); rho = w = 0 for a disabled edge, s is reported for every edge."""
        T = self.T if T is None else T
        E = len(self.ei)
        # r of pose_graph_reference.edge_terms without its Jacobian: the same operations, the same bits
        r = [R.se3_log(self.Z[e] @ R.rigid_inv(T[self.ej[e]]) @ T[self.ei[e]]) for e in range(E)]
        s = np.array([r[e] @ self.Om[e] @ r[e] for e in range(E)]).reshape(E)
        rho, w = np.zeros(E), np.zeros(E)
        for e in np.flatnonzero(self.enabled):
            rho[e], w[e] = rho_w(self.kinds[e], self.deltas[e], s[e])
        return float(rho.sum()), s, rho, w

    def chi2(self, T=None, per_edge=False):
        cost, s, _, _ = self.edge_weights(T)
        return (cost, s) if per_edge else cost

    def normal_equations(self, T=None):
        r, A = self.linearize(T)
        F = len(self.free)
        H, g = np.zeros((6 * F, 6 * F)), np.zeros(6 * F)
        cost = 0.0
        rho = np.zeros(len(self.ei))
        for e in np.flatnonzero(self.enabled):
            rho[e], w = rho_w(self.kinds[e], self.deltas[e], r[e] @ self.Om[e] @ r[e])
            W = w * (A[e].T @ self.Om[e] @ A[e])
            b = w * (A[e].T @ self.Om[e] @ r[e])
            a, c = self.slot[self.ei[e]], self.slot[self.ej[e]]
            if a >= 0:
                H[6 * a:6 * a + 6, 6 * a:6 * a + 6] += W
                g[6 * a:6 * a + 6] += b
            if c >= 0:
                H[6 * c:6 * c + 6, 6 * c:6 * c + 6] += W
                g[6 * c:6 * c + 6] -= b
            if a >= 0 and c >= 0:
                H[6 * a:6 * a + 6, 6 * c:6 * c + 6] -= W
                H[6 * c:6 * c + 6, 6 * a:6 * a + 6] -= W
        cost = float(rho.sum())      # edge_weights' expression
        return H, g, cost


# ---- the corrupted graphs of the tests: some closures of a noisy graph replaced by wrong ones
FIRST_CLOSURE = {"n70": 69, "n300": 299}
DELTA = 6.0
OPT = dict(max_iters=60, tol_update=1e-8, cg_tol=1e-8, cg_max_iters=400)      # the optimiser settings of every robust run
COMBOS = (("n70", HUBER), ("n70", CAUCHY), ("n70", GEMAN_MCCLURE), ("n300", HUBER), ("n300", CAUCHY))


@functools.lru_cache(maxsize=None)
def corrupted(name):
    """(case dict with the wrong closures in Z, bad edge indices).  Built once per process and never modified."""
    c = dict(cases.case(name, "noisy"))
    E = len(c["ei"])
    bad = list(range(FIRST_CLOSURE[name] + 1, E, 3))[:8]
    rng = np.random.default_rng(5)
    Z = c["Z"].copy()
    for e in bad:
        d = np.concatenate([rng.choice([-1, 1], 3) * rng.uniform(.5, 1, 3), rng.choice([-1, 1], 3) * rng.uniform(.2, .4, 3)])
        Z[e] = (R.se3_exp(d) @ Z[e].astype(np.float64)).astype(np.float32)
    Z.setflags(write=False)
    c["Z"] = Z
    return c, tuple(bad)


def closure_kinds(name, kind):
    """[E] kinds: `kind` on the closure edges, NONE on the odometry chain."""
    c, _ = corrupted(name)
    k = np.zeros(len(c["ei"]), np.int64)
    k[FIRST_CLOSURE[name]:] = kind
    return k


def graph(name, kind=NONE, enabled=None):
    c, _ = corrupted(name)
    return RobustGraph(c["poses"], c["fixed"], c["ei"], c["ej"], c["Z"], c["Om"], closure_kinds(name, kind), DELTA, enabled)


def without(name, drop):
    """The case built without the edges `drop`."""
    c, _ = corrupted(name)
    keep = np.setdiff1d(np.arange(len(c["ei"])), np.asarray(drop))
    return dict(c, ei=c["ei"][keep], ej=c["ej"][keep], Z=c["Z"][keep], Om=c["Om"][keep])


@functools.lru_cache(maxsize=None)
def optimum(name, kind, solver="dense"):
    """(poses, result, trace) of the reference on the corrupted graph, closures of `kind` (NONE: the quadratic optimiser)."""
    T, res, trace = R.optimize(graph(name, kind), solver=solver, **OPT)
    T.setflags(write=False)
    return T, res, trace


@functools.lru_cache(maxsize=None)
def clean_optimum(name):
    """The optimum of the graph without the wrong edges: what the recovery is measured against."""
    c = without(name, corrupted(name)[1])
    T, res, trace = R.optimize(R.Graph(c["poses"], c["fixed"], c["ei"], c["ej"], c["Z"], c["Om"]), **OPT)
    T.setflags(write=False)
    return T, res, trace


STORED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_robust_optima.npz")


@functools.lru_cache(maxsize=None)
def stored_optimum(name, what):
    """The dense optimum of COMBOS' (name, kind), or with what = "clean" clean_optimum(name), as tests/golden/make_golden_pose_graph_robust.py
    stored it: what the GPU tests compare with (tests/test_pose_graph_robust_cpu.py holds the file to a fresh computation)."""
    with np.load(STORED) as f:
        T = f["%s/%s" % (name, what if what == "clean" else KIND_NAMES[what])]
    T.setflags(write=False)
    return T


def distance(T, clean):
    """How far the poses T lie from `clean`, the optimum of the graph without the wrong edges: the largest difference of a pose entry,
    which on these graphs is a translation entry, in metres."""
    return float(np.abs(np.asarray(T, np.float64) - clean).max())
