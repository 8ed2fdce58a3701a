"""Marginal and relative pose covariances of rgbd360_graph_marginals / rgbd360_graph_relative_covariances (include/rgbd360_hip.h, DESIGN.md
3.18) restated in float64 numpy on top of tests/pose_graph_reference.py and tests/pose_graph_robust_reference.py: the dense Gauss-Newton
matrix H of normal_equations (robust-weighted, disabled edges absent, as RobustGraph builds it), numpy.linalg.inv, the adjoint sandwich,
the variance factor, and -- separately -- a column-by-column restatement of the block-Jacobi conjugate gradients at lambda = 0 that the
device runs.  Nothing in this file calls the library."""
import functools
import json
import os

import numpy as np

import pose_graph_cases as cases
import pose_graph_reference as R
import pose_graph_robust_reference as RR

CG_TOL, CG_MAX_ITERS = 1e-10, 1000      # rgbd360_graph_default_cov_params
NOT_CONVERGED = 5                        # RGBD360_NOT_CONVERGED
DEVICE_FACTOR, DEVICE_FLOOR = 8.0, 1e-13      # what the device may add to the recorded error of the restatement
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_cov.json")
CASES = [(n, "noisy") for n in cases.NAMES] + [("n70", "consistent")]
ROBUST_CASE = "n70-cauchy-disabled"
ROBUST_DISABLED = (70, 72)               # one wrong closure and one good one of pose_graph_robust_reference.corrupted("n70")


def sym(M):
    return 0.5 * (M + M.T)


def dense(graph, T=None):
    """(Sigma = H^-1 [6F,6F], H, cost) at the poses T (default: the graph's)."""
    H, _, cost = graph.normal_equations(T)
    return np.linalg.inv(H), H, cost


def block(graph, S, a, b):
    """The 6x6 block (a, b) of a matrix over the free vertices; zero when a or b is fixed or isolated."""
    sa, sb = graph.slot[a], graph.slot[b]
    if sa < 0 or sb < 0:
        return np.zeros((6, 6))
    return S[6 * sa:6 * sa + 6, 6 * sb:6 * sb + 6]


def rhs(graph, i, j):
    """B [6F,6] = E_j - E_i; i = None: E_j.  A fixed or isolated end contributes nothing."""
    B = np.zeros((6 * len(graph.free), 6))
    if graph.slot[j] >= 0:
        B[6 * graph.slot[j]:6 * graph.slot[j] + 6] += np.eye(6)
    if i is not None and graph.slot[i] >= 0:
        B[6 * graph.slot[i]:6 * graph.slot[i] + 6] -= np.eye(6)
    return B


def sandwich(graph, M, i, T=None):
    Ad = R.adjoint(R.rigid_inv((graph.T if T is None else T)[i]))
    return Ad @ M @ Ad.T


def marginal(graph, Sigma, v):
    return sym(block(graph, Sigma, v, v))


def relative(graph, Sigma, i, j, T=None):
    """C_ij = Ad(T_i^-1) (Sigma_ii + Sigma_jj - Sigma_ij - Sigma_ji) Ad(T_i^-1)^T."""
    if i == j:
        return np.zeros((6, 6))
    D = block(graph, Sigma, i, i) + block(graph, Sigma, j, j) - block(graph, Sigma, i, j) - block(graph, Sigma, j, i)
    return sym(sandwich(graph, D, i, T))


def variance_factor(graph, T=None):
    """(cost, dof, cost / dof or 1): dof = 6 (enabled edges) - 6 (free vertices)."""
    cost = graph.chi2(T)
    n_edges = int(graph.enabled.sum()) if hasattr(graph, "enabled") else len(graph.ei)
    dof = 6 * n_edges - 6 * len(graph.free)
    return cost, dof, (cost / dof if dof > 0 else 1.0)


def pcg_block(H, B, cg_tol=CG_TOL, cg_max_iters=CG_MAX_ITERS):
    """H X = B column by column with pose_graph_reference.pcg at lambda = 0.  Returns (X, iterations [6], |r|_M / |r0|_M [6])."""
    X, its, res = np.zeros_like(B), [], []
    for c in range(B.shape[1]):
        X[:, c], it, rr = R.pcg(H, -B[:, c], 0.0, cg_tol, cg_max_iters)
        its.append(it)
        res.append(rr)
    return X, np.array(its), np.array(res)


def marginal_pcg(graph, H, v, **kw):
    """(Sigma_vv, iterations, residual) the way the device computes it: B^T X of one block solve."""
    B = rhs(graph, None, v)
    if not B.any():
        return np.zeros((6, 6)), 0, 0.0
    X, its, res = pcg_block(H, B, **kw)
    return sym(B.T @ X), int(its.max()), float(res.max())


def relative_pcg(graph, H, i, j, T=None, **kw):
    B = rhs(graph, i, j)
    if i == j or not B.any():
        return np.zeros((6, 6)), 0, 0.0
    X, its, res = pcg_block(H, B, **kw)
    return sym(sandwich(graph, B.T @ X, i, T)), int(its.max()), float(res.max())


def error(C_hat, C):
    """max |C_hat_ab - C_ab| / sqrt(C_aa C_bb) over the entries of one block; C must have a positive diagonal."""
    d = np.sqrt(np.diag(C))
    return float((np.abs(np.asarray(C_hat) - C) / np.outer(d, d)).max())


def queries(graph):
    """(marginal vertices, relative pairs) of the accuracy checks: {first free, middle, last, a fixed one, the isolated one} and
    {(0, last), (middle, last), (last, middle), (v, v), one chain pair}; middle and last are free vertices."""
    free = graph.free
    first, mid, last = int(free[0]), int(free[len(free) // 2]), int(free[-1])
    verts = [first, mid, last, int(np.flatnonzero(graph.user_fixed)[-1])] + [int(v) for v in np.flatnonzero(graph.isolated)[:1]]
    pairs = [(0, last), (mid, last), (last, mid), (mid, mid), (last - 1, last)]
    return verts, pairs


@functools.lru_cache(maxsize=None)
def case_graph(name, form):
    """The reference graph of a case at the float32 rounding of the reference optimum (what rgbd360_graph_set_poses hands the device), and
    those poses [N,4,4] float32."""
    if name == ROBUST_CASE:
        enabled = np.ones(len(RR.corrupted("n70")[0]["ei"]), bool)
        enabled[list(ROBUST_DISABLED)] = False
        g = RR.graph("n70", RR.CAUCHY, enabled)
        poses = RR.stored_optimum("n70", RR.CAUCHY).astype(np.float32)
    else:
        g = cases.reference_graph(cases.case(name, form))
        poses = cases.reference_optimum(name, form)[0].astype(np.float32)
    g.T = poses.astype(np.float64)
    g.T.setflags(write=False)
    poses.setflags(write=False)
    return g, poses


@functools.lru_cache(maxsize=None)
def case_dense(name, form):
    """(graph, poses, Sigma, H, marginals {v: block}, relatives {(i, j): block}) of a case, computed once per process."""
    g, poses = case_graph(name, form)
    Sigma, H, _ = dense(g)
    verts, pairs = queries(g)
    return g, poses, Sigma, H, {v: marginal(g, Sigma, v) for v in verts}, {p: relative(g, Sigma, *p) for p in pairs}


def restatement_error(name, form):
    """The error of the numpy PCG restatement against the dense inverse over the case's queried blocks, at the defaults:
    (error, largest iteration count, largest residual)."""
    g, _, _, H, marg, rel = case_dense(name, form)
    worst, its, res = 0.0, 0, 0.0
    for v, want in marg.items():
        got, it, rr = marginal_pcg(g, H, v)
        its, res = max(its, it), max(res, rr)
        if want.any():
            worst = max(worst, error(got, want))
        else:
            assert not got.any()
    for (i, j), want in rel.items():
        got, it, rr = relative_pcg(g, H, i, j)
        its, res = max(its, it), max(res, rr)
        if want.any():
            worst = max(worst, error(got, want))
        else:
            assert not got.any()
    return worst, its, res


def case_id(name, form):
    return name if name == ROBUST_CASE else "%s-%s" % (name, form)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def device_bound(name, form):
    """What a device block may differ from the dense inverse by, in the measure of error(): 8 x the recorded error of the restatement plus
    1e-13.  The device adds edges in CSR order and scalars in workgroup rows where numpy adds dense rows, and conjugate gradients carry
    such differences through their few hundred iterations; measured against the reference, never against the device."""
    return DEVICE_FACTOR * golden()[case_id(name, form)]["error"] + DEVICE_FLOOR
