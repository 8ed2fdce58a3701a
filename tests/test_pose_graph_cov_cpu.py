"""CPU tests of the covariance definitions (rgbd360_graph_marginals / rgbd360_graph_relative_covariances, include/rgbd360_hip.h, DESIGN.md
3.18) on the numpy restatement tests/pose_graph_cov_reference.py: what a marginal and a relative covariance ARE, in which tangent they live,
and that the stored golden bound is what a fresh computation gives.  Nothing here calls the library."""
import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_cov_reference as CR
import pose_graph_reference as R
import pose_graph_robust_reference as RR


def rotations(Z):
    """Z with every rotation block replaced by the nearest rotation: a float32 Z is orthogonal to 1e-7 only, and the rigid inverse of the
    residual takes it to be exact."""
    Z = np.array(Z, np.float64)
    for z in Z:
        U, _, Vt = np.linalg.svd(z[:3, :3])
        z[:3, :3] = U @ Vt
    return Z


def chained(c):
    """float64 poses of the odometry chain k -> k + 1 from vertex 0: every chain residual is zero up to rounding."""
    Z = rotations(c["Z"][:69])
    T = [rotations(c["poses"][:1])[0]]
    for k in range(len(c["poses"]) - 1):
        T.append(T[-1] @ Z[k])
    return np.stack(T)


def tree(c, Om=None, n_edges=69):
    g = R.Graph(c["poses"], c["fixed"], c["ei"][:n_edges], c["ej"][:n_edges], c["Z"][:n_edges], Om)
    g.Z = rotations(g.Z)
    return g


def test_n2_marginal_is_the_inverse_of_the_edge_hessian():
    g = cases.reference_graph(cases.case("n2", "noisy"))
    _, A = g.linearize()
    Sigma, H, _ = CR.dense(g)
    want = np.linalg.inv(A[0].T @ g.Om[0] @ A[0])      # vertex 1 is the `to` end: H_11 = (-A)^T Omega (-A)
    got = CR.marginal(g, Sigma, 1)
    assert CR.error(got, CR.sym(want)) <= 1e-12
    assert not CR.marginal(g, Sigma, 0).any()           # the fixed vertex
    got_pcg, it, res = CR.marginal_pcg(g, H, 1)
    assert it == 1 and res <= CR.CG_TOL and CR.error(got_pcg, got) <= 1e-12      # block-Jacobi is exact on one free vertex


@pytest.mark.parametrize("information", ["identity", "noisy"])
def test_tree_relative_covariance_is_the_edge_covariance(information):
    """On a tree with zero residuals H = J^T Omega J with a square J, so the covariance of every edge's residual is Omega_e^-1; C_ij is
    that covariance only if it lives in the residual's tangent: the A's cancel because A = Ad(Z T_j^-1) = Ad(T_i^-1) there."""
    c = cases.case("n70", "consistent")
    Om = None if information == "identity" else cases.case("n70", "noisy")["Om"][:69]
    g = tree(c, Om)
    T = chained(c)
    assert np.abs(g.linearize(T)[0]).max() < 1e-12
    Sigma, _, _ = CR.dense(g, T)
    for k in range(69):
        want = np.linalg.inv(g.Om[k])
        got = CR.relative(g, Sigma, k, k + 1, T)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), k


def test_closures_add_information():
    c = cases.case("n70", "consistent")
    T = chained(c)
    g_tree, g_full = tree(c), tree(c, n_edges=81)
    S_tree, S_full = CR.dense(g_tree, T)[0], CR.dense(g_full, T)[0]
    for k in range(69):
        a, b = CR.relative(g_tree, S_tree, k, k + 1, T), CR.relative(g_full, S_full, k, k + 1, T)
        assert np.linalg.eigvalsh(a - b).min() >= -1e-12 * np.linalg.norm(a, 2), k
    v = 69      # and the end of the chain, far from the fixed vertex, is known better
    d = CR.marginal(g_tree, S_tree, v) - CR.marginal(g_full, S_full, v)
    assert np.linalg.eigvalsh(d).min() >= -1e-12 * np.linalg.norm(CR.marginal(g_tree, S_tree, v), 2)
    assert np.linalg.eigvalsh(d).max() > 0.0


def test_fixed_from_and_zero_blocks():
    g, _, Sigma, H, _, _ = CR.case_dense("variant", "noisy")
    j = int(g.free[-1])
    for i in (0, 150):      # both fixed
        Ad = R.adjoint(R.rigid_inv(g.T[i]))
        want = CR.sym(Ad @ CR.block(g, Sigma, j, j) @ Ad.T)
        assert np.array_equal(CR.relative(g, Sigma, i, j), want)
        got, it, res = CR.relative_pcg(g, H, i, j)
        assert CR.error(got, want) <= CR.device_bound("variant", "noisy")
    assert not CR.relative(g, Sigma, 0, 150).any() and not CR.relative(g, Sigma, j, j).any()
    assert not CR.marginal(g, Sigma, 300).any() and CR.relative_pcg(g, H, 0, 150)[1:] == (0, 0.0)
    # a free `from` and a fixed `to`: the marginal of `from` in its own frame
    Ad = R.adjoint(R.rigid_inv(g.T[j]))
    assert np.allclose(CR.relative(g, Sigma, j, 0), CR.sym(Ad @ CR.block(g, Sigma, j, j) @ Ad.T), rtol=0, atol=0)


def test_a_disabled_edge_is_an_absent_edge():
    drop = list(CR.ROBUST_DISABLED)
    enabled = np.ones(len(RR.corrupted("n70")[0]["ei"]), bool)
    enabled[drop] = False
    a = RR.graph("n70", RR.NONE, enabled)
    c = RR.without("n70", drop)
    b = R.Graph(c["poses"], c["fixed"], c["ei"], c["ej"], c["Z"], c["Om"])
    Sa, Sb = CR.dense(a)[0], CR.dense(b)[0]
    assert np.array_equal(Sa, Sb)
    assert CR.variance_factor(a)[1] == CR.variance_factor(b)[1] == 6 * (81 - 2) - 6 * 69
    # and the robust weight enters H: a Cauchy closure with a large residual carries less information
    w = RR.graph("n70", RR.CAUCHY, enabled)
    Sw = CR.dense(w)[0]
    assert np.linalg.eigvalsh(Sw - Sa).min() >= -1e-12 * np.linalg.norm(Sa, 2) and np.linalg.eigvalsh(Sw - Sa).max() > 0.0


def test_variance_factor():
    g, _ = CR.case_graph("n70", "noisy")
    r, _ = g.linearize()
    cost = float(sum(r[e] @ g.Om[e] @ r[e] for e in range(81)))
    got = CR.variance_factor(g)
    assert got[1] == 6 * 81 - 6 * 69 and abs(got[0] - cost) <= 1e-12 * cost and abs(got[2] - cost / 72) <= 1e-12 * cost
    assert CR.variance_factor(cases.reference_graph(cases.case("n2", "noisy")))[1:] == (0, 1.0)      # dof = 0: the factor is 1
    assert CR.golden()["n70-noisy"]["dof"] == 72 and abs(CR.golden()["n70-noisy"]["variance_factor"] - got[2]) <= 1e-9 * got[2]


def test_relative_covariance_against_finite_differences():
    """xi(x) = log(T_i'^-1 T_j' (T_i^-1 T_j)^-1) with T' = apply_update(x): its Jacobian by central differences of step 1e-6 (error of order
    1e-12 from the step, 1e-10 from rounding) is Ad(T_i^-1) at x_j and minus that at x_i, and C_ij = J Sigma J^T."""
    g, _ = CR.case_graph("ring5", "noisy")
    T = rotations(g.T)      # (float32 poses are rotations to 1e-7 only, which the rigid inverse below would turn into an error of the check)
    Sigma = CR.dense(g, T)[0]
    F = len(g.free)
    h = 1e-6
    for i, j in ((1, 4), (3, 2), (0, 3)):
        rel0_inv = R.rigid_inv(R.rigid_inv(T[i]) @ T[j])
        J = np.zeros((6, 6 * F))
        for k in range(6 * F):
            x = np.zeros(6 * F)
            x[k] = h
            Tp, Tm = g.apply_update(x, T), g.apply_update(-x, T)
            J[:, k] = (R.se3_log(R.rigid_inv(Tp[i]) @ Tp[j] @ rel0_inv) - R.se3_log(R.rigid_inv(Tm[i]) @ Tm[j] @ rel0_inv)) / (2 * h)
        Ad = R.adjoint(R.rigid_inv(T[i]))
        want = np.zeros((6, 6 * F))
        want[:, 6 * g.slot[j]:6 * g.slot[j] + 6] = Ad
        if g.slot[i] >= 0:
            want[:, 6 * g.slot[i]:6 * g.slot[i] + 6] = -Ad
        assert np.abs(J - want).max() <= 1e-8 * np.abs(Ad).max(), (i, j)
        C_fd = J @ Sigma @ J.T
        assert CR.error(CR.sym(C_fd), CR.relative(g, Sigma, i, j, T)) <= 1e-7, (i, j)


def test_golden_file_covers_every_case_and_matches_a_fresh_computation():
    G = CR.golden()
    assert sorted(G) == sorted([CR.case_id(n, f) for n, f in CR.CASES] + [CR.ROBUST_CASE])
    for name, form in (("n2", "noisy"), ("ring5", "noisy"), ("n70", "consistent")):
        err, its, res = CR.restatement_error(name, form)
        rec = G[CR.case_id(name, form)]
        print(name, form, "error", err, "recorded", rec["error"], "iterations", its)
        assert err <= CR.device_bound(name, form)      # another BLAS may add in another order: the same allowance as the device
        assert its <= CR.CG_MAX_ITERS and res <= CR.CG_TOL
    for rec in G.values():
        assert 0.0 < rec["error"] <= 1e-8 and rec["cg_iterations_max"] < CR.CG_MAX_ITERS and rec["cg_residual_max"] <= CR.CG_TOL
