"""The pose-graph optimiser of rgbd360_graph_* (include/rgbd360_hip.h) restated in float64 numpy: the SE(3) pieces of
csrc/gn_math.h, the per-edge linearisation, a dense Hessian, Levenberg-Marquardt with an exact numpy.linalg.solve, and -- separately --
the block-Jacobi preconditioned conjugate gradients the device runs.  Poses are 4x4 row-major numpy arrays here (world <- frame); an
edge is (i, j, Z, Omega) with Z = frame j in frame i.  Nothing in this file calls the library."""
import numpy as np


def hat(u):
    return np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])


def se3_exp(x):
    """gn::se3_exp: the full exponential, tangent (v; w), with its small-angle branches."""
    x = np.asarray(x, np.float64)
    u, w = x[:3], x[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    cx = np.cross(w, u)
    if th2 < 1e-8:
        B = 0.5
        A = 1.0 - th2 / 6.0
        t = u + 0.5 * cx
    else:
        if th2 < 1e-6:
            Cc = (1.0 / 6.0) * (1.0 - th2 / 20.0)
            A = 1.0 - th2 * Cc
            B = 0.5 - 0.25 * (1.0 / 6.0) * th2
        else:
            A = np.sin(th) / th
            B = (1.0 - np.cos(th)) / th2
            Cc = (1.0 - A) / th2
        t = u + B * cx + Cc * np.cross(w, cx)
    W = hat(w)
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + A * W + B * (W @ W)
    E[:3, 3] = t
    return E


def se3_log(E):
    """gn::se3_log."""
    E = np.asarray(E, np.float64)
    R, t = E[:3, :3], E[:3, 3]
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt(a @ a)
    c = 0.5 * (np.trace(R) - 1.0)
    angle = np.arctan2(s, c)
    if s >= 1e-4:
        w = (angle / s) * a
    elif c > 0.0:
        w = (1.0 + s * s / 6.0) * a
    else:
        d = np.diag(R) - c
        k = int(np.argmax(d))
        om = 1.0 - c
        n = np.zeros(3)
        n[k] = np.sqrt(max(d[k], 0.0) / om)
        for m in range(3):
            if m != k:
                n[m] = 0.5 * (R[k, m] + R[m, k]) / (om * n[k]) if n[k] > 0.0 else 0.0
        w = (-1.0 if n @ a < 0.0 else 1.0) * angle * n
    th2 = float(w @ w)
    if th2 < 1e-2:
        D = ((th2 / 1209600.0 + 1.0 / 30240.0) * th2 + 1.0 / 720.0) * th2 + 1.0 / 12.0
    else:
        th = np.sqrt(th2)
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / th2
        D = (1.0 - A / (2.0 * B)) / th2
    cx = np.cross(w, t)
    return np.concatenate([t - 0.5 * cx + D * np.cross(w, cx), w])


def rigid_inv(T):
    I = np.eye(4)
    I[:3, :3] = T[:3, :3].T
    I[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return I


def adjoint(T):
    R, t = T[:3, :3], T[:3, 3]
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = R
    Ad[:3, 3:] = hat(t) @ R
    Ad[3:, 3:] = R
    return Ad


def ad(r):
    M = np.zeros((6, 6))
    M[:3, :3] = hat(r[3:])
    M[:3, 3:] = hat(r[:3])
    M[3:, 3:] = hat(r[3:])
    return M


def jl_inv(r):
    """gn::se3_jl_inv: the series I - ad/2 + ad^2/12 - ad^4/720 + ad^6/30240."""
    a = ad(np.asarray(r, np.float64))
    a2 = a @ a
    a4 = a2 @ a2
    return np.eye(6) - 0.5 * a + a2 / 12.0 - a4 / 720.0 + (a4 @ a2) / 30240.0


def sym(Om):
    Om = np.asarray(Om, np.float64)
    return 0.5 * (Om + Om.T)


def edge_terms(Ti, Tj, Z):
    """(r, A) of one edge: r = log(Z Tj^-1 Ti), A = dr/dx_i = J_l^-1(r) Ad(Z Tj^-1); dr/dx_j = -A."""
    M = np.asarray(Z, np.float64) @ rigid_inv(Tj)
    r = se3_log(M @ Ti)
    return r, jl_inv(r) @ adjoint(M)


class Graph:
    """poses [N,4,4] float64 (the float32 inputs widened), fixed [N] bool, edges: i [E], j [E], Z [E,4,4], Om [E,6,6]."""

    def __init__(self, poses, fixed, ei, ej, Z, Om=None):
        self.T = np.array(poses, np.float32).astype(np.float64)
        self.n = len(self.T)
        self.ei = np.asarray(ei, np.int64).reshape(-1)
        self.ej = np.asarray(ej, np.int64).reshape(-1)
        self.Z = np.array(Z, np.float32).astype(np.float64).reshape(-1, 4, 4)
        E = len(self.ei)
        self.Om = np.tile(np.eye(6), (E, 1, 1)) if Om is None else np.stack([sym(np.array(o, np.float32)) for o in Om]) if E else np.zeros((0, 6, 6))
        deg = np.zeros(self.n, np.int64)
        np.add.at(deg, self.ei, 1)
        np.add.at(deg, self.ej, 1)
        self.user_fixed = np.asarray(fixed, bool).copy()
        self.isolated = (deg == 0) & ~self.user_fixed
        self.fixed = self.user_fixed | (deg == 0)
        self.free = np.flatnonzero(~self.fixed)
        self.slot = -np.ones(self.n, np.int64)
        self.slot[self.free] = np.arange(len(self.free))

    def linearize(self, T=None):
        T = self.T if T is None else T
        E = len(self.ei)
        r, A = np.zeros((E, 6)), np.zeros((E, 6, 6))
        for e in range(E):
            r[e], A[e] = edge_terms(T[self.ei[e]], T[self.ej[e]], self.Z[e])
        return r, A

    def chi2(self, T=None, per_edge=False):
        T = self.T if T is None else T
        r = self.linearize(T)[0]
        c = np.array([r[e] @ self.Om[e] @ r[e] for e in range(len(self.ei))])
        return (float(c.sum()), c) if per_edge else float(c.sum())

    def normal_equations(self, T=None):
        """Dense H [6F,6F] and g [6F] over the free vertices, and chi2."""
        r, A = self.linearize(T)
        F = len(self.free)
        H, g = np.zeros((6 * F, 6 * F)), np.zeros(6 * F)
        chi2 = float(np.array([r[e] @ self.Om[e] @ r[e] for e in range(len(self.ei))]).sum())      # Graph.chi2's expression
        for e in range(len(self.ei)):
            W = A[e].T @ self.Om[e] @ A[e]
            b = A[e].T @ self.Om[e] @ r[e]
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
        return H, g, chi2

    def apply_update(self, x, T=None):
        T = self.T if T is None else T
        out = T.copy()
        for k, v in enumerate(self.free):
            out[v] = se3_exp(x[6 * k:6 * k + 6]) @ T[v]
        return out


def pcg(H, g, lam, cg_tol, cg_max_iters):
    """Solves (H + lam diag H) x = -g by conjugate gradients preconditioned with the inverse of the damped 6x6 diagonal blocks.
    Returns (x, iterations, |r|_M / |r0|_M)."""
    n = len(g)
    Hd = H + lam * np.diag(np.diag(H))
    Minv = np.zeros_like(H)
    for k in range(0, n, 6):
        Minv[k:k + 6, k:k + 6] = np.linalg.inv(Hd[k:k + 6, k:k + 6])
    x = np.zeros(n)
    r = -g.copy()
    z = Minv @ r
    p = z.copy()
    rz = rz0 = float(r @ z)
    it = 0
    if not rz0 > 0.0:
        return x, 0, 0.0
    while it < cg_max_iters:
        q = Hd @ p
        pq = float(p @ q)
        if not pq > 0.0:
            break
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        z = Minv @ r
        rz_new = float(r @ z)
        it += 1
        if not np.sqrt(max(rz_new, 0.0)) > cg_tol * np.sqrt(rz0):
            rz = rz_new
            break
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, it, float(np.sqrt(max(rz, 0.0) / rz0))


def optimize(graph, max_iters=10, tol_update=1e-6, lambda_init=1e-3, lambda_max=1e30, solver="dense", cg_tol=1e-8, cg_max_iters=400):
    """The Levenberg-Marquardt loop of the definition.  Returns (poses [N,4,4] float64, result dict, trace list)."""
    T = graph.T.copy()
    lam = lambda_init
    res = dict(status=0, iterations=0, accepted=0, converged=0, cg_iterations=0, n_fixed=int(graph.user_fixed.sum()), n_isolated=int(graph.isolated.sum()))
    trace = []
    chi2 = graph.chi2(T)
    res["chi2_initial"] = chi2
    if len(graph.free) == 0 or len(graph.ei) == 0:
        res.update(chi2_final=chi2, lambda_final=lam)
        return T, res, trace
    for it in range(max_iters):
        H, g, chi2 = graph.normal_equations(T)
        d = np.diag(H)
        ok = True
        for k in range(0, len(g), 6):
            try:
                np.linalg.cholesky(H[k:k + 6, k:k + 6] + lam * np.diag(d[k:k + 6]))
            except np.linalg.LinAlgError:
                ok = False
        if not ok:
            res["status"] = 1
            break
        if solver == "dense":
            x, cg_it, cg_res = np.linalg.solve(H + lam * np.diag(d), -g), 0, 0.0
        else:
            x, cg_it, cg_res = pcg(H, g, lam, cg_tol, cg_max_iters)
        Tt = graph.apply_update(x, T)
        chi2_t = graph.chi2(Tt)
        acc = bool(chi2_t < chi2)
        max_x = float(np.abs(x).max())
        trace.append(dict(chi2=chi2, chi2_trial=chi2_t, lam=lam, accepted=int(acc), cg_iterations=cg_it, cg_residual=cg_res, max_update=max_x))
        res["iterations"] += 1
        res["cg_iterations"] += cg_it
        if acc:
            T = Tt
            chi2 = chi2_t
            res["accepted"] += 1
            lam = max(lam / 10.0, 1e-9)
            if max_x <= tol_update:
                res["converged"] = 1
                break
        else:
            lam *= 10.0
            if lam > lambda_max:
                res["status"] = 1
                break
    res.update(chi2_final=graph.chi2(T), lambda_final=lam)
    return T, res, trace
