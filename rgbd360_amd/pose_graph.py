"""Device pose-graph optimiser: the edges FrameStore.align returns go in, the poses VoxelMap.move_* takes come out.

Mirror of rgbd360_graph_* (include/rgbd360_hip.h, csrc/pose_graph.h): the reference's optimizer.addVertex / addEdge(nearestKF, newKF,
relPose, registerer.getInfoMat()) / optimizeGraph / getPoses (KFsphere_SLAM.cpp:262-265, 542-550, 630, 679-689) without g2o:

    graph = PoseGraph(reg)
    graph.add_vertices(odometry_poses, fixed=[0])
    poses, status, iters, results = store.align(pairs, guesses)
    graph.add_alignments([t for t, s in pairs], [s for t, s in pairs], poses, results)      # Z = pose, Omega = results[k].hessian
    res = graph.optimize()
    for k, T in enumerate(graph.poses()): gmap.move_sphere(rgb[k], depth[k], odometry_poses[k], T)

Poses are 4x4 numpy arrays world <- frame; an edge (i, j, Z) says Z = frame j in frame i.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from .register import Rgbd360Error, _ptr
from .voxel_map import _as_dict

ILL_POSED = 1     # RGBD360_ILL_POSED
NOT_CONVERGED = 5     # RGBD360_NOT_CONVERGED
ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE = 0, 1, 2, 3     # RGBD360_GRAPH_ROBUST_*


def _poses_cm(T, what):
    T = np.asarray(T, np.float32)
    if T.ndim == 2:
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != (4, 4):
        raise Rgbd360Error(f"PoseGraph.{what}: poses must be 4x4 (or n x 4 x 4)")
    return np.ascontiguousarray(T.transpose(0, 2, 1).reshape(-1))


class PoseGraph:
    def __init__(self, reg):
        """reg: the RegisterPhotoICP whose context (device, stream) the graph lives on; close() the graph before it."""
        self._L = _lib.load()
        self._reg = reg
        ctx = reg._ctx()
        h = C.c_void_p()
        rc = self._L.rgbd360_graph_create(ctx, C.byref(h))
        if rc != 0:
            raise Rgbd360Error(f"rgbd360_graph_create failed ({rc}): {self._L.rgbd360_last_error(ctx).decode()}")
        self._h = h
        self._ctx_value = ctx.value

    # ---- lifecycle
    def close(self):
        if self._h is not None:
            if self._reg._h is not None and self._reg._h.value == self._ctx_value:
                self._L.rgbd360_graph_destroy(self._h)
            else:
                warnings.warn("PoseGraph.close: the registration context was closed or recreated before the graph; its device memory is "
                              "not freed (close the graph first)", ResourceWarning, stacklevel=2)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if self._h is None:
            raise Rgbd360Error("PoseGraph is closed")
        if self._reg._h is None or self._reg._h.value != self._ctx_value:
            raise Rgbd360Error("PoseGraph: the registration context was closed or recreated (a setter was called) after the graph was made")
        return self._h

    def _check(self, rc: int):
        if rc < 0:
            raise Rgbd360Error(f"rgbd360_graph call failed ({rc}): {self._L.rgbd360_graph_last_error(self._h).decode()}")
        return rc

    # ---- the graph
    @property
    def n_vertices(self) -> int:
        return int(self._L.rgbd360_graph_n_vertices(self._handle()))

    @property
    def n_edges(self) -> int:
        return int(self._L.rgbd360_graph_n_edges(self._handle()))

    def clear(self):
        self._check(self._L.rgbd360_graph_clear(self._handle()))

    def add_vertices(self, poses, fixed=None) -> int:
        """poses: n x 4 x 4; fixed: None, n bool flags, or a list of indices into this call's poses.  Returns the index of the first new vertex."""
        p = _poses_cm(poses, "add_vertices")
        n = p.size // 16
        f = None
        if fixed is not None:
            fa = np.asarray(fixed)
            if fa.dtype == bool:
                f = np.ascontiguousarray(fa, np.uint8)
            else:
                f = np.zeros(n, np.uint8)
                idx = np.asarray(fa, np.int64).reshape(-1)
                if idx.size and (idx.min() < 0 or idx.max() >= n):
                    raise Rgbd360Error("PoseGraph.add_vertices: a fixed index is outside this call's poses")
                f[idx] = 1
            if f.shape != (n,):
                raise Rgbd360Error("PoseGraph.add_vertices: one fixed flag per pose")
        return self._check(self._L.rgbd360_graph_add_vertices(self._handle(), n, _ptr(p), None if f is None else _ptr(f)))

    def add_edges(self, frm, to, rel_poses, information=None):
        """Edges frm[k] -> to[k] with rel_poses[k] = frame to[k] in frame frm[k]; information: None (identity) or n x 6 x 6."""
        i = np.ascontiguousarray(np.asarray(frm).reshape(-1), np.int32)
        j = np.ascontiguousarray(np.asarray(to).reshape(-1), np.int32)
        z = _poses_cm(rel_poses, "add_edges") if i.size else np.zeros(0, np.float32)
        if not (i.size == j.size == z.size // 16):
            raise Rgbd360Error("PoseGraph.add_edges: one from, one to and one relative pose per edge")
        om = None
        if information is not None:
            I = np.asarray(information, np.float32).reshape(-1, 6, 6)
            if I.shape[0] != i.size:
                raise Rgbd360Error("PoseGraph.add_edges: one 6x6 information matrix per edge")
            om = np.ascontiguousarray(I.transpose(0, 2, 1).reshape(-1))
        self._check(self._L.rgbd360_graph_add_edges(self._handle(), int(i.size), _ptr(i), _ptr(j), _ptr(z), None if om is None else _ptr(om)))

    def add_alignments(self, trg, src, poses, results) -> int:
        """What FrameStore.align returned for the pairs (trg[k], src[k]) -- store entries = vertex indices -- as edges trg[k] -> src[k]:
        Z = poses[k], Omega = results[k].hessian.  Pairs whose status is not 0 are skipped; returns how many."""
        poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
        keep = [k for k in range(len(results)) if results[k].status == 0]
        if keep:
            H = np.stack([np.array(results[k].hessian, np.float32).reshape(6, 6).T for k in keep])
            self.add_edges([trg[k] for k in keep], [src[k] for k in keep], poses[keep], H)
        return len(results) - len(keep)

    def set_poses(self, first: int, poses):
        p = _poses_cm(poses, "set_poses")
        self._check(self._L.rgbd360_graph_set_poses(self._handle(), int(first), p.size // 16, _ptr(p)))

    def set_fixed(self, first: int, fixed):
        f = np.ascontiguousarray(np.asarray(fixed).reshape(-1), np.uint8)
        self._check(self._L.rgbd360_graph_set_fixed(self._handle(), int(first), int(f.size), _ptr(f)))

    # ---- robust and switchable edges
    def set_edge_robust(self, first: int, kinds, deltas=None):
        """Kind (ROBUST_*) and delta of the edges from `first` on; a scalar kind or delta is broadcast against the other.  deltas may be
        None only when every kind is ROBUST_NONE."""
        k = np.asarray(kinds, np.int32)
        d = None if deltas is None else np.asarray(deltas, np.float64)
        sizes = {a.size for a in (k, d) if a is not None and a.ndim}
        if len(sizes) > 1:
            raise Rgbd360Error("PoseGraph.set_edge_robust: one kind and one delta per edge (or scalars)")
        n = sizes.pop() if sizes else 1
        k = np.ascontiguousarray(np.broadcast_to(k.reshape(-1) if k.ndim else k, (n,)))
        if d is not None:
            d = np.ascontiguousarray(np.broadcast_to(d.reshape(-1) if d.ndim else d, (n,)))
        self._check(self._L.rgbd360_graph_set_edge_robust(self._handle(), int(first), int(n), _ptr(k), None if d is None else _ptr(d)))

    def set_edge_enabled(self, first: int, enabled):
        """Switches the edges from `first` on off (False) or on; a disabled edge adds nothing to the cost or the normal equations."""
        f = np.ascontiguousarray(np.asarray(enabled).reshape(-1) != 0, np.uint8)
        self._check(self._L.rgbd360_graph_set_edge_enabled(self._handle(), int(first), int(f.size), _ptr(f)))

    def edge_state(self):
        """(kinds [E] int32, deltas [E] float64, enabled [E] bool)."""
        E = self.n_edges
        k, d, f = np.zeros(max(E, 1), np.int32), np.zeros(max(E, 1), np.float64), np.zeros(max(E, 1), np.uint8)
        self._check(self._L.rgbd360_graph_get_edge_state(self._handle(), 0, E, _ptr(k), _ptr(d), _ptr(f)))
        return k[:E], d[:E], f[:E].astype(bool)

    def edge_weights(self):
        """(cost, s [E], rho [E], w [E]) float64 at the current poses: the raw s = r^T Omega r of every edge, the robust rho and the
        weight w = d rho / d s (both 0 for a disabled edge); cost is what chi2() returns."""
        E = self.n_edges
        c = C.c_double()
        s, rho, w = (np.zeros(max(E, 1), np.float64) for _ in range(3))
        self._check(self._L.rgbd360_graph_edge_weights(self._handle(), C.byref(c), _ptr(s), _ptr(rho), _ptr(w)))
        return c.value, s[:E], rho[:E], w[:E]

    def poses(self, first: int = 0, n=None) -> np.ndarray:
        """[n, 4, 4] float32."""
        n = self.n_vertices - int(first) if n is None else int(n)
        out = np.zeros(max(n, 0) * 16, np.float32)
        self._check(self._L.rgbd360_graph_get_poses(self._handle(), int(first), n, _ptr(out)))
        return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy()

    # ---- optimisation
    def params(self, **fields):
        """The defaults (max_iters 10, tol_update 1e-6, lambda_init 1e-3, lambda_max 1e30, cg_tol 1e-8, cg_max_iters 400) with the given
        fields replaced."""
        p = _lib.GraphParams()
        self._L.rgbd360_graph_default_params(C.byref(p))
        for name, v in fields.items():
            if not hasattr(p, name):
                raise TypeError(f"GraphParams has no field {name!r}")
            if v is not None:
                setattr(p, name, v)
        return p

    def optimize(self, **params) -> dict:
        """Runs the Levenberg-Marquardt loop on the device; returns the result struct as a dict (status, iterations, accepted, converged,
        chi2_initial, chi2_final, lambda_final, cg_iterations, n_fixed, n_isolated).  poses() then holds the optimised poses."""
        res = _lib.GraphResult()
        self._check(self._L.rgbd360_graph_optimize(self._handle(), C.byref(self.params(**params)), C.byref(res)))
        return _as_dict(res)

    def chi2(self, per_edge: bool = False):
        """The cost at the current poses (the sum of rho over the enabled edges); with per_edge also the [E] float64 raw terms
        r^T Omega r of every edge, enabled or not."""
        c = C.c_double()
        pe = np.zeros(max(self.n_edges, 1), np.float64) if per_edge else None
        self._check(self._L.rgbd360_graph_chi2(self._handle(), C.byref(c), None if pe is None else _ptr(pe)))
        return (c.value, pe[:self.n_edges]) if per_edge else c.value

    def trace(self):
        """One dict per Levenberg-Marquardt iteration of the last optimize: chi2, chi2_trial, lambda_, accepted, cg_iterations, cg_residual,
        max_update."""
        n = C.c_int()
        self._check(self._L.rgbd360_graph_get_trace(self._handle(), 0, C.byref(n), None))
        tr = (_lib.GraphIteration * max(n.value, 1))()
        self._check(self._L.rgbd360_graph_get_trace(self._handle(), n.value, None, tr))
        return [_as_dict(t) for t in tr[:n.value]]

    # ---- covariances
    def cov_params(self, **fields):
        """The defaults (cg_max_iters 1000, cg_tol 1e-10) with the given fields replaced."""
        p = _lib.GraphCovParams()
        self._L.rgbd360_graph_default_cov_params(C.byref(p))
        for name, v in fields.items():
            if not hasattr(p, name):
                raise TypeError(f"GraphCovParams has no field {name!r}")
            if v is not None:
                setattr(p, name, v)
        return p

    def _covariances(self, frm, to, params):
        j = np.ascontiguousarray(np.asarray(to).reshape(-1), np.int32)
        i = None if frm is None else np.ascontiguousarray(np.asarray(frm).reshape(-1), np.int32)
        if i is not None and i.size != j.size:
            raise Rgbd360Error("PoseGraph.relative_covariances: one from and one to per pair")
        n = int(j.size)
        cov = np.zeros((max(n, 1), 36), np.float64)
        its, rr = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64)
        res = _lib.GraphCovResult()
        p = self.cov_params(**params)
        if i is None:
            self._check(self._L.rgbd360_graph_marginals(self._handle(), n, _ptr(j), C.byref(p), _ptr(cov), _ptr(its), _ptr(rr), C.byref(res)))
        else:
            self._check(self._L.rgbd360_graph_relative_covariances(self._handle(), n, _ptr(i), _ptr(j), C.byref(p), _ptr(cov), _ptr(its), _ptr(rr),
                                                                   C.byref(res)))
        out = _as_dict(res)
        out["cg_iterations"], out["cg_residual"] = its[:n], rr[:n]
        if res.status != 0:
            out["message"] = self._L.rgbd360_graph_last_error(self._h).decode()
        return cov[:n].reshape(-1, 6, 6).transpose(0, 2, 1).copy(), out

    def marginals(self, vertices, **params):
        """(cov [n,6,6] float64, result dict): Sigma_vv, the 6x6 diagonal blocks of the inverse of the Gauss-Newton matrix at the current
        poses (lambda = 0, robust weights, disabled edges absent), in the update tangent (v; w); exact zeros for fixed and isolated
        vertices.  The result holds status (0, ILL_POSED, NOT_CONVERGED), n_queries, n_not_converged, cg_iterations_max, cg_residual_max,
        dof, cost, variance_factor (cost / dof: scale a covariance by it before gating on it), n_fixed, n_isolated, the per-query arrays
        cg_iterations and cg_residual, and `message` when the status is not 0.  params: cg_max_iters, cg_tol."""
        return self._covariances(None, vertices, params)

    def relative_covariances(self, from_, to, **params):
        """(cov [n,6,6] float64, result dict): C_ij = Ad(T_i^-1) (Sigma_ii + Sigma_jj - Sigma_ij - Sigma_ji) Ad(T_i^-1)^T of the pairs
        (from_[k], to[k]), the covariance of the left perturbation of T_i^-1 T_j -- the tangent of an edge (i, j, Z)'s residual, so
        commensurate with the inverse information of such an edge.  The result is that of marginals()."""
        return self._covariances(from_, to, params)

    # ---- diagnostics (rgbd360_hip_diag.h)
    def linearize(self):
        """(r [E,6], A [E,6,6]) float64 at the current poses."""
        E = self.n_edges
        r = np.zeros((max(E, 1), 6), np.float64)
        A = np.zeros((max(E, 1), 36), np.float64)
        self._check(self._L.rgbd360_graph_linearize(self._handle(), _ptr(r), _ptr(A)))
        return r[:E], A[:E].reshape(-1, 6, 6).transpose(0, 2, 1).copy()

    def apply(self, x, lam: float = 0.0) -> np.ndarray:
        """y = (H + lam diag H) x; x, y: [N, 6] float64 (rows of fixed and isolated vertices are read and written as 0)."""
        N = self.n_vertices
        x = np.ascontiguousarray(np.asarray(x, np.float64).reshape(N, 6))
        y = np.zeros((max(N, 1), 6), np.float64)
        self._check(self._L.rgbd360_graph_apply(self._handle(), float(lam), _ptr(x), _ptr(y)))
        return y[:N]

    def time_kernels(self, reps: int = 20) -> np.ndarray:
        out = np.zeros(10, np.float32)
        self._check(self._L.rgbd360_graph_time_kernels(self._handle(), int(reps), _ptr(out)))
        return out

    def time_cov_kernels(self, vertices, reps: int = 20) -> np.ndarray:
        """rgbd360_graph_time_cov_kernels: [8] float32 microseconds of the kernels of one covariance batch of up to 16 marginals."""
        v = np.ascontiguousarray(np.asarray(vertices).reshape(-1), np.int32)
        out = np.zeros(8, np.float32)
        self._check(self._L.rgbd360_graph_time_cov_kernels(self._handle(), int(v.size), _ptr(v), int(reps), _ptr(out)))
        return out
