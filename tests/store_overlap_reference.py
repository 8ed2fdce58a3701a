"""The record rgbd360_store_overlap must produce for one pair, restated with numpy from outputs a per-pair path already has: its warp
indices, its LUT and its target depth plane.  Nothing here runs a warp of its own.

Per source pixel i (include/rgbd360_overlap.h):
  n_valid       lut[i].x != -10000 (the kInvalidPoint test of the per-pixel pass, RPI.h:40)
  n_visible     idx[i] != (-1, -1)
  n_target      visible and D = depth_trg[idx[i]] finite (RPI.h:3064)
  classes       float32, every operation rounded on its own:  diff = range - D,  tol = tol_abs + tol_rel * D
                consistent |diff| <= tol,  behind diff > tol,  in_front -diff > tol
with range = sqrt((X X + Y Y) + Z Z) of the unfused R p + t (warp_images_reference.transformed, warp_images_reference.py:69).  That
is bit for bit the range of index arithmetic 1; arithmetic 0 forms X, Y, Z and d^2 with fused multiply-adds, so its range may differ
in the last bits and a point within `n_borderline` of a class boundary may change class.
"""
import numpy as np

from tests import warp_images_reference as W

F = np.float32
INVALID_POINT = F(-10000.0)
FIELDS = ("n_valid", "n_visible", "n_target", "n_consistent", "n_behind", "n_in_front")


def counts(idx, lut, depth_trg, pose, tol_abs=0.05, tol_rel=0.02):
    """idx (n, 2) int32 warp indices, lut (n, 3) float32 source points, depth_trg (rows, cols) float32, pose 4x4 (source in target).
    Returns a dict of the six counts plus n_borderline: the points with a finite D whose | |diff| - tol |, in float64, is at most
    1e-5 * max(D, range); and "sure": per class, the points of the class that are not borderline."""
    idx = np.asarray(idx)
    lut = np.asarray(lut, F)
    depth_trg = np.asarray(depth_trg, F)
    tol_abs, tol_rel = F(tol_abs), F(tol_rel)
    valid = lut[:, 0] != INVALID_POINT
    vis = idx[:, 0] >= 0
    X, Y, Z = W.transformed(lut, pose)
    with np.errstate(invalid="ignore", over="ignore"):
        rng = np.sqrt(((X * X + Y * Y) + Z * Z).astype(F)).astype(F)
        D = np.full(idx.shape[0], np.nan, F)
        D[vis] = depth_trg[idx[vis, 0], idx[vis, 1]]
        target = vis & np.isfinite(D)
        diff = (rng - D).astype(F)
        tol = (tol_abs + (tol_rel * D).astype(F)).astype(F)
        consistent = target & (np.abs(diff) <= tol)
        behind = target & (diff > tol)
        in_front = target & (-diff > tol)
        margin = np.abs(np.abs(diff.astype(np.float64)) - tol.astype(np.float64))
        borderline = target & (margin <= 1e-5 * np.maximum(D.astype(np.float64), rng.astype(np.float64)))
    out = dict(n_valid=int(valid.sum()), n_visible=int(vis.sum()), n_target=int(target.sum()), n_consistent=int(consistent.sum()),
               n_behind=int(behind.sum()), n_in_front=int(in_front.sum()), n_borderline=int(borderline.sum()))
    out["sure"] = dict(n_consistent=int((consistent & ~borderline).sum()), n_behind=int((behind & ~borderline).sum()),
                       n_in_front=int((in_front & ~borderline).sum()))
    return out


def from_context(ctx, level, pose, tol_abs=0.05, tol_rel=0.02):
    """ctx: anything with warp_indices(level, pose), lut(level) and plane("depth_trg", level) for a pair of frames it holds -- a
    RegisterPhotoICP context or the CPU oracle."""
    return counts(ctx.warp_indices(level, pose), ctx.lut(level), ctx.plane("depth_trg", level), pose, tol_abs, tol_rel)


def check(got, want, exact, what=""):
    """got: one record of FrameStore.overlap (or a dict); want: counts(...).  exact (index arithmetic 1): every count equal.
    Otherwise (arithmetic 0): n_valid / n_visible / n_target equal, the class identity holds, and every class lies in
    [sure, sure + n_borderline]."""
    g = {k: int(got[k]) for k in FIELDS}
    assert g["n_consistent"] + g["n_behind"] + g["n_in_front"] == g["n_target"], (what, g)
    for k in ("n_valid", "n_visible", "n_target"):
        assert g[k] == want[k], (what, k, g, want)
    nb = want["n_borderline"]
    for k in ("n_consistent", "n_behind", "n_in_front"):
        if exact:
            assert g[k] == want[k], (what, k, g, want)
        else:
            assert want["sure"][k] <= g[k] <= want["sure"][k] + nb, (what, k, g, want)


def rel_pose(Wa, Wb):
    """T_ab = W_a^-1 W_b as rgbd360_store_overlap_all forms it (the formula of the header): float64 from the float32 inputs, the rigid
    inverse (R^T, -R^T t), every product and sum on its own, one rounding to float32.  Returns (4x4 float32, float64 |t_ab|)."""
    A = np.asarray(Wa, F).astype(np.float64)
    B = np.asarray(Wb, F).astype(np.float64)
    T = np.zeros((4, 4), F)
    t = np.zeros(3)
    for r in range(3):
        it = -((A[0, r] * A[0, 3] + A[1, r] * A[1, 3]) + A[2, r] * A[2, 3])
        for c in range(3):
            T[r, c] = F((A[0, r] * B[0, c] + A[1, r] * B[1, c]) + A[2, r] * B[2, c])
        t[r] = ((A[0, r] * B[0, 3] + A[1, r] * B[1, 3]) + A[2, r] * B[2, 3]) + it
        T[r, 3] = F(t[r])
    T[3, 3] = F(1)
    return T, float(np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]))
