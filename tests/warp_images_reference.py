"""The planes rgbd360_warp_images must produce, restated with numpy from outputs the CPU oracle already has: its warp indices,
its pyramid planes and its LUT.  Nothing here runs a warp of its own.

Rules (RPI.h = the reference's include/RegisterPhotoICP.h):
  winner        the LARGEST source index that lands on a target pixel (the loop of RPI.h:2953 runs i ascending, writes overwrite)
  warped_gray   methods 0, 2: Isrc[winner], written before the saliency test (RPI.h:3033 precedes 3038)
  warped_depth  methods 1, 2: spherical |R p + t| where the target depth is finite (RPI.h:2976, 3064-3067); pinhole the
                transformed z, no test (RPI.h:1051); method 2 only where the target's gray gradient is salient (the `continue`
                of RPI.h:3038-3039 / 1031-1032 skips the depth block)
  diff_*        |target - warped| over the whole level, holes included (RPI.h:4664-4676)
A plane that does not apply to the method is zero.
"""
import numpy as np

F = np.float32
THRES_SAL_PHOTO = F(0.01)       # RPI.h:213 thresSaliencyIntensity, the default of both the oracle and the library


def pushed(T_gt):
    """T_gt . translate(0.2, 0.3, 0.5), the second pose of the tests: far enough from the truth that a fifth of the hit target pixels
    of the 256 x 128 pair collect several sources."""
    M = np.eye(4)
    M[:3, 3] = (0.2, 0.3, 0.5)
    return np.asarray(T_gt) @ M


def winners(idx, rows, cols):
    """idx: (n, 2) int32 (row, col) per source pixel, (-1, -1) = not visible.  Flat int32 plane: the largest source index per target
    pixel, -1 where nothing landed."""
    idx = np.asarray(idx)
    vis = idx[:, 0] >= 0
    src = np.nonzero(vis)[0].astype(np.int32)
    flat = idx[vis, 0].astype(np.int64) * cols + idx[vis, 1].astype(np.int64)
    win = np.full(rows * cols, -1, np.int32)
    np.maximum.at(win, flat, src)
    return win


def counts(idx, rows, cols):
    """How many source pixels land on every target pixel (flat)."""
    idx = np.asarray(idx)
    vis = idx[:, 0] >= 0
    flat = idx[vis, 0].astype(np.int64) * cols + idx[vis, 1].astype(np.int64)
    return np.bincount(flat, minlength=rows * cols)


def transformed(lut, pose):
    """R p + t of every LUT point in float32 without fused operations (Eigen's product order, tests/np_restatement.py:124-126)."""
    x, y, z = (np.ascontiguousarray(lut[:, k], F) for k in range(3))
    R = np.asarray(pose, F)[:3, :3]
    t = np.asarray(pose, F)[:3, 3]
    X = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
    Y = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
    Z = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]
    return X.astype(F), Y.astype(F), Z.astype(F)


def planes_from(idx, lut, pose, method, gray_src, gray_trg, depth_trg, gx, gy, pinhole=False, thres=THRES_SAL_PHOTO):
    """The five planes (rows x cols) from the oracle's outputs: idx = warp_indices(level, pose), lut = lut(level) (n x 3), the rest
    its planes of the level."""
    rows, cols = gray_trg.shape
    win = winners(idx, rows, cols)
    hit = win >= 0
    w = np.where(hit, win, 0)
    X, Y, Z = transformed(lut, pose)
    if pinhole:
        rng = Z
    else:
        rng = np.sqrt(((X * X + Y * Y) + Z * Z).astype(F)).astype(F)          # np_restatement.py:127
    gs, gt, dt = gray_src.ravel(), gray_trg.ravel(), depth_trg.ravel()
    photo, depth = method != 1, method != 0
    wg = np.zeros(rows * cols, F)
    wd = np.zeros(rows * cols, F)
    dg = np.zeros(rows * cols, F)
    dd = np.zeros(rows * cols, F)
    if photo:
        wg = np.where(hit, gs[w], F(0)).astype(F)
        dg = np.abs(gt - wg).astype(F)
    if depth:
        takes = hit.copy()
        if not pinhole:
            takes &= np.isfinite(dt)
        if method == 2:
            takes &= ~((np.abs(gx.ravel()) < thres) & (np.abs(gy.ravel()) < thres))
        wd = np.where(takes, rng[w], F(0)).astype(F)
        with np.errstate(invalid="ignore"):
            dd = np.abs(dt - wd).astype(F)
    sh = (rows, cols)
    return dict(winner=win.reshape(sh), warped_gray=wg.reshape(sh), warped_depth=wd.reshape(sh), diff_gray=dg.reshape(sh),
                diff_depth=dd.reshape(sh))


def from_oracle(ora, level, pose, method, pinhole=False):
    """The five planes for an oracle with both frames set (and the camera, for the pinhole path), in its current math mode."""
    idx = ora.warp_indices_pinhole(level, pose) if pinhole else ora.warp_indices(level, pose)
    lut = ora.lut_pinhole(level) if pinhole else ora.lut(level)
    P = {k: ora.plane(k, level) for k in ("gray_src", "gray_trg", "depth_trg", "gx", "gy")}
    out = planes_from(idx, lut, pose, method, P["gray_src"], P["gray_trg"], P["depth_trg"], P["gx"], P["gy"], pinhole,
                      F(ora.params.thres_sal_photo))
    out["idx"] = idx
    return out
