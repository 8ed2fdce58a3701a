"""Independent numpy restatement of the 8-sensor rig's warp in the REFERENCE's arithmetic (the oracle's math_mode 0,
oracle/photo_icp_ref.cpp warp_robot; what rgbd360_rig_set_index_arithmetic(rig, 1) computes on the device).

The reference's two passes warp a pixel differently:
  chain 0, calcPhotoICPError_robot (RPI.h:4923-4924, 5021-5029): P = C p with C = (Rt^-1 T) Rt formed in float,
           column = round((double)(X fx) * inv + ox), inv = 1.0 / (double)Z;
  chain 1, calcHessianGradient_robot (RPI.h:5278-5290): q = T (Rt p), P = Rt^-1 q, column = round(((double)X * (double)fx) * inv + ox).
Every float operation is a separate float32 numpy operation in Eigen's order (numpy never fuses a multiply-add); the projection runs
in float64; round is half away from zero; a projection that is not finite or exceeds 1e9 in magnitude is invisible.
Test infrastructure only."""
import numpy as np

F = np.float32


def level_intrinsics(K, level):
    """RPI.h:4916-4920: scaleFactor = 1.0 / pow(2, level) stored to float, intrinsics scaled in float."""
    sf = F(1.0 / 2.0 ** level)
    return tuple(F(F(k) * sf) for k in K)


def mat4_mul_f32(A, B):
    """The oracle's mat4_mul_f32 on row-major float32 4x4: C[r, c] = ((A[r,0] B[0,c] + A[r,1] B[1,c]) + A[r,2] B[2,c]) + A[r,3] B[3,c]."""
    A, B = np.asarray(A, F), np.asarray(B, F)
    C = np.empty((4, 4), F)
    for r in range(4):
        for c in range(4):
            C[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return C


def rigid_inverse_f32(M):
    """The oracle's rigid_inverse_f32: [R^T | -R^T t] in float, the translation summed in index order."""
    M = np.asarray(M, F)
    Inv = np.zeros((4, 4), F)
    Inv[:3, :3] = M[:3, :3].T
    for i in range(3):
        Inv[i, 3] = -((Inv[i, 0] * M[0, 3] + Inv[i, 1] * M[1, 3]) + Inv[i, 2] * M[2, 3])
    Inv[3, 3] = F(1)
    return Inv


def xform_f32(M, P):
    """The oracle's xform_f32 on (n, 3) float32 points: ((m0 x + m1 y) + m2 z) + t per row, no fused multiply-add."""
    M = np.asarray(M, F)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)], axis=1)


def round_half_away(x):
    """C round() on float64: t = trunc(x), plus sign(x) where |x - t| >= 0.5 (x - t is exact).  np.round would round half to even."""
    t = np.trunc(x)
    return t + np.sign(x) * (np.abs(x - t) >= 0.5)


def warp_chain(T, Rt, lut, K, rows, cols, chain):
    """Target (row, col) of every LUT point (n x 3, x = -10000 for an invalid one) through chain 0 or 1 at rig pose T (4x4) with the
    sensor's extrinsic Rt (sensor -> rig).  K: the LEVEL's float32 intrinsics.  Returns (rc (n, 2) int32 with (-1, -1) where invisible or
    invalid, P (n, 3) float32 = the transformed point, q (n, 3) float32 = the rig-frame point (chain 1; zeros for chain 0))."""
    T, Rt = np.asarray(T, F), np.asarray(Rt, F)
    Rt_inv = rigid_inverse_f32(Rt)
    fx, fy, ox, oy = K
    P0 = np.asarray(lut, F)
    valid = P0[:, 0] != F(-10000.0)
    with np.errstate(all="ignore"):
        if chain == 0:
            Cm = mat4_mul_f32(mat4_mul_f32(Rt_inv, T), Rt)            # relPoseCam = poseCamRobot_inv * poseGuess * poseCamRobot
            P = xform_f32(Cm, P0)
            q = np.zeros_like(P)
            inv = 1.0 / P[:, 2].astype(np.float64)
            dc = (P[:, 0] * fx).astype(np.float64) * inv + np.float64(ox)
            dr = (P[:, 1] * fy).astype(np.float64) * inv + np.float64(oy)
        else:
            q = xform_f32(T, xform_f32(Rt, P0))
            P = xform_f32(Rt_inv, q)
            inv = 1.0 / P[:, 2].astype(np.float64)
            dc = (P[:, 0].astype(np.float64) * np.float64(fx)) * inv + np.float64(ox)
            dr = (P[:, 1].astype(np.float64) * np.float64(fy)) * inv + np.float64(oy)
        sane = np.isfinite(dr) & np.isfinite(dc) & (np.abs(dr) <= 1e9) & (np.abs(dc) <= 1e9)
        r = np.where(sane, round_half_away(np.where(sane, dr, -1.0)), -1.0)
        c = np.where(sane, round_half_away(np.where(sane, dc, -1.0)), -1.0)
    vis = valid & sane & (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
    rc = np.where(vis[:, None], np.stack([r, c], axis=1), -1).astype(np.int32)
    return rc, P, q


def weight_huber(err, reg):
    """RPI.h:545-554 weightHuber<float> on float32 arrays."""
    err, reg = np.asarray(err, F), np.asarray(reg, F)
    a = np.abs(err)
    with np.errstate(all="ignore"):
        w = np.sqrt(F(2) * reg * a - reg * reg) / a
    return np.where(a < reg, F(1), w).astype(F)


def error_sums(rc0, P0, gray_src, gray_trg, depth_trg, sigma_photo, sigma_depth, method):
    """calcPhotoICPError_robot's sums (e2p, e2d, nP, nD) from chain 0's indices and transformed depth (FIX C), in float64."""
    vis = rc0[:, 0] >= 0
    idx = rc0[vis, 0] * gray_trg.shape[1] + rc0[vis, 1]
    e2p = e2d = 0.0
    nP = nD = 0
    if method in (0, 2):
        diff = (gray_trg.reshape(-1)[idx] - gray_src.reshape(-1)[vis]).astype(F)
        w = weight_huber(diff, F(sigma_photo)).astype(np.float64) * (1.0 / np.float64(F(sigma_photo)))
        r = (w * diff).astype(F)
        e2p, nP = float(np.sum((r * r).astype(np.float64))), int(vis.sum())
    if method in (1, 2):
        d2 = depth_trg.reshape(-1)[idx]
        fin = np.isfinite(d2)
        d1 = P0[vis, 2][fin]
        diff = (d2[fin] - d1).astype(F)
        sd = (F(sigma_depth) * d1).astype(F)
        w = (weight_huber(diff, sd) / sd).astype(np.float64)                 # float / float, stored to double
        r = (w * diff).astype(F)
        e2d, nD = float(np.sum((r * r).astype(np.float64))), int(fin.sum())
    return e2p, e2d, nP, nD


def row_count(rc1, depth_trg, gx, gy, dgx, dgy, thr_photo, thr_depth, method):
    """calcHessianGradient_robot's Jacobian-row count from chain 1's indices: a flat intensity gradient skips the pixel, a finite target
    depth with a flat depth gradient skips it too, photometric row included (RPI.h:5331-5332, 5352-5353)."""
    vis = rc1[:, 0] >= 0
    idx = rc1[vis, 0] * gx.shape[1] + rc1[vis, 1]
    sal_p = ~((np.abs(gx.reshape(-1)[idx]) < thr_photo) & (np.abs(gy.reshape(-1)[idx]) < thr_photo))
    sal_d = ~((np.abs(dgx.reshape(-1)[idx]) < thr_depth) & (np.abs(dgy.reshape(-1)[idx]) < thr_depth))
    fin = np.isfinite(depth_trg.reshape(-1)[idx])
    if method == 0:
        return int(sal_p.sum())
    if method == 1:
        return int((fin & sal_d).sum())
    keep = sal_p & (~fin | sal_d)
    return int(keep.sum() + (keep & fin).sum())


def sensor_oracle(oracle_mod, frame_trg, frame_src, K, n_pyr):
    """A one-sensor Oracle with the rig's per-sensor settings (no seam mask, the sensor's pinhole camera): its pinhole LUT is the cloud
    the rig's calcPhotoICPError_robot / calcHessianGradient_robot warp (both build it with buildLUT_pinhole)."""
    o = oracle_mod.Oracle(n_pyr=n_pyr, mask_seams=0)
    o.set_camera(*[float(k) for k in K])
    o.set_target(*frame_trg)
    o.set_source(*frame_src)
    return o


def random_poses(rng, n, rot=0.04, trans=0.06):
    """n rig motions: the identity, then random rotations up to `rot` rad about random axes and translations up to `trans` m."""
    out = [np.eye(4)]
    for _ in range(n - 1):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = rng.uniform(0, rot)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = rng.uniform(-trans, trans, size=3)
        out.append(T)
    return out
