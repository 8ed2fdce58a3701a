"""numpy restatement of generalized ICP against the voxel map (include/rgbd360_hip.h, "generalized ICP against the map";
csrc/map_align_gicp.h) on top of the restatements it extends: the match is map_align_reference.Evaluation (steps 1-4,
bit for bit), the target's normals are map_normals_reference.layer, the step is map_align_reference.gn_step.  Added here: the weight of
a match written operation for operation in float64 (numpy's + - * / sqrt are IEEE-exact and never fused, so it agrees with the
library's function bit for bit), the row and the loop.  Independent of the library: array operations only."""
import numpy as np

import map_align_reference as A
import map_normals_reference as N
import voxel_map_reference as R

F = np.float32
D = np.float64
KEPT, TARGET, SOURCE = 1, 2, 4          # the bits of a point's class byte
ROW_NAMES = ("n",) + tuple("h%d%d" % (a, b) for a in range(6) for b in range(a, 6)) + tuple("g%d" % a for a in range(6)) + ("cost", "ee")
COUNTERS = ("n_valid", "n_box_rejected", "n_out_of_range", "n_target_planes", "n_source_planes", "n_plane_pairs")


def covariance(n, s):
    """delta_jk - s (n_j n_k) as the six upper-triangle terms, [k, 6]; the off-diagonal terms as 0.0 - s (n_j n_k)."""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    return np.stack([1.0 - s * (x * x), 0.0 - s * (x * y), 0.0 - s * (x * z), 1.0 - s * (y * y), 0.0 - s * (y * z), 1.0 - s * (z * z)], axis=1)


def weight(nb, has_b, na, has_a, pose, epsilon):
    """Steps 2-4 for k matches at once.  nb [k, 3] float64 (the doubles of the float32 target normals), has_b [k] bool; na [k, 3] float32
    or None (no normal array), has_a: an array was passed; pose 4x4 float32; epsilon: the float32 parameter.  Returns (M [k, 6] float64 =
    M00 M01 M02 M11 M12 M22, used [k] = TARGET | SOURCE bits)."""
    nb = np.asarray(nb, D).reshape(-1, 3)
    k = len(nb)
    has_b = np.broadcast_to(np.asarray(has_b, bool), (k,))
    s = D(1.0) - D(F(epsilon))
    T = np.asarray(pose, F).reshape(4, 4).astype(D)
    with np.errstate(all="ignore"):
        cb = np.where(has_b[:, None], covariance(nb, s), np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]))
        ca = np.zeros((k, 6), D)
        present = np.zeros(k, bool)
        if has_a and na is not None:
            n32 = np.asarray(na, F).reshape(-1, 3)
            nd = n32.astype(D)
            q = (nd[:, 0] * nd[:, 0] + nd[:, 1] * nd[:, 1]) + nd[:, 2] * nd[:, 2]
            present = np.isfinite(n32).all(axis=1) & (q > 0.0)
            ln = np.sqrt(np.where(present, q, 1.0))
            h = nd / ln[:, None]
            r = np.stack([(T[j, 0] * h[:, 0] + T[j, 1] * h[:, 1]) + T[j, 2] * h[:, 2] for j in range(3)], axis=1)
            ca = np.where(present[:, None], covariance(np.where(present[:, None], r, 0.0), s), 0.0)
        a00, a01, a02, a11, a12, a22 = ((cb + ca)[:, j] for j in range(6))
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        M = np.stack([c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det], axis=1)
    return M, np.where(has_b, TARGET, 0) + np.where(present, SOURCE, 0)


def terms(M, w, e):
    """Step 5 per match: the 30 terms of the row [k, 30] from M [k, 6], the posed points w [k, 3] and e [k, 3], all float64."""
    m00, m01, m02, m11, m12, m22 = M.T
    wx, wy, wz = w.T
    ex, ey, ez = e.T
    qx, qy, qz = (m00 * ex + m01 * ey) + m02 * ez, (m01 * ex + m11 * ey) + m12 * ez, (m02 * ex + m12 * ey) + m22 * ez
    m3 = (wy * m02 - wz * m01, wy * m12 - wz * m11, wy * m22 - wz * m12)
    m4 = (wz * m00 - wx * m02, wz * m01 - wx * m12, wz * m02 - wx * m22)
    m5 = (wx * m01 - wy * m00, wx * m11 - wy * m01, wx * m12 - wy * m02)
    cost = (ex * qx + ey * qy) + ez * qz
    H = [m00, m01, m02, m3[0], m4[0], m5[0], m11, m12, m3[1], m4[1], m5[1], m22, m3[2], m4[2], m5[2],
         wy * m3[2] - wz * m3[1], wy * m4[2] - wz * m4[1], wy * m5[2] - wz * m5[1], wz * m4[0] - wx * m4[2], wz * m5[0] - wx * m5[2],
         wx * m5[1] - wy * m5[0]]
    g = [qx, qy, qz, wy * qz - wz * qy, wz * qx - wx * qz, wx * qy - wy * qx]
    return np.stack([np.ones(len(M))] + H + g + [cost, (ex * ex + ey * ey) + ez * ez], axis=1).reshape(len(M), 30)


class Layers:
    """The target's normal layers by their three parameters, built once per map and shared (a layer is a function of the map alone)."""

    def __init__(self, target):
        self.target, self.made = target, {}

    def get(self, min_count, min_support, max_flatness):
        k = (int(min_count), int(min_support), float(F(max_flatness)))
        if k not in self.made:
            self.made[k] = N.layer(self.target, *k)
        return self.made[k]


class GicpEvaluation:
    """Steps 1-6 at one pose.  Per input point: key3 and d2 (map_align_reference.Evaluation's), cls (KEPT | TARGET | SOURCE bits),
    weight_cost [n, 7] float64 (zeros without a kept match); the six counters and the row of 30 sums; `rows` [kept, 30]: the terms of
    every kept match in the input's order."""

    def __init__(self, target, xyz, pose, leaf, box, max_dist, normals=None, min_count=1, epsilon=1e-3, use_target_normals=1, min_support=5, max_flatness=0.05,
                 layers=None):
        xyz = np.asarray(xyz, F).reshape(-1, 3)
        self.point = A.Evaluation(target, xyz, pose, leaf, box, max_dist, min_count)
        self.key3, self.d2 = self.point.key3, self.point.d2
        kept = np.nonzero(self.key3[:, 0] != A.NO_KEY)[0]
        row = self.point.row[kept]
        w = R.transform(xyz[kept], pose) if len(kept) else np.zeros((0, 3), F)
        e = (w - target.xyz[row]).astype(D) if len(kept) else np.zeros((0, 3), D)      # Match::be: float32, widened
        if use_target_normals and len(target):
            L = (layers or Layers(target)).get(min_count, min_support, max_flatness)
            has_b = L["status"][row] == N.OK
            nb = L["normal"][row].astype(D)
        else:
            has_b, nb = np.zeros(len(kept), bool), np.zeros((len(kept), 3), D)
        na = None if normals is None else np.asarray(normals, F).reshape(-1, 3)[kept]
        M, used = weight(nb, has_b, na, normals is not None, pose, epsilon)
        self.rows = terms(M, w.astype(D), e)
        self.cls = np.zeros(len(xyz), np.uint8)
        self.cls[kept] = KEPT | used
        self.weight_cost = np.zeros((len(xyz), 7), D)
        self.weight_cost[kept, :6] = M
        self.weight_cost[kept, 6] = self.rows[:, 28]
        self.sums = self.rows.sum(axis=0) if len(kept) else np.zeros(30, D)
        self.n = len(kept)
        self.counters = dict(self.point.counters, n_target_planes=int(((used & TARGET) != 0).sum()), n_source_planes=int(((used & SOURCE) != 0).sum()),
                             n_plane_pairs=int((used == (TARGET | SOURCE)).sum()))

    def normal_equations(self):
        return assemble(self.sums)


def assemble(s):
    """H (6 x 6, symmetric) and g straight from the row, cast to float32."""
    H = np.zeros((6, 6), D)
    h = 1
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = s[h]
            h += 1
    return H.astype(F), np.asarray(s[22:28], D).astype(F)


class GicpAlignment:
    """The loop of map_align_reference.Alignment on GicpEvaluation: fitness = sum cost / n, fitness_point = sum e.e / n."""

    def __init__(self, target, xyz, guess, leaf, box, max_dist, normals=None, max_iters=10, eps=1e-6, min_count=1, min_matches=6, epsilon=1e-3,
                 use_target_normals=1, min_support=5, max_flatness=0.05, layers=None):
        pose = np.asarray(guess, F).reshape(4, 4).copy()
        self.status, self.iterations, self.converged, self.trace, self.margins = A.OK, 0, 0, [], []
        layers = layers or Layers(target)
        ev = lambda T: GicpEvaluation(target, xyz, T, leaf, box, max_dist, normals, min_count, epsilon, use_target_normals, min_support, max_flatness, layers)
        for _ in range(max_iters):
            e = ev(pose)
            if e.n < min_matches:
                self.status = A.NO_VALID_PIXELS
                break
            step = A.gn_step(*e.normal_equations(), pose)
            if step is None:
                self.status = A.ILL_POSED
                break
            pose, u = step
            self.iterations += 1
            self.trace.append((e.n, float(e.sums[28]), u))
            vv = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
            ww = (u[3] * u[3] + u[4] * u[4]) + u[5] * u[5]
            stop = bool(vv <= F(eps) and ww <= F(eps))
            r = float(max(vv, ww)) / float(F(eps)) if eps > 0 else np.inf
            self.margins.append(np.inf if r == 0 else max(r, 1 / r))
            if stop:
                self.converged = 1
                break
        self.pose = pose
        self.final = ev(pose)
        if self.status == A.OK and self.final.n < min_matches:
            self.status = A.NO_VALID_PIXELS
        self.n_matched = self.final.n
        self.fitness = float(self.final.sums[28] / self.final.n) if self.final.n else 0.0
        self.fitness_point = float(self.final.sums[29] / self.final.n) if self.final.n else 0.0
        self.hessian, self.gradient = self.final.normal_equations()


def map_source(ref, min_count=1, min_support=5, max_flatness=0.05):
    """A restated map as the source of an alignment: (xyz, normals) of its voxels in ascending (i_z, i_y, i_x) order, which is the order of
    its rows; the normal is zero where a voxel has none."""
    L = N.layer(ref, min_count, min_support, max_flatness)
    live = ref.count > 0
    return ref.xyz[live], L["normal"][live]
