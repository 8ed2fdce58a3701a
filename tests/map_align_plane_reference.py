"""numpy restatement of the point-to-plane alignment of a frame against the voxel map (include/rgbd360_hip.h, "point-to-plane ICP of a
frame against the map"; csrc/map_align_plane.h) on top of map_align_reference.py: candidates and the match are that
module's Evaluation (steps 1-4, bit for bit), the step is its gn_step.  Added here: the support sums over all candidates, the plane
function written operation for operation in float64 (numpy's + - * / sqrt are IEEE-exact and never fused, so it agrees with the
library's function bit for bit), the row and the loop.  Independent of the library: array operations only."""
import numpy as np

import map_align_reference as A
import voxel_map_reference as R

F = np.float32
D = np.float64
NONE, KEPT, UNSUPPORTED, NONPLANAR = 0, 1, 2, 3
ROW_NAMES = ("n",) + tuple("h%d%d" % (a, b) for a in range(6) for b in range(a, 6)) + tuple("g%d" % a for a in range(6)) + ("rr", "ee")


def plane_fit(cov, max_flatness):
    """Step 3 for k supports at once.  cov [k, 6] float64 = C00, C01, C02, C11, C12, C22.  Returns (normal [k, 3], planar [k] bool,
    l0 [k], l1 [k]); the normal is zero where no cross product is positive.  max_flatness: the float32 parameter, widened."""
    cov = np.asarray(cov, D).reshape(-1, 6)
    mf = D(F(max_flatness))
    a00, a01, a02, a11, a12, a22 = (cov[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        c2 = (a00 + a11) + a22
        c1 = ((a00 * a11 - a01 * a01) + (a00 * a22 - a02 * a02)) + (a11 * a22 - a12 * a12)
        c0 = (a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a12 * a02)) + a02 * (a01 * a12 - a11 * a02)
        l = np.zeros(len(cov), D)
        active = np.ones(len(cov), bool)
        for _ in range(12):
            f = ((l - c2) * l + c1) * l - c0
            df = (3.0 * l - 2.0 * c2) * l + c1
            active = active & (df > 0.0)
            step = f / df
            l = np.where(active, l - step, l)
            active = active & ~(np.abs(step) <= 1e-15 * c2)
        r0, r1, r2 = (a00 - l, a01, a02), (a01, a11 - l, a12), (a02, a12, a22 - l)
        cross = lambda u, v: (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        sq = lambda n: (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        n01, n02, n12 = cross(r0, r1), cross(r0, r2), cross(r1, r2)
        qq, n = sq(n01), np.stack(n01, axis=1)
        for cand in (n02, n12):
            q = sq(cand)
            better = q > qq
            qq = np.where(better, q, qq)
            n = np.where(better[:, None], np.stack(cand, axis=1), n)
        s = c2 - l
        p = c1 - l * s
        disc = s * s - 4.0 * p
        l1 = 0.5 * (s - np.sqrt(np.where(disc > 0.0, disc, 0.0)))
        some = qq > 0.0
        n = np.where(some[:, None], n / np.sqrt(np.where(some, qq, 1.0))[:, None], 0.0)
        planar = some & (l1 > 0.0) & (l <= mf * l1)
    return n, planar, l, l1


def covariance(se, see, m):
    """e_mean = sum e / m and C = sum e e^T / m - e_mean e_mean^T, [k, 3] and [k, 6], every operation on its own."""
    dm = np.asarray(m, D)[:, None]
    mean = se / dm
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cov = np.stack([see[:, k] / dm[:, 0] - mean[:, a] * mean[:, b] for k, (a, b) in enumerate(pairs)], axis=1)
    return mean, cov


class PlaneEvaluation:
    """Steps 1-5 at one pose.  Per input point: key3 and d2 (map_align_reference.Evaluation's), cls (NONE / KEPT / UNSUPPORTED /
    NONPLANAR), normal_r [n, 4] float64 (zeros unless KEPT); the counters (five) and the row of 30 sums over the KEPT points."""

    def __init__(self, target, xyz, pose, leaf, box, max_dist, min_count=1, min_support=5, max_flatness=0.05):
        xyz = np.asarray(xyz, F).reshape(-1, 3)
        self.point = A.Evaluation(target, xyz, pose, leaf, box, max_dist, min_count)
        self.key3, self.d2 = self.point.key3, self.point.d2
        w, idx, counters = R.passing(xyz, pose, box)
        i = R.voxel_index(w, leaf)
        keys = A.packed_keys(target.key) if len(target) else np.zeros(0, np.int64)
        k = len(w)
        se, see, m = np.zeros((k, 3), D), np.zeros((k, 6), D), np.zeros(k, np.int64)
        wd = w.astype(D)
        for d in A.CELLS:       # the candidates of Evaluation, cell by cell in the same order
            nb = i + np.array(d, np.int64) + R.BIAS
            ok = ((nb >= 0) & (nb < (1 << 21))).all(axis=1)
            pk = (nb[:, 2] << 42) | (nb[:, 1] << 21) | nb[:, 0]
            if not len(keys):
                break
            pos = np.minimum(np.searchsorted(keys, pk), len(keys) - 1)
            found = ok & (keys[pos] == pk) & (target.count[pos] >= min_count)
            e = wd - target.xyz[pos].astype(D)
            ex, ey, ez = e.T
            m += found
            se = se + np.where(found[:, None], e, 0.0)
            see = see + np.where(found[:, None], np.stack([ex * ex, ex * ey, ex * ez, ey * ey, ey * ez, ez * ez], axis=1), 0.0)
        matched = self.key3[idx, 0] != A.NO_KEY
        unsupported = matched & (m < min_support)
        fit = matched & ~unsupported
        mean, cov = covariance(se[fit], see[fit], m[fit])
        n, planar, self.l0, self.l1 = plane_fit(cov, max_flatness)
        r = (n[:, 0] * mean[:, 0] + n[:, 1] * mean[:, 1]) + n[:, 2] * mean[:, 2]
        cls = np.zeros(k, np.uint8)
        cls[unsupported] = UNSUPPORTED
        cls[np.nonzero(fit)[0][planar]] = KEPT
        cls[np.nonzero(fit)[0][~planar]] = NONPLANAR
        self.cls = np.zeros(len(xyz), np.uint8)
        self.cls[idx] = cls
        self.support = np.zeros(len(xyz), np.int64)
        self.support[idx] = m
        self.normal_r = np.zeros((len(xyz), 4), D)
        sel = idx[np.nonzero(fit)[0][planar]]
        self.normal_r[sel, :3] = n[planar]
        self.normal_r[sel, 3] = r[planar]
        # the row over the contributing points
        wk = wd[np.nonzero(fit)[0][planar]]
        nk, rk = n[planar], r[planar]
        x, y, z = wk.T if len(wk) else (np.zeros(0),) * 3
        nx, ny, nz = nk.T if len(nk) else (np.zeros(0),) * 3
        J = [nx, ny, nz, y * nz - z * ny, z * nx - x * nz, x * ny - y * nx]
        eb = (w[np.nonzero(fit)[0][planar]] - target.xyz[self.point.row[sel]]).astype(D) if len(wk) else np.zeros((0, 3))      # e of the match, float32
        terms = [np.ones(len(wk))] + [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * rk for a in range(6)]
        terms += [rk * rk, (eb[:, 0] * eb[:, 0] + eb[:, 1] * eb[:, 1]) + eb[:, 2] * eb[:, 2]]
        self.sums = np.array([t.sum() for t in terms], D)
        self.n = int(planar.sum())
        self.counters = dict(counters, n_unsupported=int(unsupported.sum()), n_nonplanar=int((fit).sum() - planar.sum()))

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


class PlaneAlignment:
    """The loop of map_align_reference.Alignment on PlaneEvaluation: fitness = sum r r / n, fitness_point = sum e.e / n."""

    def __init__(self, target, xyz, guess, leaf, box, max_dist, max_iters=10, eps=1e-6, min_count=1, min_matches=6, min_support=5, max_flatness=0.05):
        pose = np.asarray(guess, F).reshape(4, 4).copy()
        self.status, self.iterations, self.converged, self.trace, self.margins = A.OK, 0, 0, [], []
        ev = lambda T: PlaneEvaluation(target, xyz, T, leaf, box, max_dist, min_count, min_support, max_flatness)
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


def corner_scene(seed, pose=None, size=2.0, step=0.01):
    """A room corner: the planes x = 0, y = 0 and z = 0, each size x size metres from the common corner, sampled on a jittered grid of
    `step` metres (every sample lies exactly on its plane).  With `pose` (world <- frame) the samples are moved by its inverse: the
    cloud of a frame that sees the corner from `pose`.  float32 [n, 3]."""
    rng = np.random.default_rng(seed)
    g = np.arange(0.0, size, step) + 0.5 * step
    u, v = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    pts = []
    for axis in range(3):
        ju = u + rng.uniform(-0.5, 0.5, len(u)) * step
        jv = v + rng.uniform(-0.5, 0.5, len(v)) * step
        p = np.zeros((len(u), 3))
        p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = ju, jv
        pts.append(p)
    p = np.concatenate(pts)
    if pose is not None:
        T = np.linalg.inv(np.asarray(pose, D))
        p = p @ T[:3, :3].T + T[:3, 3]
    return p.astype(F)
