"""numpy restatement of the alignment of a frame against the voxel map (include/rgbd360_hip.h, "point-to-point ICP of a frame against
the map"; csrc/map_align.h) on top of voxel_map_reference.py: float32 operation by operation per point, float64 sums,
and the Gauss-Newton step from tests/gn_reference.py (the float32 rank test and LU inverse of gn_math.h in their division form, the
pseudo-exponential in mpmath rounded once).  Independent of the library: array operations only, no code shared with it.

The target is a voxel_map_reference.Map, i.e. a table that never dropped a point: every inserted key is found and no other, which is
what a lookup that ends at the first empty slot or at the probe bound gives on such a table."""
import numpy as np

import gn_reference as G
import voxel_map_reference as R

F = np.float32
NO_KEY = -2 ** 31
OK, ILL_POSED, NO_VALID_PIXELS = 0, 1, 2
# the centre first, then the other 26 in the order of three nested loops, dz outermost, dx innermost, each ascending
CELLS = [(0, 0, 0)] + [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
SUM_NAMES = ("n", "wx", "wy", "wz", "xx", "xy", "xz", "yy", "yz", "zz", "ex", "ey", "ez", "cx", "cy", "cz", "ee")


def sphere_cloud_np(depth, convention=2):
    """The convention-2 sphere cloud (RPI.h:4556-4571) of a depth image in numpy float32: the device's expressions with numpy's
    sin / cos, so within a few ulp of rgbd360_sphere_cloud, not bit-equal.  For the CPU tests, which have no device."""
    assert convention == 2
    d = np.asarray(depth)
    d = d.astype(F) * F(0.001) if d.dtype == np.uint16 else d.astype(F)
    rows, cols = d.shape
    res = F(2 * np.pi / cols)
    theta = np.arange(cols, dtype=F) * res
    phi = (F(0.5 * rows - 0.5) - np.arange(rows, dtype=F)) * res
    st, ct, sp, cp = np.sin(theta)[None, :], np.cos(theta)[None, :], np.sin(phi)[:, None], np.cos(phi)[:, None]
    xyz = np.stack([d * sp, -d * cp * st, -d * cp * ct], axis=2).astype(F)
    xyz[d == 0] = np.nan
    return xyz.reshape(-1, 3)


def packed_keys(key3):
    k = np.asarray(key3, np.int64) + R.BIAS
    return (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]


class Evaluation:
    """Steps 1-5 at one pose: per input point key3 (NO_KEY without a kept match) and d2 of the nearest candidate (+inf without one),
    the counters and the 17 sums over the kept matches."""

    def __init__(self, target, xyz, pose, leaf, box, max_dist, min_count=1):
        xyz = np.asarray(xyz, F).reshape(-1, 3)
        w, idx, self.counters = R.passing(xyz, pose, box)
        i = R.voxel_index(w, leaf)
        keys = packed_keys(target.key) if len(target) else np.zeros(0, np.int64)       # ascending, like the map's rows
        m = len(w)
        best = np.full(m, np.inf, F)
        best_row = np.full(m, -1, np.int64)
        best_e = np.zeros((m, 3), F)
        for d in CELLS:
            nb = i + np.array(d, np.int64) + R.BIAS
            ok = ((nb >= 0) & (nb < (1 << 21))).all(axis=1)       # outside the 21-bit range: no candidate, never wrapped
            pk = (nb[:, 2] << 42) | (nb[:, 1] << 21) | nb[:, 0]
            pos = np.minimum(np.searchsorted(keys, pk), max(len(keys) - 1, 0))
            found = ok & (keys[pos] == pk) & (target.count[pos] >= min_count) if len(keys) else np.zeros(m, bool)
            c = target.xyz[pos] if len(keys) else np.zeros((m, 3), F)
            with np.errstate(all="ignore"):
                e = w - c
                d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            better = found & (d2 < best)          # strictly smaller: a tie stays with the earlier candidate
            best = np.where(better, d2, best)
            best_row = np.where(better, pos, best_row)
            best_e = np.where(better[:, None], e, best_e)
        kept = (best_row >= 0) & (best <= F(max_dist) * F(max_dist))
        self.key3 = np.full((len(xyz), 3), NO_KEY, np.int32)
        self.d2 = np.full(len(xyz), np.inf, F)
        self.d2[idx] = best
        if kept.any():
            self.key3[idx[kept]] = target.key[best_row[kept]]
        self.row = np.full(len(xyz), -1, np.int64)          # the matched voxel's row in the target, kept or not
        self.row[idx] = best_row
        wk, ek = w[kept].astype(np.float64), best_e[kept].astype(np.float64)
        x, y, z = wk.T if len(wk) else (np.zeros(0),) * 3
        ex, ey, ez = ek.T if len(ek) else (np.zeros(0),) * 3
        terms = [np.ones(len(wk)), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z, ex, ey, ez, y * ez - z * ey, z * ex - x * ez, x * ey - y * ex,
                 (ex * ex + ey * ey) + ez * ez]
        self.sums = np.array([t.sum() for t in terms], np.float64)
        self.n = int(kept.sum())

    def normal_equations(self):
        return assemble(self.sums)


def assemble(s):
    """H (6 x 6) and g of J = [I | -[w]x] from the 17 sums, in double, cast to float32."""
    n, wx, wy, wz, xx, xy, xz, yy, yz, zz = s[:10]
    H = np.array([[n, 0, 0, 0, wz, -wy], [0, n, 0, -wz, 0, wx], [0, 0, n, wy, -wx, 0],
                  [0, -wz, wy, yy + zz, -xy, -xz], [wz, 0, -wx, -xy, xx + zz, -yz], [-wy, wx, 0, -xz, -yz, xx + yy]], np.float64)
    return H.astype(F), np.asarray(s[10:16], np.float64).astype(F)


def gn_step(H, g, pose):
    """gn::step with lambda 0: None when the rank test fails, else (new pose 4x4 float32, update[6] float32)."""
    if G.rank6_f32(H) != 6:
        return None
    u = G.update_f32(H, g, "div")
    if u is None:
        return None
    E = G.pseudo_exp_f32_mp(u.astype(np.float64))
    return G.mat4_mul_f32(E, np.asarray(pose, F)), u


class Alignment:
    """The loop: at most max_iters steps, then the final evaluation.  margins: per stop-or-continue decision the factor between
    max(v.v, w.w) and eps, whichever way round (>= 1)."""

    def __init__(self, target, xyz, guess, leaf, box, max_dist, max_iters=10, eps=1e-6, min_count=1, min_matches=6):
        pose = np.asarray(guess, F).reshape(4, 4).copy()
        self.status, self.iterations, self.converged, self.trace, self.margins = OK, 0, 0, [], []
        ev = lambda T: Evaluation(target, xyz, T, leaf, box, max_dist, min_count)
        for _ in range(max_iters):
            e = ev(pose)
            if e.n < min_matches:
                self.status = NO_VALID_PIXELS
                break
            step = gn_step(*e.normal_equations(), pose)
            if step is None:
                self.status = ILL_POSED
                break
            pose, u = step
            self.iterations += 1
            self.trace.append((e.n, float(e.sums[16]), u))
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
        if self.status == OK and self.final.n < min_matches:
            self.status = NO_VALID_PIXELS
        self.n_matched = self.final.n
        self.fitness = float(self.final.sums[16] / self.final.n) if self.final.n else 0.0
        self.hessian, self.gradient = self.final.normal_equations()


def pose_error(T, P):
    """(rotation angle in radians, translation distance in metres) of P^-1 T, in double."""
    D = np.linalg.inv(np.asarray(P, np.float64)) @ np.asarray(T, np.float64)
    c = min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0))
    s = np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0
    return float(np.arctan2(s, c)), float(np.linalg.norm(D[:3, 3]))


def perturbed(P, trans, rot, seed):
    """P with a left increment of `trans` metres and `rot` radians in seeded random directions, float32."""
    rng = np.random.default_rng(seed)
    t, a = rng.normal(size=3), rng.normal(size=3)
    v = np.concatenate([trans * t / np.linalg.norm(t), rot * a / np.linalg.norm(a)])
    return (G.pseudo_exp_mp(v) @ np.asarray(P, np.float64)).astype(F)
