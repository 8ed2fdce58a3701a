"""numpy restatement of the robust kernels of the alignments against the voxel map (include/rgbd360_hip.h, "robust kernels of the
alignments against the map"; csrc/map_align.h: RobustWeight and vmap::Robust) on top of the four restatements of the
quadratic methods, which are imported and not edited: the match, the classes and every per-point quantity are theirs, the terms t are
formed as they form them, the weighted terms as w * (t), the loop is theirs (A.gn_step, the same stop tests).  Added here: rho and w of
the three kinds for arrays (the operations of gn::robust_rho_w in its order; pose_graph_robust_reference.rho_w is the scalar form),
the robust row, and two orders of summation:
  "numpy"   every word summed as the method's own restatement sums it (point and plane: t.sum() per term; generalized ICP and colour:
            rows.sum(axis=0)), so that a robust evaluation whose weights are all 1.0 has the quadratic restatement's bytes;
  "device"  the order of the evaluation kernel (vmap::eval_tile, block_row_sum, icp_solve_rows): a thread's four points 256 apart one
            after another, the wave's 64 lanes through a butterfly of offsets 32 .. 1, the four waves in ascending order, the workgroups'
            rows in ascending order -- a tile of 1024 points per workgroup, of an image row for a sphere frame (`shape` = (rows, cols)) or
            of the cloud.  Adding 0.0 for a point that does not contribute changes no bit, so the device's sums come out word for word.
The probe count of a row is a property of the table's slots, not of the definition: RobustEvaluation.row holds NaN there.
Independent of the library: array operations only."""
import numpy as np

import map_align_gicp_reference as GI
import map_align_plane_reference as PL
import map_align_reference as A
import map_colour_reference as CO
import voxel_map_reference as R

F = np.float32
D = np.float64
POINT, PLANE, GICP, COLOUR = 0, 1, 2, 3
NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3
KINDS = (HUBER, CAUCHY, GEMAN_MCCLURE)
KIND_NAMES = {NONE: "none", HUBER: "huber", CAUCHY: "cauchy", GEMAN_MCCLURE: "geman_mcclure"}
SUM_SQ = {POINT: 16, PLANE: 28, GICP: 28, COLOUR: 28}          # the cost word: the words in front of it are weighted
N_SUMS = {POINT: 17, PLANE: 30, GICP: 30, COLOUR: 31}          # the sums of a row, in front of its counters
COUNTERS = {POINT: (), PLANE: ("n_unsupported", "n_nonplanar"), GICP: ("n_target_planes", "n_source_planes", "n_plane_pairs"),
            COLOUR: ("n_no_normal", "n_no_gradient")}
WORDS = {m: N_SUMS[m] + 3 + len(COUNTERS[m]) + 2 for m in COUNTERS}        # the method's row: sums, counters, probes, points searched
ASSEMBLE = {POINT: A.assemble, PLANE: PL.assemble, GICP: GI.assemble, COLOUR: CO.assemble}
TILE, THREADS = 1024, 256


def rho_w(kind, delta, s):
    """(rho, w) of gn::robust_rho_w for an array s of cost terms, operation for operation.  Whenever not s > 0, and for NONE, (s, 1)."""
    s = np.asarray(s, D)
    rho, w = s.copy(), np.ones(s.shape, D)
    delta = D(delta)
    d2 = delta * delta
    pos = s > 0.0
    with np.errstate(all="ignore"):
        if kind == HUBER:
            out = pos & ~(s <= d2)
            q = np.sqrt(s[out])
            rho[out] = 2.0 * delta * q - d2
            w[out] = delta / q
        elif kind == CAUCHY:
            u = s[pos] / d2
            rho[pos] = d2 * np.log1p(u)
            w[pos] = 1.0 / (1.0 + u)
        elif kind == GEMAN_MCCLURE:
            t = d2 / (d2 + s[pos])
            rho[pos] = s[pos] * t
            w[pos] = t * t
        elif kind != NONE:
            raise ValueError("kind %r" % (kind,))
    return rho, w


def device_sum(values, idx, n_points, shape=None):
    """The sums the evaluation and solve kernels give for per-point values [k, T] of the input points idx (ascending), T words at once."""
    values = np.asarray(values, D)
    values = values.reshape(len(idx), values.shape[1] if values.ndim == 2 else 1)
    idx = np.asarray(idx, np.int64)
    if shape is None:
        n_blocks = max((n_points + TILE - 1) // TILE, 1)
        block, within = idx // TILE, idx % TILE
    else:
        rows, cols = shape
        gx = (cols + TILE - 1) // TILE
        n_blocks = max(rows * gx, 1)
        r, c = idx // cols, idx % cols
        block, within = r * gx + c // TILE, c % TILE
    slots = np.zeros((n_blocks, TILE // THREADS, THREADS, values.shape[1]), D)
    slots[block, within // THREADS, within % THREADS] = values
    acc = np.zeros(slots.shape[:1] + slots.shape[2:], D)
    for k in range(slots.shape[1]):         # a thread's points, one after another
        acc = acc + slots[:, k]
    v = acc.reshape(n_blocks, THREADS // 64, 64, -1)
    for off in (32, 16, 8, 4, 2, 1):        # the butterfly, as lane 0 sees it
        v = v[:, :, :off] + v[:, :, off:2 * off]
    v = v[:, :, 0]
    part = v[:, 0]
    for wv in range(1, THREADS // 64):      # the waves in ascending order
        part = part + v[:, wv]
    total = np.zeros(values.shape[1], D)
    for b in range(n_blocks):               # the rows in ascending order
        total = total + part[b]
    return total


def _point_terms(ev, target, xyz, pose):
    idx = np.nonzero(ev.key3[:, 0] != A.NO_KEY)[0]
    w32 = R.transform(xyz[idx], pose) if len(idx) else np.zeros((0, 3), F)
    e = (w32 - target.xyz[ev.row[idx]]).astype(D) if len(idx) else np.zeros((0, 3), D)
    x, y, z = w32.astype(D).T
    ex, ey, ez = e.T
    terms = [np.ones(len(idx)), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z, ex, ey, ez, y * ez - z * ey, z * ex - x * ez, x * ey - y * ex,
             (ex * ex + ey * ey) + ez * ez]
    return idx, np.stack(terms, axis=1).reshape(len(idx), 17)


def _plane_terms(ev, target, xyz, pose):
    idx = np.nonzero(ev.cls == PL.KEPT)[0]
    w32 = R.transform(xyz[idx], pose) if len(idx) else np.zeros((0, 3), F)
    eb = (w32 - target.xyz[ev.point.row[idx]]).astype(D) if len(idx) else np.zeros((0, 3), D)
    x, y, z = w32.astype(D).T
    nx, ny, nz = ev.normal_r[idx, :3].T
    rk = ev.normal_r[idx, 3]
    J = [nx, ny, nz, y * nz - z * ny, z * nx - x * nz, x * ny - y * nx]
    terms = [np.ones(len(idx))] + [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * rk for a in range(6)]
    terms += [rk * rk, (eb[:, 0] * eb[:, 0] + eb[:, 1] * eb[:, 1]) + eb[:, 2] * eb[:, 2]]
    return idx, np.stack(terms, axis=1).reshape(len(idx), 30)


class RobustEvaluation:
    """One robust evaluation of `method` at `pose` under (kind, delta).  base: the quadratic restatement's evaluation; idx: the input points
    that contribute; s, rho, w_contrib: their cost terms, losses and weights; w [n points]: the weight per input point, 0.0 where none;
    sums: the method's sums, weighted (word 0: sum w; the cost word: sum rho; the diagnostic sums behind it unweighted); n, n_downweighted,
    sum_w; counters; row: the whole robust row as the device lays it out (NaN in the probe word).  params: the method's own keyword
    arguments (min_count, min_support, max_flatness, epsilon, use_target_normals, lambda_geometric, ..., layers); normals / rgb: the
    source's, for generalized ICP / the colour method."""

    def __init__(self, method, kind, delta, target, xyz, pose, leaf, box, max_dist, order="numpy", shape=None, normals=None, rgb=None, **params):
        xyz = np.asarray(xyz, F).reshape(-1, 3)
        self.method, self.kind, self.delta = method, kind, float(delta)
        if method == POINT:
            self.base = A.Evaluation(target, xyz, pose, leaf, box, max_dist, **params)
            self.idx, terms = _point_terms(self.base, target, xyz, pose)
        elif method == PLANE:
            self.base = PL.PlaneEvaluation(target, xyz, pose, leaf, box, max_dist, **params)
            self.idx, terms = _plane_terms(self.base, target, xyz, pose)
        elif method == GICP:
            self.base = GI.GicpEvaluation(target, xyz, pose, leaf, box, max_dist, normals, **params)
            self.idx, terms = np.nonzero(self.base.key3[:, 0] != A.NO_KEY)[0], self.base.rows
        else:
            self.base = CO.ColourEvaluation(target, xyz, rgb, pose, leaf, box, max_dist, **params)
            self.idx = np.nonzero(((self.base.cls & CO.KEPT) != 0) & ((self.base.cls & CO.DROPPED_NO_NORMAL) == 0))[0]
            terms = self.base.rows
        assert len(terms) == len(self.idx) == self.base.n
        q = SUM_SQ[method]
        self.s = terms[:, q].copy()
        self.rho, self.w_contrib = rho_w(kind, delta, self.s)
        weighted = terms.copy()
        weighted[:, :q] = self.w_contrib[:, None] * (terms[:, :q])
        weighted[:, q] = self.rho
        self.terms = weighted
        if order == "device":
            self.sums = device_sum(weighted, self.idx, len(xyz), shape)
        elif method in (POINT, PLANE):
            self.sums = np.array([np.ascontiguousarray(weighted[:, k]).sum() for k in range(weighted.shape[1])], D)
        else:
            self.sums = weighted.sum(axis=0) if len(weighted) else np.zeros(weighted.shape[1], D)
        self.w = np.zeros(len(xyz), D)
        self.w[self.idx] = self.w_contrib
        self.n, self.n_downweighted, self.sum_w = len(self.idx), int((self.w_contrib < 1.0).sum()), float(self.sums[0])
        self.counters = self.base.counters
        c = self.counters
        tail = [c["n_valid"], c["n_box_rejected"], c["n_out_of_range"]] + [c[k] for k in COUNTERS[method]]
        searched = c["n_valid"] - c["n_box_rejected"] - c["n_out_of_range"]
        self.row = np.array(list(self.sums) + [D(v) for v in tail] + [np.nan, D(searched), D(self.n), D(self.n_downweighted)], D)
        assert len(self.row) == WORDS[method] + 2

    def normal_equations(self):
        return ASSEMBLE[self.method](self.sums)


class RobustAlignment:
    """The loop of map_align_reference.Alignment on RobustEvaluation: n counts the contributing points, the trace's sum of squares is
    sum rho, fitness = sum rho / n; fitness_point (plane, generalized ICP) = sum e.e / n, unweighted."""

    def __init__(self, method, kind, delta, target, xyz, guess, leaf, box, max_dist, max_iters=10, eps=1e-6, min_matches=6, order="numpy", shape=None,
                 **params):
        pose = np.asarray(guess, F).reshape(4, 4).copy()
        self.status, self.iterations, self.converged, self.trace, self.margins, self.poses = A.OK, 0, 0, [], [], []
        q = SUM_SQ[method]
        ev = lambda T: RobustEvaluation(method, kind, delta, target, xyz, T, leaf, box, max_dist, order, shape, **params)
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
            self.poses.append(pose)
            self.trace.append((e.n, float(e.sums[q]), u))
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
        self.fitness = float(self.final.sums[q] / self.final.n) if self.final.n else 0.0
        self.fitness_point = float(self.final.sums[29] / self.final.n) if self.final.n and method in (PLANE, GICP) else 0.0
        self.hessian, self.gradient = self.final.normal_equations()
        self.info = dict(method=method, kind=kind, delta_eff=float(delta), sum_w=self.final.sum_w, n=self.final.n, n_downweighted=self.final.n_downweighted)


def trial(lift, patch=(0.5, 1.5)):
    """The trial of DESIGN.md 3.31: the corner scene at leaf 0.1 as the map, a sparser sample of it as the source with the floor points
    inside `patch` (in x and in y) raised by `lift`, seen from the general pose; the guess 2 cm and 0.5 degrees beside it.
    (target map, source cloud in the frame of P, P, guess, the number of raised points)."""
    target = R.Map([(PL.corner_scene(101, step=0.02), None, np.eye(4, dtype=F))], 0.1, None)
    src = PL.corner_scene(201, None, step=0.04).astype(D)
    lo, hi = patch
    raised = (src[:, 2] == 0.0) & (src[:, 0] > lo) & (src[:, 0] < hi) & (src[:, 1] > lo) & (src[:, 1] < hi)
    src[raised, 2] += lift
    P = R.general_pose()
    T = np.linalg.inv(np.asarray(P, D))
    cloud = (src @ T[:3, :3].T + T[:3, 3]).astype(F)
    return target, cloud, P, A.perturbed(P, 0.02, np.radians(0.5), 7), int(raised.sum())
