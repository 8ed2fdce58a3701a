"""The rig calibration against the voxel map (rgbd360_map_calibrate_rig_*, csrc/rig_calib.h; include/rgbd360_hip.h, "the rig's
extrinsics against the map") restated in numpy: the evaluation through map_align_plane_reference.PlaneEvaluation, the solve in scalar
loops over Python floats (IEEE float64, one rounding per operation) in the header's order, the update through gn_reference's float32
pseudo-exponential and 4 x 4 product.  Matrices are [row, column] here; the library stores them column-major.  Also the scene the
tests share."""
import math

import numpy as np

import gn_reference as G
import map_align_plane_reference as PL
import map_align_reference as A
import voxel_map_reference as R

F = np.float32
D = np.float64
PIVOT = 1e-12
MAX_SENSORS = 16


def adjoint(T):
    """Ad(T) = [[R, [t]x R], [0, R]] in float64 from the float32 pose, gn::se3_adjoint's products."""
    T = np.asarray(T, F).astype(D)
    t = [float(T[0, 3]), float(T[1, 3]), float(T[2, 3])]
    Ad = [[0.0] * 6 for _ in range(6)]
    for c in range(3):
        R0, R1, R2 = float(T[0, c]), float(T[1, c]), float(T[2, c])
        Ad[0][c], Ad[1][c], Ad[2][c] = R0, R1, R2
        Ad[0][c + 3] = t[1] * R2 - t[2] * R1
        Ad[1][c + 3] = t[2] * R0 - t[0] * R2
        Ad[2][c + 3] = t[0] * R1 - t[1] * R0
        Ad[3][c + 3], Ad[4][c + 3], Ad[5][c + 3] = R0, R1, R2
    return Ad


class Input:
    """The blocks of one input from its 30 sums: A, b, C = A Ad, G = Ad^T C, gs = Ad^T b; sums of products ascend from 0.0."""

    def __init__(self, row, min_input, Ad):
        row = [0.0 + float(v) for v in row]         # (the library adds the input's rows to 0.0)
        self.A = [[0.0] * 6 for _ in range(6)]
        h = 1
        for a in range(6):
            for b in range(a, 6):
                self.A[a][b] = self.A[b][a] = row[h]
                h += 1
        self.b = row[22:28]
        self.n, self.rr = row[0], row[28]
        self.used = int(row[0]) >= min_input
        self.C = [[0.0] * 6 for _ in range(6)]
        self.G = [[0.0] * 6 for _ in range(6)]
        for c in range(6):
            for r in range(6):
                s = 0.0
                for k in range(6):
                    s += self.A[r][k] * Ad[k][c]
                self.C[r][c] = s
        for c in range(6):
            for r in range(6):
                s = 0.0
                for k in range(6):
                    s += Ad[k][r] * self.C[k][c]
                self.G[r][c] = s
        self.gs = []
        for r in range(6):
            s = 0.0
            for k in range(6):
                s += Ad[k][r] * self.b[k]
            self.gs.append(s)
        self.W = None


class Frame:
    """F_k, f_k over the contributing inputs and, eliminated, the Cholesky factor, z = L^-1 f and W_ks = L^-1 C_ks."""

    def __init__(self, inputs, refine, fixed, lam):
        Fm = [[0.0] * 6 for _ in range(6)]
        f = [0.0] * 6
        self.has = False
        for inp in inputs:
            if not inp.used:
                continue
            self.has = True
            for r in range(6):
                for c in range(6):
                    Fm[r][c] += inp.A[r][c]
                f[r] += inp.b[r]
        self.elim, self.ill = self.has and bool(refine), False
        if not self.elim:
            return
        f = [-v for v in f]
        d0 = [Fm[i][i] for i in range(6)]
        for i in range(6):
            Fm[i][i] = d0[i] + lam * d0[i]
        L = [[0.0] * 6 for _ in range(6)]
        for j in range(6):
            for i in range(j, 6):
                s = Fm[i][j]
                for p in range(j):
                    s -= L[i][p] * L[j][p]
                if i == j:
                    if not s > PIVOT * d0[j]:
                        self.ill = True
                        return
                    L[j][j] = math.sqrt(s)
                else:
                    L[i][j] = s / L[j][j]
        self.L = L
        self.z = [0.0] * 6
        for i in range(6):
            s = f[i]
            for p in range(i):
                s -= L[i][p] * self.z[p]
            self.z[i] = s / L[i][i]
        for sn, inp in enumerate(inputs):
            if not inp.used or sn == fixed:
                continue
            W = [[0.0] * 6 for _ in range(6)]
            for c in range(6):
                for i in range(6):
                    s = inp.C[i][c]
                    for p in range(i):
                        s -= L[i][p] * W[p][c]
                    W[i][c] = s / L[i][i]
            inp.W = W


def apply_update(x, pose):
    """pose <- pseudo_exp((float32) x) pose; the float32 update, v.v and w.w."""
    u = np.array(x, D).astype(F)
    E = G.pseudo_exp_f32_mp(u.astype(D))
    vv = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
    ww = (u[3] * u[3] + u[4] * u[4]) + u[5] * u[5]
    return G.mat4_mul_f32(E, np.asarray(pose, F)), u, vv, ww


class Solve:
    """One step on given rows: rows [K S, 30], T [K, 4, 4], E [S, 4, 4] -> status, updates [K + S, 6] float32 (delta_k then epsilon_s), the new
    T and E, max_vv / max_ww, n (contributing points), cost, used, skipped, cond (the reduced matrix's condition number, a measurement)."""

    def __init__(self, rows, T, E, refine=0, fixed=-1, lam=0.0, min_input=6, min_matches=6):
        T, E = np.array(T, F).copy(), np.array(E, F).copy()
        K, S = len(T), len(E)
        lam = float(F(lam))
        rows = np.asarray(rows, D).reshape(K * S, 30)
        self.inputs = [[Input(rows[k * S + s], min_input, adj) for s in range(S)] for k, adj in ((k, adjoint(T[k])) for k in range(K))]
        self.frames = [Frame(self.inputs[k], refine, fixed, lam) for k in range(K)]
        flat = [i for fr in self.inputs for i in fr]
        self.used = sum(1 for i in flat if i.used)
        self.skipped = sum(1 for fr in self.frames if not fr.has)
        self.n = sum(int(i.n) for i in flat if i.used)
        self.cost = 0.0
        for i in flat:
            if i.used:
                self.cost += i.rr
        self.T, self.E, self.updates = T, E, np.zeros((K + S, 6), F)
        self.max_vv = self.max_ww = F(0)
        self.cond = None
        if self.n < min_matches:
            self.status = A.NO_VALID_PIXELS
            return
        if any(fr.ill for fr in self.frames):
            self.status = A.ILL_POSED
            return
        free = [s for s in range(S) if s != fixed]
        n = 6 * len(free)
        M = [[0.0] * n for _ in range(n)]
        rhs = [0.0] * n
        for i in range(n):
            si, a = free[i // 6], i % 6
            for j in range(i + 1):
                sj, c = free[j // 6], j % 6
                acc = 0.0
                if si == sj:
                    for k in range(K):
                        if self.inputs[k][si].used:
                            acc += self.inputs[k][si].G[a][c]
                for k in range(K):
                    ii, ij = self.inputs[k][si], self.inputs[k][sj]
                    if not self.frames[k].elim or not ii.used or not ij.used:
                        continue
                    s = 0.0
                    for r in range(6):
                        s += ii.W[r][a] * ij.W[r][c]
                    acc -= s
                M[i][j] = acc
            acc = 0.0
            for k in range(K):
                if self.inputs[k][si].used:
                    acc += self.inputs[k][si].gs[a]
            acc = -acc
            for k in range(K):
                ii = self.inputs[k][si]
                if not self.frames[k].elim or not ii.used:
                    continue
                s = 0.0
                for r in range(6):
                    s += ii.W[r][a] * self.frames[k].z[r]
                acc -= s
            rhs[i] = acc
        if n:
            full = np.array(M) + np.tril(np.array(M), -1).T
            d = np.sqrt(np.abs(np.diag(full)))
            if (d > 0).all():
                self.cond = float(np.linalg.cond(full / np.outer(d, d)))
        d0 = [M[i][i] for i in range(n)]
        for i in range(n):
            M[i][i] = d0[i] + lam * d0[i]
        for j in range(n):
            col = []
            for i in range(j, n):
                s = M[i][j]
                for p in range(j):
                    s -= M[i][p] * M[j][p]
                col.append(s)
            if not col[0] > PIVOT * d0[j]:
                self.status = A.ILL_POSED
                return
            d = math.sqrt(col[0])
            M[j][j] = d
            for i in range(j + 1, n):
                M[i][j] = col[i - j] / d
        for j in range(n):
            y = rhs[j] / M[j][j]
            rhs[j] = y
            for i in range(j + 1, n):
                rhs[i] -= M[i][j] * y
        for j in range(n - 1, -1, -1):
            x = rhs[j] / M[j][j]
            rhs[j] = x
            for i in range(j):
                rhs[i] -= M[j][i] * x
        self.status = A.OK
        vvs, wws = [], []
        for slot, s in enumerate(free):
            self.E[s], self.updates[K + s], vv, ww = apply_update(rhs[6 * slot:6 * slot + 6], E[s])
            vvs.append(vv), wws.append(ww)
        for k in range(K):
            fr = self.frames[k]
            if not fr.elim:
                continue
            v = list(fr.z)
            for slot, s in enumerate(free):
                inp = self.inputs[k][s]
                if not inp.used:
                    continue
                for r in range(6):
                    for c in range(6):
                        v[r] -= inp.W[r][c] * rhs[6 * slot + c]
            dl = [0.0] * 6
            for i in range(5, -1, -1):
                s = v[i]
                for p in range(5, i, -1):
                    s -= fr.L[p][i] * dl[p]
                dl[i] = s / fr.L[i][i]
            self.T[k], self.updates[k], vv, ww = apply_update(dl, T[k])
            vvs.append(vv), wws.append(ww)
        self.max_vv = max(vvs + [F(0)])
        self.max_ww = max(wws + [F(0)])


def rows_of(target, clouds, T, E, leaf, max_dist, **plane):
    """[K S, 30]: the sums of every input at P_ks = T_k E_s (float32 product); an empty cloud gives zeros."""
    K, S = len(T), len(E)
    rows = np.zeros((K * S, 30), D)
    for k in range(K):
        for s in range(S):
            x = np.asarray(clouds[k * S + s], F).reshape(-1, 3)
            if len(x):
                rows[k * S + s] = PL.PlaneEvaluation(target, x, G.mat4_mul_f32(T[k], E[s]), leaf, None, max_dist, **plane).sums
    return rows


class RigCalibration:
    """The loop: at most max_iters steps, then the final evaluation.  trace: (n, cost, max_vv, max_ww) per applied step."""

    def __init__(self, target, clouds, T, E, leaf, max_dist, max_iters=10, eps=1e-6, min_matches=6, refine=0, fixed=-1, lam=0.0, min_input=6, **plane):
        T, E = np.array(T, F).copy(), np.array(E, F).copy()
        self.status, self.iterations, self.converged, self.trace, self.conds = A.OK, 0, 0, [], []
        ev = lambda: rows_of(target, clouds, T, E, leaf, max_dist, **plane)
        for _ in range(max_iters):
            st = Solve(ev(), T, E, refine, fixed, lam, min_input, min_matches)
            if st.status != A.OK:
                self.status = st.status
                break
            T, E = st.T, st.E
            self.iterations += 1
            self.trace.append((st.n, st.cost, float(st.max_vv), float(st.max_ww)))
            self.conds.append(st.cond)
            if st.max_vv <= F(eps) and st.max_ww <= F(eps):
                self.converged = 1
                break
        self.T, self.E = T, E
        self.rows = ev()
        n_in = [int(r[0]) for r in self.rows]
        used = [n >= min_input for n in n_in]
        self.n_inputs_used = sum(used)
        self.n_matched = sum(n for n, u in zip(n_in, used) if u)
        self.cost = 0.0
        for r, u in zip(self.rows, used):
            if u:
                self.cost += float(r[28])
        S = len(E)
        self.n_frames_skipped = sum(1 for k in range(len(T)) if not any(used[k * S:(k + 1) * S]))
        if self.status == A.OK and self.n_matched < min_matches:
            self.status = A.NO_VALID_PIXELS
        self.fitness = self.cost / self.n_matched if self.n_matched else 0.0


# ---- the scene of the tests: a closed 2 m cube, K = 6 rig poses around its centre, S = 4 sensors looking outwards
LEAF, MAX_FLATNESS, N_FRAMES, N_SENSORS = 0.1, 5e-4, 6, 4


def rot(axis, angle):
    v = np.zeros(6)
    v[3 + axis] = angle
    return G.pseudo_exp_mp(v)


def cube(seed_a, seed_b, step):
    return np.concatenate([PL.corner_scene(seed_a, step=step), (F(2) - PL.corner_scene(seed_b, step=step)).astype(F)])


def true_rig(n_frames=N_FRAMES, n_sensors=N_SENSORS, seed=7):
    """(T [K, 4, 4], E [S, 4, 4]) float32: rig poses at (1, 1, 1) +- 0.4 with random rotations; sensors looking outwards (their z axis),
    360 / S degrees apart about the rig's y axis, tilted 0.3 rad, 5 cm off the rig's centre."""
    rng = np.random.default_rng(seed)
    T = []
    for _ in range(n_frames):
        v = np.concatenate([np.ones(3) + rng.uniform(-0.4, 0.4, 3), rng.normal(size=3) * 0.7])
        T.append(G.pseudo_exp_mp(v).astype(F))
    E = []
    for s in range(n_sensors):
        M = rot(1, 2 * np.pi * s / n_sensors) @ rot(0, 0.3)
        M[:3, 3] = M[:3, :3] @ np.array([0.0, 0.0, 0.05])
        E.append(M.astype(F))
    return np.stack(T), np.stack(E)


def sensor_clouds(world, T, E):
    """Per (k, s), frame-major: the points of `world` sensor s sees in frame k (z > 0.2, |x|, |y| < z tan 35 deg), in the sensor's coordinates."""
    out, lim = [], np.tan(np.deg2rad(35.0))
    for k in range(len(T)):
        for s in range(len(E)):
            P = np.linalg.inv(T[k].astype(D) @ E[s].astype(D))
            p = world.astype(D) @ P[:3, :3].T + P[:3, 3]
            keep = (p[:, 2] > 0.2) & (np.abs(p[:, 0]) < p[:, 2] * lim) & (np.abs(p[:, 1]) < p[:, 2] * lim)
            out.append(p[keep].astype(F))
    return out


def perturbed_all(Ms, trans, rot_sigma, seed, skip=()):
    """Every pose with a left increment N(0, trans) metres / N(0, rot_sigma) radians per axis; the poses in `skip` stay."""
    rng = np.random.default_rng(seed)
    out = []
    for i, M in enumerate(Ms):
        v = np.concatenate([rng.normal(size=3) * trans, rng.normal(size=3) * rot_sigma])
        out.append(M if i in skip else (G.pseudo_exp_mp(v) @ M.astype(D)).astype(F))
    return np.stack(out)


def largest_translation_error(Ms, truth):
    return max(A.pose_error(M, P)[1] for M, P in zip(Ms, truth))


_SCENE = {}


def scene():
    """The shared scene, built once: target (the map's restatement at leaf 0.1), map_cloud, T, E (truth), clouds (K S arrays)."""
    if not _SCENE:
        T, E = true_rig()
        map_cloud = cube(101, 102, 0.02)
        _SCENE.update(map_cloud=map_cloud, target=R.Map([(map_cloud, None, np.eye(4, dtype=F))], LEAF, None), T=T, E=E,
                      clouds=sensor_clouds(cube(201, 202, 0.04), T, E))
    return _SCENE


# The start of the scenario: every free extrinsic (and, joint, every rig pose) off by a left increment of fixed size in a seeded random
# direction: sqrt(3) x 0.02 m and sqrt(3) x 0.01 rad, the expected norms of N(0, 0.02 m) / N(0, 0.01 rad) per axis.
START_TRANS, START_ROT = 0.02 * 3 ** 0.5, 0.01 * 3 ** 0.5


def start(joint):
    """(T0, E0, refine, fixed) of the scenario's two modes."""
    sc = scene()
    E0 = np.stack([sc["E"][s] if joint and s == 0 else A.perturbed(sc["E"][s], START_TRANS, START_ROT, 300 + s) for s in range(N_SENSORS)])
    T0 = np.stack([A.perturbed(P, START_TRANS, START_ROT, 400 + k) for k, P in enumerate(sc["T"])]) if joint else sc["T"].copy()
    return T0, E0, int(joint), 0 if joint else -1


def plane_kw():
    return dict(max_flatness=MAX_FLATNESS)


def solve_cases():
    """The cases of the solve tests: name -> (rows [K S, 30], T, E, dict of Solve's keyword arguments).  Built once."""
    if "cases" in _SCENE:
        return _SCENE["cases"]
    sc = scene()
    out = {}
    for joint in (0, 1):
        T0, E0, refine, fixed = start(joint)
        rows = rows_of(sc["target"], sc["clouds"], T0, E0, LEAF, LEAF, **plane_kw())
        kw = dict(refine=refine, fixed=fixed)
        name = "joint" if joint else "extrinsics"
        out[name] = (rows, T0, E0, kw)
        out[name + "_lambda"] = (rows, T0, E0, dict(kw, lam=0.01))
        empty = rows.copy()
        empty[1 * N_SENSORS + 2] = 0.0
        out[name + "_empty_input"] = (empty, T0, E0, kw)
        out[name + "_small_input"] = (rows, T0, E0, dict(kw, min_input=int(np.sort(rows[:, 0])[3]) + 1))      # the four smallest inputs drop out
        gone = rows.copy()
        gone[2 * N_SENSORS:3 * N_SENSORS] = 0.0
        out[name + "_empty_frame"] = (gone, T0, E0, kw)
    rows, T0, E0, _ = out["extrinsics"]
    out["one_by_one"] = (rows[:1], T0[:1], E0[:1], dict(refine=0, fixed=-1))
    T16, E16 = true_rig(2, MAX_SENSORS, seed=9)
    clouds16 = sensor_clouds(cube(201, 202, 0.04), T16, E16)
    E16s = np.stack([A.perturbed(E16[s], START_TRANS, START_ROT, 500 + s) for s in range(MAX_SENSORS)])
    rows16 = rows_of(sc["target"], clouds16, T16, E16s, LEAF, LEAF, **plane_kw())
    out["sixteen"] = (rows16, T16, E16s, dict(refine=0, fixed=-1))
    E16f = E16s.copy()
    E16f[5] = E16[5]
    out["sixteen_joint"] = (rows_of(sc["target"], clouds16, T16, E16f, LEAF, LEAF, **plane_kw()), T16, E16f, dict(refine=1, fixed=5))
    _SCENE["cases"] = out
    return out


def wall_case():
    """ILL_POSED: one sensor that sees the same wall (the inside of z = 0) in every frame, the frames differing by motions that keep the
    wall where it is (a turn about its normal, a shift along it): every frame constrains the same three of the extrinsic's six
    directions.  (A wall seen from rig poses of different orientation constrains all six: that is well-posed.)"""
    sc = scene()
    w = PL.corner_scene(201, step=0.04)
    wall = w[(w[:, 2] == 0) & (w[:, 0] > 0.3) & (w[:, 0] < 1.7) & (w[:, 1] > 0.3) & (w[:, 1] < 1.7)]
    E = sc["E"][:1]
    T = []
    for k in range(3):
        Z = rot(2, 0.3 * k)
        Z[:3, 3] = (0.1 * k, -0.05 * k, 0.0)
        T.append((Z @ sc["T"][0].astype(D)).astype(F))
    T = np.stack(T)
    clouds = []
    for k in range(3):
        P = np.linalg.inv(T[k].astype(D) @ E[0].astype(D))
        clouds.append((wall.astype(D) @ P[:3, :3].T + P[:3, 3]).astype(F))
    return rows_of(sc["target"], clouds, T, E, LEAF, LEAF, **plane_kw()), T, E, dict(refine=0, fixed=-1)


def singular_rows():
    """ILL_POSED by hand: every input's A = n j j^T of one direction j (rank 1), b = j."""
    sc = scene()
    j = np.array([1.0, 2.0, -1.0, 0.5, 0.25, -2.0])
    row = np.zeros(30)
    row[0] = 100.0
    row[1:22] = [100.0 * j[a] * j[b] for a in range(6) for b in range(a, 6)]
    row[22:28] = j
    row[28] = 1.0
    return np.tile(row, (2 * 2, 1)), sc["T"][:2], sc["E"][:2], dict(refine=0, fixed=-1)
