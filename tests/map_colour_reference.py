"""numpy restatement of the voxel map's colour layer and of coloured ICP against the map (include/rgbd360_hip.h, "colour of the map" and
"coloured ICP against the map"; csrc/map_colour.h, csrc/map_align_colour.h) on top of the restatements they extend: the
map is voxel_map_reference.Map (its integer colour sums C), the 27 cells are map_align_reference.CELLS, the normals are
map_normals_reference.layer, the match is map_align_reference.Evaluation (steps 1-4, bit for bit) and the step is
map_align_reference.gn_step.  Added here, operation for operation in float64 (numpy's + - * / sqrt are IEEE-exact and never fused, so
the per-voxel and per-point values agree with the library's bit for bit): the intensity, the tangent basis, the five sums and the 2 x 2
solve of a voxel's gradient; the two residuals and the row of a source point; the loop; and the sliding scene (a textured floor and
wall) on which geometry alone cannot place the frame.  Independent of the library: array operations only."""
import numpy as np

import map_align_reference as A
import map_normals_reference as N
import voxel_map_reference as R

F = np.float32
D = np.float64
NONE, OK, NO_NORMAL, NO_GRADIENT = 0, 1, 2, 3
KEPT, DROPPED_NO_NORMAL, ZERO_GRADIENT = 1, 2, 4          # the bits of a point's class byte
STAT_NAMES = ("n_voxels", "n_below_min_count", "n_no_normal", "n_no_gradient", "n_gradients")
DEFAULTS = dict(min_count=1, min_support=5, max_flatness=0.05, min_gradient_support=4, min_spread=0.01)
ALIGN_DEFAULTS = dict(max_iters=10, eps=1e-6, min_count=1, min_matches=6, lambda_geometric=0.968, min_support=5, max_flatness=0.05,
                      min_gradient_support=4, min_spread=0.01)
ROW_NAMES = ("n",) + tuple("h%d%d" % (a, b) for a in range(6) for b in range(a, 6)) + tuple("g%d" % a for a in range(6)) + ("cost", "gg", "cc")
COUNTERS = ("n_valid", "n_box_rejected", "n_out_of_range", "n_no_normal", "n_no_gradient")


def intensity64(sums, count):
    """I64 = double(4899 Sr + 9617 Sg + 1868 Sb) / ((double(count) 16384) 255); sums [k, 3] integers, count [k] (or a scalar) >= 1."""
    s = np.asarray(sums, np.int64).reshape(-1, 3)
    y = 4899 * s[:, 0] + 9617 * s[:, 1] + 1868 * s[:, 2]
    return y.astype(D) / ((np.asarray(count, np.int64).astype(D) * 16384.0) * 255.0)


def tangent_basis(n32):
    """u, v [k, 3] float64 of the float32 normals n32 [k, 3]: the axis of smallest |n_k| (the lowest index on a tie) crossed with n,
    normalised, and n x u."""
    n = np.asarray(n32, F).reshape(-1, 3).astype(D)
    n0, n1, n2 = n.T
    a0, a1, a2 = np.abs(n0), np.abs(n1), np.abs(n2)
    k = np.where(a1 < a0, 1, 0)
    least = np.where(a1 < a0, a1, a0)
    k = np.where(a2 < least, 2, k)
    zero = np.zeros(len(n))
    t0 = np.where(k == 0, zero, np.where(k == 1, n2, -n1))
    t1 = np.where(k == 0, -n2, np.where(k == 1, zero, n0))
    t2 = np.where(k == 0, n1, np.where(k == 1, -n0, zero))
    with np.errstate(all="ignore"):
        ln = np.sqrt((t0 * t0 + t1 * t1) + t2 * t2)
        u = np.stack([t0 / ln, t1 / ln, t2 / ln], axis=1)
    v = np.stack([n1 * u[:, 2] - n2 * u[:, 1], n2 * u[:, 0] - n0 * u[:, 2], n0 * u[:, 1] - n1 * u[:, 0]], axis=1)
    return u, v


def fit(n32, i32, r, i_nb, present, min_gradient_support=4, min_spread=0.01):
    """The gradient of k voxels at once.  n32 [k, 3], i32 [k] float32; r [k, J, 3] float32 and i_nb [k, J] float32: the J neighbour places
    in their order, present [k, J] bool.  Returns (d [k, 3] float32, status [k] = OK / NO_GRADIENT, sums [k, 5] float64, m [k])."""
    n32 = np.asarray(n32, F).reshape(-1, 3)
    k = len(n32)
    r = np.asarray(r, F).reshape(k, -1, 3)
    i_nb = np.asarray(i_nb, F).reshape(k, -1)
    present = np.asarray(present, bool).reshape(k, -1)
    u, v = tangent_basis(n32)
    i0 = np.asarray(i32, F).reshape(k).astype(D)
    s = np.zeros((5, k), D)
    m = np.zeros(k, np.int64)
    with np.errstate(all="ignore"):
        for j in range(r.shape[1]):
            rx, ry, rz = (r[:, j, q].astype(D) for q in range(3))
            a = (rx * u[:, 0] + ry * u[:, 1]) + rz * u[:, 2]
            b = (rx * v[:, 0] + ry * v[:, 1]) + rz * v[:, 2]
            delta = i_nb[:, j].astype(D) - i0
            on = present[:, j]
            m += on
            for q, term in enumerate((a * a, a * b, b * b, a * delta, b * delta)):
                s[q] = s[q] + np.where(on, term, 0.0)
        saa, sab, sbb, sad, sbd = s
        tr = saa + sbb
        det = saa * sbb - sab * sab
        ok = (m >= min_gradient_support) & (det > D(F(min_spread)) * (tr * tr))
        du = (sad * sbb - sbd * sab) / det
        dv = (saa * sbd - sab * sad) / det
        d = np.stack([du * u[:, q] + dv * v[:, q] for q in range(3)], axis=1)
    d32 = np.where(ok[:, None], d, 0.0).astype(F)
    return d32, np.where(ok, OK, NO_GRADIENT).astype(np.int32), s.T.copy(), m


def layer(ref, min_count=1, min_support=5, max_flatness=0.05, min_gradient_support=4, min_spread=0.01, normal_layer=None):
    """Per row of `ref`: dict(status int32, intensity float32, gradient [k, 3] float32, support int64: the neighbours of the fit)."""
    k = len(ref)
    status = np.zeros(k, np.int32)
    intensity = np.zeros(k, F)
    gradient = np.zeros((k, 3), F)
    support = np.zeros(k, np.int64)
    if k == 0:
        return dict(status=status, intensity=intensity, gradient=gradient, support=support)
    live = ref.count > 0
    intensity[live] = intensity64(ref.C[live], ref.count[live]).astype(F)
    NL = normal_layer if normal_layer is not None else N.layer(ref, min_count, min_support, max_flatness)
    fitted = live & (ref.count >= min_count)
    status[fitted & (NL["status"] != N.OK)] = NO_NORMAL
    rows = np.nonzero(fitted & (NL["status"] == N.OK))[0]
    if not len(rows):
        return dict(status=status, intensity=intensity, gradient=gradient, support=support)
    keys = A.packed_keys(ref.key)
    i = ref.key[rows].astype(np.int64)
    cells = A.CELLS[1:]          # (the centre cell is the voxel itself)
    r = np.zeros((len(rows), len(cells), 3), F)
    i_nb = np.zeros((len(rows), len(cells)), F)
    present = np.zeros((len(rows), len(cells)), bool)
    for j, d in enumerate(cells):
        nb = i + np.array(d, np.int64) + R.BIAS
        ok = ((nb >= 0) & (nb < (1 << 21))).all(axis=1)
        pk = (nb[:, 2] << 42) | (nb[:, 1] << 21) | nb[:, 0]
        pos = np.minimum(np.searchsorted(keys, pk), len(keys) - 1)
        present[:, j] = ok & (keys[pos] == pk) & (ref.count[pos] >= min_count) & (ref.count[pos] > 0)
        r[:, j] = ref.xyz[pos] - ref.xyz[rows]          # float32
        i_nb[:, j] = intensity[pos]
    d32, st, _, m = fit(NL["normal"][rows], intensity[rows], r, i_nb, present, min_gradient_support, min_spread)
    gradient[rows] = d32
    status[rows] = st
    support[rows] = m
    return dict(status=status, intensity=intensity, gradient=gradient, support=support)


def colours(ref, **params):
    """The read-out: one record per row with count > 0, in the rows' order (keys ascending):
    dict(xyz, intensity, gradient, status, count, key3, support, stats)."""
    p = dict(DEFAULTS, **params)
    L = layer(ref, **p)
    live = np.nonzero(ref.count > 0)[0] if len(ref) else np.zeros(0, np.int64)
    st = L["status"][live]
    cnt = ref.count[live]
    stats = dict(n_voxels=len(live), n_below_min_count=int((cnt < p["min_count"]).sum()), n_no_normal=int((st == NO_NORMAL).sum()),
                 n_no_gradient=int((st == NO_GRADIENT).sum()), n_gradients=int((st == OK).sum()))
    return dict(xyz=ref.xyz[live], intensity=L["intensity"][live], gradient=L["gradient"][live], status=st, count=cnt.astype(np.int32),
                key3=ref.key[live], support=L["support"][live], stats=stats)


class RecordMap:
    """A map from its records (uint64 [k, 8] = key, count, Sx, Sy, Sz, Sr, Sg, Sb per live voxel, keys ascending: VoxelMap.records()) with
    the fields of voxel_map_reference.Map that the restatements read: whatever edits made the device's table, its layers restate from here."""

    def __init__(self, records):
        rec = np.ascontiguousarray(records, np.uint64).reshape(-1, 8)
        k = rec[:, 0].astype(np.int64)
        assert (np.diff(k) > 0).all()
        self.key = np.stack([(k & 0x1fffff) - R.BIAS, ((k >> 21) & 0x1fffff) - R.BIAS, (k >> 42) - R.BIAS], axis=1).astype(np.int32)
        self.count = rec[:, 1].astype(np.int64)
        self.S = rec[:, 2:5].view(np.int64).copy()
        self.C = rec[:, 5:8].view(np.int64).copy()
        self.xyz = (self.S.astype(D) / (self.count.astype(D) * R.FIX)[:, None]).astype(F)

    def __len__(self):
        return len(self.count)


class Layers:
    """The target's normal and colour layers by their parameters, built once per map and shared (a layer is a function of the map alone)."""

    def __init__(self, target):
        self.target, self.normal, self.colour = target, {}, {}

    def get(self, min_count, min_support, max_flatness, min_gradient_support, min_spread):
        kn = (int(min_count), int(min_support), float(F(max_flatness)))
        if kn not in self.normal:
            self.normal[kn] = N.layer(self.target, *kn)
        kc = kn + (int(min_gradient_support), float(F(min_spread)))
        if kc not in self.colour:
            self.colour[kc] = layer(self.target, *kc, normal_layer=self.normal[kn])
        return self.normal[kn], self.colour[kc]


class ColourEvaluation:
    """Steps 1-6 at one pose.  Per input point: key3 and d2 (map_align_reference.Evaluation's), cls (KEPT | DROPPED_NO_NORMAL |
    ZERO_GRADIENT bits), residuals [n, 2] float64 (r_G, r_C; zeros unless the point contributes); the five counters and the row of 31 sums;
    `rows` [contributing, 31]: the terms of every contributing point in the input's order."""

    def __init__(self, target, xyz, rgb, pose, leaf, box, max_dist, min_count=1, lambda_geometric=0.968, min_support=5, max_flatness=0.05,
                 min_gradient_support=4, min_spread=0.01, layers=None):
        xyz = np.asarray(xyz, F).reshape(-1, 3)
        rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
        assert rgb.shape == xyz.shape
        self.point = A.Evaluation(target, xyz, pose, leaf, box, max_dist, min_count)
        self.key3, self.d2 = self.point.key3, self.point.d2
        kept = np.nonzero(self.key3[:, 0] != A.NO_KEY)[0]
        self.cls = np.zeros(len(xyz), np.uint8)
        self.residuals = np.zeros((len(xyz), 2), D)
        lam = D(F(lambda_geometric))
        oml = D(1.0) - lam
        n_no_normal = n_no_gradient = 0
        self.rows = np.zeros((0, 31), D)
        if len(kept):
            NL, CL = (layers or Layers(target)).get(min_count, min_support, max_flatness, min_gradient_support, min_spread)
            row = self.point.row[kept]
            has_n = NL["status"][row] == N.OK
            self.cls[kept] = np.where(has_n, KEPT, KEPT | DROPPED_NO_NORMAL)
            n_no_normal = int((~has_n).sum())
            use, row = kept[has_n], row[has_n]
            zero_d = CL["status"][row] != OK
            self.cls[use] |= np.where(zero_d, ZERO_GRADIENT, 0).astype(np.uint8)
            n_no_gradient = int(zero_d.sum())
            w32 = R.transform(xyz[use], pose) if len(use) else np.zeros((0, 3), F)
            e = (w32 - target.xyz[row]).astype(D)          # Match::be: float32, widened
            w = w32.astype(D)
            n = NL["normal"][row].astype(D)
            d = CL["gradient"][row].astype(D)
            i_map = CL["intensity"][row].astype(D)
            i_q = intensity64(rgb[use], np.ones(len(use), np.int64))
            rg = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
            p = e - rg[:, None] * n
            rc = (i_map + ((d[:, 0] * p[:, 0] + d[:, 1] * p[:, 1]) + d[:, 2] * p[:, 2])) - i_q
            cross = lambda a: [w[:, 1] * a[:, 2] - w[:, 2] * a[:, 1], w[:, 2] * a[:, 0] - w[:, 0] * a[:, 2], w[:, 0] * a[:, 1] - w[:, 1] * a[:, 0]]
            JG = [n[:, 0], n[:, 1], n[:, 2]] + cross(n)
            JC = [d[:, 0], d[:, 1], d[:, 2]] + cross(d)
            H, g = [], []
            for a in range(6):
                sg, sc = lam * JG[a], oml * JC[a]
                H += [sg * JG[b] + sc * JC[b] for b in range(a, 6)]
                g.append(sg * rg + sc * rc)
            gg, cc = rg * rg, rc * rc
            self.rows = np.stack([np.ones(len(use))] + H + g + [lam * gg + oml * cc, gg, cc], axis=1).reshape(len(use), 31)
            self.residuals[use, 0] = rg
            self.residuals[use, 1] = rc
        self.sums = self.rows.sum(axis=0) if len(self.rows) else np.zeros(31, D)
        self.n = len(self.rows)
        self.counters = dict(self.point.counters, n_no_normal=n_no_normal, n_no_gradient=n_no_gradient)

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


def hessian64(s):
    """The same H in float64 (the conditioning of a scene)."""
    H = np.zeros((6, 6), D)
    h = 1
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = s[h]
            h += 1
    return H


class ColourAlignment:
    """The loop of map_align_reference.Alignment on ColourEvaluation: fitness = cost / n, rms_geometric = sqrt(gg / n), rms_colour =
    sqrt(cc / n).  margins as there; matches: n per iteration."""

    def __init__(self, target, xyz, rgb, guess, leaf, box, max_dist, max_iters=10, eps=1e-6, min_count=1, min_matches=6, lambda_geometric=0.968,
                 min_support=5, max_flatness=0.05, min_gradient_support=4, min_spread=0.01, layers=None):
        pose = np.asarray(guess, F).reshape(4, 4).copy()
        self.status, self.iterations, self.converged, self.trace, self.margins = A.OK, 0, 0, [], []
        layers = layers or Layers(target)
        ev = lambda T: ColourEvaluation(target, xyz, rgb, T, leaf, box, max_dist, min_count, lambda_geometric, min_support, max_flatness,
                                        min_gradient_support, min_spread, layers)
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
        n = self.final.n
        self.n_matched = n
        self.fitness = float(self.final.sums[28] / n) if n else 0.0
        self.rms_geometric = float(np.sqrt(self.final.sums[29] / n)) if n else 0.0
        self.rms_colour = float(np.sqrt(self.final.sums[30] / n)) if n else 0.0
        self.hessian, self.gradient = self.final.normal_equations()


# ---- the sliding scene: a textured floor z = 0 and wall x = 0.  Geometry fixes z, x and the three rotations and leaves y free; the texture
# fixes y.  The points lie exactly on the two planes and carry uint8 colours of a smooth texture (wavelengths of 0.7 m and more: several
# leaves, and a basin wider than the guess's 10 cm).
def texture(p):
    """uint8 colours [k, 3] of the surface points p [k, 3] float64: a function of (x, y) on the floor and of (z, y) on the wall -- the
    same expression, since one of x, z is 0 on either surface."""
    s, y = p[:, 0] + p[:, 2], p[:, 1]
    r = 0.5 + 0.22 * np.sin(2 * np.pi * y / 0.9 + 0.3) + 0.18 * np.sin(2 * np.pi * s / 1.3 + 1.1)
    g = 0.5 + 0.25 * np.sin(2 * np.pi * (y + 0.5 * s) / 1.1 + 2.0) + 0.15 * np.cos(2 * np.pi * s / 0.8)
    b = 0.5 + 0.2 * np.cos(2 * np.pi * y / 0.7 + 0.9) + 0.2 * np.sin(2 * np.pi * (s - y) / 1.7)
    return np.clip(np.rint(255.0 * np.stack([r, g, b], axis=1)), 0, 255).astype(np.uint8)


def surface_points(n, rng, y_half, extent):
    """n points, half on the floor (x in (0, extent), z = 0) and half on the wall (x = 0, z in (0, extent)), |y| < y_half; float32."""
    p = np.zeros((n, 3), D)
    p[:, 1] = rng.uniform(-y_half, y_half, n)
    s = rng.uniform(0.0, extent, n)
    floor = np.arange(n) % 2 == 0
    p[floor, 0] = s[floor]
    p[~floor, 2] = s[~floor]
    p = p.astype(F)
    return p, texture(p.astype(D))


def sliding_scene(n_map=60000, n_source=4000, seed=5):
    """(map cloud xyz, rgb; source cloud xyz, rgb): the map's points in world coordinates, the source's in its own frame, whose true pose
    is the identity."""
    rng = np.random.default_rng(seed)
    mx, mc = surface_points(n_map, rng, 1.6, 2.0)
    sx, sc = surface_points(n_source, rng, 1.0, 1.6)
    keep = (sx[:, 0] + sx[:, 2]) > 0.25          # away from the edge between the two planes, where voxels have no normal
    return mx, mc, sx[keep], sc[keep]


def sliding_guess(along=0.10):
    """The guess of the sliding-scene tests: `along` metres along the free axis y, 2 and 3 cm in x and z, 2 and 1 mrad about x and z."""
    import gn_reference as G
    return G.pseudo_exp_mp(np.array([0.02, along, -0.03, 0.002, 0.0, -0.001])).astype(F)
