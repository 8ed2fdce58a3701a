"""numpy restatement of the planar regions of the voxel map (include/rgbd360_hip.h, "planar regions of the map"; DESIGN.md 3.24;
csrc/map_planes.h), built on the restatements it extends: the map of voxel_map_reference, the cell order of map_align_reference.CELLS and
the per-voxel normals of map_normals_reference.layer.

Input: the map of tests/voxel_map_reference.py (keys ascending, read-out centroids); a row whose count is 0 stands for a tombstone and is
absent everywhere.  Predicates are float64 + - x on the float64 values of the float32 inputs, operation for operation as the device does
them; the sums are int64.  Independent of the library: array operations only (the hull of a handful of points is a loop over them)."""
import numpy as np

import map_align_reference as A
import map_normals_reference as N
import voxel_map_reference as R

F = np.float32
D = np.float64
FIX = 65536.0
DEFAULTS = dict(min_count=1, min_support=5, max_flatness=0.05, max_voxel_curvature=np.inf, cos_angle=0.9961947, max_offset=0.5, min_voxels=50,
                max_curvature=0.0013)
STAT_NAMES = ("n_voxels", "n_eligible", "n_links", "n_regions", "n_planes_available", "n_voxels_in_planes")
# RGBD360_MAP_PLANE_DIRS: (a_k, b_k) about 1024 (cos, sin) of 2 pi k / 64, literal
DIRS = np.array([
    (1024, 0), (1019, 100), (1004, 200), (980, 297), (946, 392), (903, 483), (851, 569), (792, 650), (724, 724), (650, 792), (569, 851),
    (483, 903), (392, 946), (297, 980), (200, 1004), (100, 1019), (0, 1024), (-100, 1019), (-200, 1004), (-297, 980), (-392, 946),
    (-483, 903), (-569, 851), (-650, 792), (-724, 724), (-792, 650), (-851, 569), (-903, 483), (-946, 392), (-980, 297), (-1004, 200),
    (-1019, 100), (-1024, 0), (-1019, -100), (-1004, -200), (-980, -297), (-946, -392), (-903, -483), (-851, -569), (-792, -650),
    (-724, -724), (-650, -792), (-569, -851), (-483, -903), (-392, -946), (-297, -980), (-200, -1004), (-100, -1019), (0, -1024),
    (100, -1019), (200, -1004), (297, -980), (392, -946), (483, -903), (569, -851), (650, -792), (724, -724), (792, -650), (851, -569),
    (903, -483), (946, -392), (980, -297), (1004, -200), (1019, -100)], np.int64)
# the 13 offsets whose neighbour has the larger key: those behind the centre in the nested dz / dy / dx loops
LARGER = [d for d in A.CELLS[1:] if (d[2], d[1], d[0]) > (0, 0, 0)]
assert len(LARGER) == 13


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def link_terms(ref, leaf, P, layer=None):
    """Every pair of eligible voxels in neighbouring cells, the smaller key first: (u, v rows, |n_u . n_v|, |n_u . e|, |n_v . e|, the
    eligibility mask, the normal layer).  The link predicate compares these with cos_angle and max_offset leaf.  layer: a hand-made
    normal layer (status, normal, curvature per row) in place of the map's own."""
    L = N.layer(ref, P["min_count"], P["min_support"], P["max_flatness"]) if layer is None else layer
    k = len(ref)
    elig = (ref.count > 0) & (L["status"] == N.OK) & (L["curvature"] <= F(P["max_voxel_curvature"])) if k else np.zeros(0, bool)
    us, vs = [], []
    if elig.any():
        keys = A.packed_keys(ref.key)
        rows = np.nonzero(elig)[0]
        i = ref.key[rows].astype(np.int64)
        for d in LARGER:
            nb = i + np.array(d, np.int64) + R.BIAS
            ok = ((nb >= 0) & (nb < (1 << 21))).all(axis=1)          # an index outside the 21-bit range does not exist
            pk = (nb[:, 2] << 42) | (nb[:, 1] << 21) | nb[:, 0]
            pos = np.minimum(np.searchsorted(keys, pk), k - 1)
            found = ok & (keys[pos] == pk) & elig[pos]
            us.append(rows[found])
            vs.append(pos[found])
    u = np.concatenate(us) if us else np.zeros(0, np.int64)
    v = np.concatenate(vs) if vs else np.zeros(0, np.int64)
    nu, nv = L["normal"][u].astype(D), L["normal"][v].astype(D)
    e = ref.xyz[v].astype(D) - ref.xyz[u].astype(D)
    return u, v, np.abs(_dot(nu, nv)), np.abs(_dot(nu, e)), np.abs(_dot(nv, e)), elig, L


def sums_in_range(n_voxels, extent_cells, leaf):
    """The range rule: N ((E + 2) leaf 2^16)^2 < 2^62 in float64."""
    b = (D(extent_cells) + 2.0) * D(F(leaf)) * FIX
    return bool(D(n_voxels) * (b * b) < 2.0 ** 62)


def segment(ref, leaf, layer=None, **params):
    """The regions: dict(eligible [k] bool, root [k] the row of the voxel's root (its own row where it is not eligible), n_links, regions:
    one dict per region by root key ascending -- row (of the root), n_voxels, n_points, extent, sums [9] int64, members (rows) --, margin:
    how far the closest pair lies from a threshold of the link predicate)."""
    P = dict(DEFAULTS, **params)
    u, v, nn, ou, ov, elig, L = link_terms(ref, leaf, P, layer)
    cos_angle, bound = D(F(P["cos_angle"])), D(F(P["max_offset"])) * D(F(leaf))
    linked = (nn >= cos_angle) & (ou <= bound) & (ov <= bound)
    margin = min([np.inf] + [float(np.abs(t - b).min()) for t, b in ((nn, cos_angle), (ou, bound), (ov, bound)) if len(t)])
    lu, lv = u[linked], v[linked]
    root = np.arange(len(ref), dtype=np.int64)
    while True:         # the smallest row of a component spreads along the links, then every row jumps to its root's root
        new = root.copy()
        np.minimum.at(new, lu, root[lv])
        np.minimum.at(new, lv, root[lu])
        new = new[new]
        if np.array_equal(new, root):
            break
        root = new
    regions = []
    for r in np.unique(root[elig]) if elig.any() else []:
        members = np.nonzero(elig & (root == r))[0]
        q = np.rint((ref.xyz[members].astype(D) - ref.xyz[r].astype(D)[None, :]) * FIX).astype(np.int64)
        sums = np.array([q[:, 0].sum(), q[:, 1].sum(), q[:, 2].sum(), (q[:, 0] * q[:, 0]).sum(), (q[:, 0] * q[:, 1]).sum(), (q[:, 0] * q[:, 2]).sum(),
                         (q[:, 1] * q[:, 1]).sum(), (q[:, 1] * q[:, 2]).sum(), (q[:, 2] * q[:, 2]).sum()], np.int64)
        extent = int(np.abs(ref.key[members].astype(np.int64) - ref.key[r].astype(np.int64)[None, :]).max())
        regions.append(dict(row=int(r), n_voxels=len(members), n_points=int(ref.count[members].sum()), extent=extent, sums=sums, members=members))
    return dict(eligible=elig, root=root, n_links=int(linked.sum()), regions=regions, margin=margin, layer=L)


def plane_from_sums(n_voxels, n_points, root_centroid, sums, viewpoint=None):
    """The plane record of a region from its sums alone (float64, numpy's eigh): dict(centroid, normal, d, curvature float64; count, e1, e2,
    evals)."""
    s = np.asarray(sums, np.int64).astype(D)
    n = D(n_voxels)
    c = (s[:3] / FIX) / n
    m2 = (s[3:] / (FIX * FIX)) / n
    C = np.array([[m2[0] - c[0] * c[0], m2[1] - c[0] * c[1], m2[2] - c[0] * c[2]],
                  [m2[1] - c[0] * c[1], m2[3] - c[1] * c[1], m2[4] - c[1] * c[2]],
                  [m2[2] - c[0] * c[2], m2[4] - c[1] * c[2], m2[5] - c[2] * c[2]]], D)
    evals, evecs = np.linalg.eigh(C)
    centroid = np.asarray(root_centroid, F).astype(D) + c
    normal = evecs[:, 0].copy()
    vp = np.zeros(3, D) if viewpoint is None else np.asarray(viewpoint, F).astype(D)
    if float((vp - centroid) @ normal) < 0:
        normal = -normal
    tr = C[0, 0] + C[1, 1] + C[2, 2]
    l1, l2 = max(evals[1], 0.0), max(evals[2], 0.0)
    return dict(centroid=centroid, normal=normal, d=float(-(normal @ centroid)), curvature=float(abs(evals[0] / tr)) if tr != 0 else 0.0,
                count=int(n_points), e1=evecs[:, 1].copy(), e2=evecs[:, 2].copy(), evals=evals, area_moment=float(12.0 * np.sqrt(l1 * l2)),
                elongation=float(np.sqrt(l2 / l1)) if l1 > 0 else float("inf"))


def convex_hull(uv):
    """Andrew's monotone chain on [n, 2] points: the hull's vertices counter-clockwise ([m, 2]; fewer than three: no hull)."""
    pts = np.unique(np.asarray(uv, D), axis=0)
    if len(pts) < 3:
        return np.zeros((0, 2), D)
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in pts[::-1]:
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    hull = np.array(lower[:-1] + upper[:-1], D)
    return hull if len(hull) >= 3 else np.zeros((0, 2), D)


def polygon_area_centre(poly):
    x, y = poly[:, 0], poly[:, 1]
    xn, yn = np.roll(x, -1), np.roll(y, -1)
    cr = x * yn - y * xn
    a2 = cr.sum()
    return abs(a2) / 2, ((x + xn) * cr).sum() / (3 * a2), ((y + yn) * cr).sum() / (3 * a2)


def planes(ref, leaf, viewpoint=None, max_planes=256, layer=None, **params):
    """The whole call: dict(planes: plane dicts as pbmap.register_planes takes them, by root key ascending, each with n_voxels, members,
    uv_all (every member in the plane's frame) and extremes (the rows of its 64 extreme members); root_key3; stats; label_key3 and
    plane_index per row of `ref` (plane_index counts over ALL planes that passed, whatever max_planes); segmentation).  Raises OverflowError
    where the library returns -8."""
    P = dict(DEFAULTS, **params)
    S = segment(ref, leaf, layer, **P)
    stats = dict(n_voxels=int((ref.count > 0).sum()), n_eligible=int(S["eligible"].sum()), n_links=S["n_links"], n_regions=len(S["regions"]),
                 n_planes_available=0, n_voxels_in_planes=0)
    passed = []
    keys = A.packed_keys(ref.key) if len(ref) else np.zeros(0, np.int64)
    for g in S["regions"]:
        if g["n_voxels"] < P["min_voxels"]:
            continue
        if not sums_in_range(g["n_voxels"], g["extent"], leaf):
            raise OverflowError("region sums out of range")
        fit = plane_from_sums(g["n_voxels"], g["n_points"], ref.xyz[g["row"]], g["sums"], viewpoint)
        if not fit["curvature"] <= D(F(P["max_curvature"])):
            continue
        origin, e1, e2 = fit["centroid"].astype(F), fit["e1"].astype(F), fit["e2"].astype(F)
        d = ref.xyz[g["members"]].astype(D) - origin.astype(D)[None, :]
        u = (d[:, 0] * D(e1[0]) + d[:, 1] * D(e1[1])) + d[:, 2] * D(e1[2])
        v = (d[:, 0] * D(e2[0]) + d[:, 1] * D(e2[1])) + d[:, 2] * D(e2[2])
        pr = u[:, None] * DIRS[None, :, 0].astype(D) + v[:, None] * DIRS[None, :, 1].astype(D)
        mk = keys[g["members"]]
        best = pr.max(axis=0)
        ext = np.array([np.nonzero(pr[:, k] == best[k])[0][np.argmin(mk[pr[:, k] == best[k]])] for k in range(64)])      # a tie: the smaller key
        poly = convex_hull(np.stack([u[ext].astype(F), v[ext].astype(F)], axis=1))
        pl = dict(centroid=fit["centroid"].astype(F), normal=fit["normal"].astype(F), d=float(F(fit["d"])), curvature=float(F(fit["curvature"])),
                  count=fit["count"], area_moment=float(F(fit["area_moment"])), elongation=float(F(fit["elongation"])), ppal_dir=e2.copy(),
                  color_count=0, fit=fit, n_voxels=g["n_voxels"], members=g["members"], uv_all=np.stack([u, v], axis=1), extremes=g["members"][ext],
                  root_row=g["row"], e1=e1, e2=e2)
        if len(poly):
            area, cu, cv = polygon_area_centre(poly)
            if float(np.cross(e1.astype(D), e2.astype(D)) @ fit["normal"]) < 0:       # counter-clockwise seen from the normal's side
                poly = poly[::-1]
            pl.update(area=float(F(area)), hull_points=len(poly), center_hull=(origin.astype(D) + cu * e1.astype(D) + cv * e2.astype(D)).astype(F),
                      hull=(origin.astype(D)[None, :] + poly[:, :1] * e1.astype(D)[None, :] + poly[:, 1:] * e2.astype(D)[None, :]).astype(F))
        else:
            pl.update(area=pl["area_moment"], hull_points=0, center_hull=pl["centroid"].copy(), hull=np.zeros((0, 3), F))
        passed.append(pl)
    stats["n_planes_available"] = len(passed)
    stats["n_voxels_in_planes"] = int(sum(pl["n_voxels"] for pl in passed))
    label_key3 = ref.key[S["root"]] if len(ref) else np.zeros((0, 3), np.int32)
    plane_index = np.full(len(ref), -1, np.int32)
    for a, pl in enumerate(passed):
        plane_index[pl["members"]] = a
    keep = list(range(len(passed)))
    if len(keep) > max_planes:          # the most voxels, a tie going to the smaller root key; root-key order among those kept
        keep = sorted(sorted(keep, key=lambda a: (-passed[a]["n_voxels"], a))[:max_planes])
    out = [dict(passed[a], root=o) for o, a in enumerate(keep)]
    root_key3 = np.array([ref.key[pl["root_row"]] for pl in out], np.int32).reshape(-1, 3)
    return dict(planes=out, root_key3=root_key3, stats=stats, label_key3=label_key3, plane_index=plane_index, segmentation=S)


# ---- scenes (exactly representable coordinates in cells of 0.25 m: every centroid is exact and no link lies near a threshold)
def patch(origin, a, b, na, nb, step=0.25, per_cell=1):
    """na x nb cells of a planar patch from `origin` along the unit axes a and b, one point in the middle of every cell (per_cell 1) or
    the four at its quarter points (per_cell 2)."""
    o, a, b = (np.asarray(t, D) for t in (origin, a, b))
    s = (np.arange(per_cell, dtype=D) * 2 + 1) / (2 * per_cell) * step
    ia, ib = np.meshgrid(np.arange(na, dtype=D), np.arange(nb, dtype=D), indexing="ij")
    pts = [o[None, :] + (ia.reshape(-1, 1) * step + sa) * a[None, :] + (ib.reshape(-1, 1) * step + sb) * b[None, :] for sa in s for sb in s]
    return np.concatenate(pts).astype(F)


def corner_scene(n=8, step=0.25):
    """A room corner: three n x n patches in the planes z = h, y = h, x = h (h = half a cell), meeting along the axes."""
    h = step / 2
    floor = patch((0, 0, 0), (1, 0, 0), (0, 1, 0), n, n, step) + F([0, 0, h])
    wall_y = patch((0, 0, 0), (1, 0, 0), (0, 0, 1), n, n, step) + F([0, h, 0])
    wall_x = patch((0, 0, 0), (0, 1, 0), (0, 0, 1), n, n, step) + F([h, 0, 0])
    return np.concatenate([floor, wall_y, wall_x]).astype(F)


def spiral_scene(side=30, width=3, step=0.25):
    """A strip `width` cells wide wound inwards as a square spiral in the plane z = half a cell, two empty cells between its turns: one
    region whose label has to travel the whole strip.  Returns (points, the strip's length in cells)."""
    pitch = width + 2
    legs = [side, side, side]
    s = side - pitch
    while s >= 2 * pitch:
        legs += [s, s]
        s -= pitch
    cells, length = set(), 0
    x = y = 0
    for k, leg in enumerate(legs):
        dx, dy = [(1, 0), (0, 1), (-1, 0), (0, -1)][k % 4]
        for _ in range(leg):
            for a in range(width):
                for b in range(width):
                    cells.add((x + a, y + b))
            x, y = x + dx, y + dy
            length += 1
    c = np.array(sorted(cells), D)
    pts = np.stack([(c[:, 0] + 0.5) * step, (c[:, 1] + 0.5) * step, np.full(len(c), step / 2)], axis=1)
    return pts.astype(F), length


def patches_scene(n=65, size=5, step=0.25):
    """n separate size x size patches in the plane z = half a cell on a grid with two empty cells between them."""
    per_row = 9
    pts = [patch(((k % per_row) * (size + 2) * step, (k // per_row) * (size + 2) * step, 0), (1, 0, 0), (0, 1, 0), size, size, step) + F([0, 0, step / 2])
           for k in range(n)]
    return np.concatenate(pts).astype(F)


def room_scene(step=0.05):
    """The relocalisation scene: an asymmetric room sampled as points every `step` -- a box 4.2 x 3.0 x 2.4 m with its floor, ceiling and
    four walls, a partition 1.8 m long and 2.4 m high standing off one wall, and a table top 1.2 x 0.8 m at 0.75 m -- so that the plane
    graph has no symmetry.  The surfaces lie in the middle of cells of 0.1 m.  World coordinates, float32."""
    def rect(o, a, b, la, lb):
        na, nb = int(round(la / step)), int(round(lb / step))
        ia, ib = np.meshgrid((np.arange(na) + 0.5) * step, (np.arange(nb) + 0.5) * step, indexing="ij")
        return np.asarray(o, D)[None, :] + ia.reshape(-1, 1) * np.asarray(a, D)[None, :] + ib.reshape(-1, 1) * np.asarray(b, D)[None, :]
    X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    x0, y0, z0 = -1.95, -1.25, -1.15
    parts = [rect((x0, y0, z0), X, Y, 4.2, 3.0), rect((x0, y0, z0 + 2.4), X, Y, 4.2, 3.0),          # floor, ceiling
             rect((x0, y0, z0), X, Z, 4.2, 2.4), rect((x0, y0 + 3.0, z0), X, Z, 4.2, 2.4),          # the two long walls
             rect((x0, y0, z0), Y, Z, 3.0, 2.4), rect((x0 + 4.2, y0, z0), Y, Z, 3.0, 2.4),          # the two short walls
             rect((x0 + 1.5, y0, z0), Y, Z, 1.8, 2.4),                                              # the partition
             rect((x0 + 2.4, y0 + 1.6, z0 + 0.8), X, Y, 1.2, 0.8)]                                  # the table top
    return np.concatenate(parts).astype(F)


def frame_pose(yaw_deg=25.0, t=(0.4, -0.3, 0.1)):
    """world <- frame: a yaw about z and a translation, float64."""
    a = np.radians(yaw_deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = t
    return T


def in_frame(points, T):
    """The world points expressed in the frame at T (world <- frame), float32."""
    Ti = np.linalg.inv(T)
    return (points.astype(D) @ Ti[:3, :3].T + Ti[:3, 3][None, :]).astype(F)
