"""numpy restatement of the voxel map's definition (include/rgbd360_hip.h, "resident voxel-grid global map").

Per point, in this order: finite test, box (frame coordinates, limits included), pose in float32 with every product and sum rounded
on its own, range (|w| < 4096), voxel index floor(w * inv_leaf) with inv_leaf = float32(1) / float32(leaf), exact integer sums
(count, rint(double(w) * 2^20) in int64, r, g, b).  Read-out: centroid = float32(double(S) / (double(count) * 2^20)), colour =
S_c // count, sorted by (i_z, i_y, i_x).  Independent of the library: array operations only, no code shared with it.
"""
import numpy as np

FIX = 1048576.0
BIAS = 1 << 20
DEFAULT_BOX = (np.array([-2.0, -4.0, -4.0], np.float32), np.array([1.0, 4.0, 4.0], np.float32))      # FilterPointCloud.h:66-71
STAT_NAMES = ("n_valid", "n_box_rejected", "n_out_of_range", "n_added", "n_dropped_full", "n_voxels")


def general_pose():
    """30 degrees about the skew axis (1, 2, 3), translation (0.7, -1.3, 0.4); world <- frame, float32."""
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(30.0)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = [0.7, -1.3, 0.4]
    return T.astype(np.float32)


def transform(xyz, pose):
    """w_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k, float32 operands throughout."""
    T = np.asarray(pose, np.float32).reshape(4, 4)
    x, y, z = (np.ascontiguousarray(xyz[:, k], np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        return np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)], axis=1)


def passing(xyz, pose, box):
    """Steps 1-4: (world points of the points that pass [m, 3] float32, their indices into xyz, the three counters)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    finite = np.isfinite(xyz).all(axis=1)
    inbox = finite.copy()
    if box is not None:
        lo, hi = (np.asarray(b, np.float32) for b in box)
        with np.errstate(invalid="ignore"):
            inbox &= ((lo[None, :] <= xyz) & (xyz <= hi[None, :])).all(axis=1)
    w = transform(xyz, pose)
    with np.errstate(invalid="ignore"):
        inrange = inbox & (np.isfinite(w) & (np.abs(w) < np.float32(4096.0))).all(axis=1)
    idx = np.nonzero(inrange)[0]
    counters = dict(n_valid=int(finite.sum()), n_box_rejected=int((finite & ~inbox).sum()), n_out_of_range=int((inbox & ~inrange).sum()))
    return w[idx], idx, counters


def voxel_index(w, leaf):
    inv_leaf = np.float32(1.0) / np.float32(leaf)
    return np.floor(w * inv_leaf).astype(np.int64)


class Map:
    """The map after a list of clouds [(xyz [n, 3] float32, rgb [n, 3] uint8 or None, pose 4x4), ...] in a table that never fills."""

    def __init__(self, clouds, leaf, box=DEFAULT_BOX):
        keys, fixed, cols, self.stats = [], [], [], []
        seen = np.zeros(0, np.int64)
        for xyz, rgb, pose in clouds:
            w, idx, st = passing(xyz, pose, box)
            i = voxel_index(w, leaf)
            packed = ((i[:, 2] + BIAS) << 42) | ((i[:, 1] + BIAS) << 21) | (i[:, 0] + BIAS)
            keys.append(packed)
            fixed.append(np.rint(w.astype(np.float64) * FIX).astype(np.int64))
            cols.append(np.zeros((len(idx), 3), np.int64) if rgb is None else np.asarray(rgb, np.uint8).reshape(-1, 3)[idx].astype(np.int64))
            seen = np.union1d(seen, packed)
            st.update(n_added=len(idx), n_dropped_full=0, n_voxels=len(seen))
            self.stats.append(st)
        packed = np.concatenate(keys) if keys else np.zeros(0, np.int64)
        uniq, inverse = np.unique(packed, return_inverse=True)      # ascending packed keys = ascending (i_z, i_y, i_x)
        m = len(uniq)
        self.n_passing = len(packed)
        self.count = np.zeros(m, np.int64)
        np.add.at(self.count, inverse, 1)
        self.S = np.zeros((m, 3), np.int64)
        self.C = np.zeros((m, 3), np.int64)
        if m:
            np.add.at(self.S, inverse, np.concatenate(fixed))
            np.add.at(self.C, inverse, np.concatenate(cols))
        self.key = np.stack([(uniq & 0x1fffff) - BIAS, ((uniq >> 21) & 0x1fffff) - BIAS, (uniq >> 42) - BIAS], axis=1).astype(np.int32)
        self.xyz = (self.S.astype(np.float64) / (self.count.astype(np.float64) * FIX)[:, None]).astype(np.float32)
        self.rgb = (self.C // np.maximum(self.count, 1)[:, None]).astype(np.uint8)

    def __len__(self):
        return len(self.count)


def assert_map_equals(got, ref, what=""):
    """got: (xyz, rgb, count, key) of an extract call; bit for bit, order included."""
    xyz, rgb, count, key = got
    assert len(count) == len(ref), (what, len(count), len(ref))
    assert np.array_equal(key, ref.key), what
    assert np.array_equal(count.astype(np.int64), ref.count), what
    assert xyz.tobytes() == ref.xyz.tobytes(), what
    assert np.array_equal(rgb, ref.rgb), what


def edge_cases():
    """Hand-made clouds (under 200 points in all) around every decision of the definition:
    [(name, xyz, rgb, pose, leaf, box), ...]."""
    f = np.float32
    up, down = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    eye = np.eye(4, dtype=np.float32)
    h = f(2.0) ** -21
    cases = []
    # signs and cell boundaries, no box: -0.0 and 0.0 share cell 0, -0.01 lies in cell -1 (floor, not truncation), 0.25 = 5 cells of
    # 0.05 (inv_leaf is 20.0f exactly) starts cell 5 and its predecessor ends cell 4, likewise on the negative side
    pts = [(-0.0, 0.0, -0.0), (0.0, -0.0, 0.0), (-0.01, -0.01, -0.01), (0.01, 0.01, 0.01), (0.25, 0.25, 0.25), (down(0.25),) * 3,
           (up(0.25),) * 3, (-0.25, -0.25, -0.25), (down(-0.25),) * 3, (up(-0.25),) * 3, (0.05, 0.1, 0.15), (-0.05, -0.1, -0.15),
           (1e-30, -1e-30, 1e-38), (h, -h, 3 * h), (5 * h, -3 * h, 7 * h),      # odd halves of the fixed-point unit 2^-20: to even
           (3.999, -3.999, 3.999), (100.0, -200.0, 300.0), (4095.999, -4095.999, 0.0)]
    # not finite: skipped and not counted as valid; |w| = 4096: out of range; the float below 4096: kept
    pts += [(np.nan, 0, 0), (0, np.nan, 0), (0, 0, np.nan), (np.inf, 0, 0), (0, -np.inf, 0), (np.nan, np.inf, -np.inf),
            (4096.0, 0, 0), (0, -4096.0, 0), (0, 0, 4096.0), (down(4096.0), up(-4096.0), down(4096.0)), (1e9, 0, 0), (0, 0, -3e38)]
    xyz = np.array(pts, np.float32)
    rgb = (np.arange(xyz.size, dtype=np.int64).reshape(-1, 3) * 37 % 256).astype(np.uint8)
    cases.append(("signs, boundaries, range; no box", xyz, rgb, eye, 0.05, None))
    cases.append(("the same in cells of 0.25 m, no colour", xyz, None, eye, 0.25, None))
    # the default box: its limits are kept, the neighbouring floats are not
    lo, hi = DEFAULT_BOX
    pts = []
    for k in range(3):
        for v, inside in ((lo[k], up(lo[k])), (hi[k], down(hi[k]))):
            for val in (v, inside, down(v) if v == lo[k] else up(v)):
                p = [0.5, 0.5, 0.5]
                p[k] = val
                pts.append(tuple(p))
    pts += [(lo[0], lo[1], lo[2]), (hi[0], hi[1], hi[2]), (lo[0], hi[1], lo[2]), (-2.5, 0, 0), (0, 5, 0), (0, 0, -4.5), (np.nan, 0, 0)]
    xyz = np.array(pts, np.float32)
    rgb = (np.arange(xyz.size, dtype=np.int64).reshape(-1, 3) * 91 % 256).astype(np.uint8)
    cases.append(("box limits, identity", xyz, rgb, eye, 0.05, DEFAULT_BOX))
    cases.append(("box limits, general pose", xyz, rgb, general_pose(), 0.05, DEFAULT_BOX))
    # the range test looks at the POSED point: a translation carries x = 4095 onto 4096 (dropped) and x = 4097 back inside (kept)
    T = eye.copy()
    T[0, 3] = 1.0
    xyz = np.array([(4095.0, 0, 0), (down(4095.0), 0, 0), (-4097.0, 0, 0), (up(-4097.0), 0, 0), (-4096.5, 1, 1), (0, 0, 0)], np.float32)
    cases.append(("range after the pose", xyz, None, T, 0.05, None))
    T2 = general_pose()
    T2[:3, 3] = [4000.0, -4000.0, 10.0]
    xyz = np.array([(x, y, 0.3) for x in (-150.0, -50.0, 0.0, 50.0, 96.0, 150.0) for y in (-150.0, 0.0, 96.0, 150.0)], np.float32)
    cases.append(("range after a general pose", xyz, None, T2, 0.004, None))
    assert sum(len(c[1]) for c in cases) <= 200
    return cases
