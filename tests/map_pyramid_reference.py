"""numpy restatement of the map pyramid and of coarse-to-fine ICP against it (include/rgbd360_hip.h, "the map pyramid and coarse-to-fine
ICP against it"; csrc/map_pyramid.h) on top of voxel_map_reference.py, map_align_reference.py and
map_align_plane_reference.py.  Level s of a map: one voxel per distinct (i_x >> s, i_y >> s, i_z >> s) (arithmetic shifts) over its
voxels, the integer sums added.  The chain: the single-level alignment on levels top_shift .. 0, each from the pose the level before
ended on; a level that does not end OK hands on the pose it was given.  Independent of the library: array operations only."""
import numpy as np

import map_align_plane_reference as P
import map_align_reference as A
import voxel_map_reference as R

F = np.float32
MAX_SHIFT = 6


def level_leaf(leaf, s):
    """leaf 2^s in float32 (exact), as a Python float."""
    return float(F(leaf) * F(2.0 ** s))


class Level:
    """The shift-merge of a voxel_map_reference.Map (or of another Level) by s: the attributes of a Map, in ascending (i_z, i_y, i_x)."""

    def __init__(self, m, s):
        assert 1 <= s <= MAX_SHIFT
        live = m.count > 0
        k = m.key[live].astype(np.int64) >> s        # numpy's >> on signed integers is arithmetic: -1 >> 1 = -1, -2 >> 1 = -1
        packed = ((k[:, 2] + R.BIAS) << 42) | ((k[:, 1] + R.BIAS) << 21) | (k[:, 0] + R.BIAS) if len(k) else np.zeros(0, np.int64)
        uniq, inverse = np.unique(packed, return_inverse=True)
        n = len(uniq)
        self.count = np.zeros(n, np.int64)
        self.S = np.zeros((n, 3), np.int64)
        self.C = np.zeros((n, 3), np.int64)
        if n:
            np.add.at(self.count, inverse, m.count[live])
            np.add.at(self.S, inverse, m.S[live])
            np.add.at(self.C, inverse, m.C[live])
        self.key = np.stack([(uniq & 0x1fffff) - R.BIAS, ((uniq >> 21) & 0x1fffff) - R.BIAS, (uniq >> 42) - R.BIAS], axis=1).astype(np.int32)
        self.xyz = (self.S.astype(np.float64) / (self.count.astype(np.float64) * R.FIX)[:, None]).astype(F)
        self.rgb = (self.C // np.maximum(self.count, 1)[:, None]).astype(np.uint8)
        self.n_points = int(self.count.sum())

    def __len__(self):
        return len(self.count)


def straddling_points():
    """Points in the cells -4 .. 3 of every axis at leaf 0.25 (inv_leaf = 4 exactly), two per cell, the cell's lower face among them, and two
    beside the origin: (xyz [n, 3] float32, rgb [n, 3] uint8)."""
    v = np.array([c * 0.25 + o for c in range(-4, 4) for o in (0.0, 0.13)], F)
    pts = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=3).reshape(-1, 3)
    pts = np.concatenate([pts, np.array([(-0.0, 0.0, -0.0), (-1e-30, 1e-30, -1e-30)], F)])
    rgb = (np.arange(pts.size, dtype=np.int64).reshape(-1, 3) * 53 % 256).astype(np.uint8)
    return pts, rgb


def assert_words_equal(a, b, what=""):
    """Two maps word for word: keys, counts, coordinate and colour sums (and with them the read-out)."""
    assert len(a) == len(b), (what, len(a), len(b))
    assert np.array_equal(a.key, b.key), what
    assert np.array_equal(a.count, b.count) and np.array_equal(a.S, b.S) and np.array_equal(a.C, b.C), what
    assert a.xyz.tobytes() == b.xyz.tobytes() and np.array_equal(a.rgb, b.rgb), what


class Chain:
    """levels: one record per level from the coarsest down, dict(shift, leaf, max_dist, pose_in, al) with al the Alignment /
    PlaneAlignment of that level; pose and status: level 0's.  `maps` may hold levels already merged, {shift: Level}."""

    def __init__(self, target, xyz, guess, leaf, box, top_shift=3, kind=0, max_dist_leaves=1.0, max_iters=10, eps=1e-6, min_count=1, min_matches=6,
                 min_support=5, max_flatness=0.05, maps=None):
        maps = {} if maps is None else maps
        pose = np.asarray(guess, F).reshape(4, 4).copy()
        self.levels = []
        for s in range(top_shift, -1, -1):
            if s and s not in maps:
                maps[s] = Level(target, s)
            lf = level_leaf(leaf, s)
            max_dist = F(max_dist_leaves) * F(lf)
            if kind == 0:
                al = A.Alignment(maps[s] if s else target, xyz, pose, lf, box, max_dist, max_iters, eps, min_count, min_matches)
            else:
                al = P.PlaneAlignment(maps[s] if s else target, xyz, pose, lf, box, max_dist, max_iters, eps, min_count, min_matches, min_support, max_flatness)
            self.levels.append(dict(shift=s, leaf=lf, max_dist=max_dist, pose_in=pose, al=al))
            if al.status == A.OK:
                pose = al.pose
        last = self.levels[-1]["al"]
        self.pose, self.status = last.pose, last.status
        self.margins = [m for lv in self.levels for m in lv["al"].margins]
