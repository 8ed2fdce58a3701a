"""numpy restatement of the voxel map's editing (include/rgbd360_hip.h, "editing the map"), built on
voxel_map_reference: a map as a dict {packed key: int64 row [count, Sx, Sy, Sz, Sr, Sg, Sb]} with insert / remove / census.

Removal, per point: steps 1-5 of the map's definition, then count -= 1, S_k -= rint(double(w_k) * 2^20), S_c -= colour_c.  A row whose
count reaches 0 stays in the dict (a tombstone) and is absent from the read-out.  Outside the contract, per voxel: a key that is not in
the dict makes its points missing; a voxel asked for more points than it holds gives min(held, asked), the rest is underflow, and
the sums of such a voxel are left alone (the content is then unspecified: only the counts are compared).  Array operations only, no
code shared with the library.
"""
import numpy as np

import voxel_map_reference as R

EDIT_STAT_NAMES = ("n_valid", "n_box_rejected", "n_out_of_range", "n_removed", "n_missing", "n_underflow", "n_voxels_emptied", "n_voxels")


def rows_of(xyz, rgb, pose, leaf, box):
    """One cloud as (sorted unique packed keys, their int64 rows [count, S(3), C(3)], the three counters of steps 1-4)."""
    w, idx, st = R.passing(xyz, pose, box)
    i = R.voxel_index(w, leaf)
    packed = ((i[:, 2] + R.BIAS) << 42) | ((i[:, 1] + R.BIAS) << 21) | (i[:, 0] + R.BIAS)
    terms = np.zeros((len(idx), 7), np.int64)
    terms[:, 0] = 1
    terms[:, 1:4] = np.rint(w.astype(np.float64) * R.FIX).astype(np.int64)
    if rgb is not None:
        terms[:, 4:7] = np.asarray(rgb, np.uint8).reshape(-1, 3)[idx].astype(np.int64)
    uniq, inverse = np.unique(packed, return_inverse=True)
    rows = np.zeros((len(uniq), 7), np.int64)
    np.add.at(rows, inverse, terms)
    return uniq, rows, st


class EditMap:
    def __init__(self, leaf, box=R.DEFAULT_BOX):
        self.leaf, self.box = leaf, box
        self.rows = {}           # packed key -> int64[7]; count 0: a tombstone

    def insert(self, xyz, rgb, pose):
        keys, rows, st = rows_of(xyz, rgb, pose, self.leaf, self.box)
        for k, r in zip(keys.tolist(), rows):
            self.rows[k] = self.rows.get(k, 0) + r
        st.update(n_added=int(rows[:, 0].sum()), n_dropped_full=0, n_voxels=len(self))
        return st

    def remove(self, xyz, rgb, pose):
        keys, rows, st = rows_of(xyz, rgb, pose, self.leaf, self.box)
        removed = missing = underflow = emptied = 0
        for k, r in zip(keys.tolist(), rows):
            if k not in self.rows:
                missing += int(r[0])
                continue
            held = self.rows[k]
            take = min(int(held[0]), int(r[0]))
            removed += take
            underflow += int(r[0]) - take
            emptied += 1 if take and take == int(held[0]) else 0
            if take == int(r[0]):
                self.rows[k] = held - r
            else:
                held = held.copy()
                held[0] -= take
                self.rows[k] = held
        st.update(n_removed=removed, n_missing=missing, n_underflow=underflow, n_voxels_emptied=emptied, n_voxels=len(self))
        return st

    def rehash(self):
        self.rows = {k: r for k, r in self.rows.items() if r[0] > 0}

    def __len__(self):
        return sum(1 for r in self.rows.values() if r[0] > 0)

    def census(self):
        all_rows = np.array(list(self.rows.values()), np.int64).reshape(-1, 7)
        count = all_rows[:, 0]
        live = count > 0
        bad = (~live & (all_rows[:, 1:] != 0).any(axis=1)) | (live & ((all_rows[:, 4:] > 255 * count[:, None]).any(axis=1) |
                                                                      (np.abs(all_rows[:, 1:4]) >= (count << 32)[:, None]).any(axis=1)))
        return dict(n_live=int(live.sum()), n_tombstones=int((~live).sum()), n_points=int(count[live].sum()), n_inconsistent=int(bad.sum()))

    def read_out(self):
        """The live voxels as an object with the fields of voxel_map_reference.Map (key, count, S, C, xyz, rgb), in its order."""
        keys = np.array(sorted(k for k, r in self.rows.items() if r[0] > 0), np.int64)
        rows = np.array([self.rows[k] for k in keys.tolist()], np.int64).reshape(-1, 7)
        out = R.Map([], self.leaf, self.box)
        out.count, out.S, out.C = rows[:, 0], rows[:, 1:4], rows[:, 4:7]
        out.key = np.stack([(keys & 0x1fffff) - R.BIAS, ((keys >> 21) & 0x1fffff) - R.BIAS, (keys >> 42) - R.BIAS], axis=1).astype(np.int32)
        out.xyz = (out.S.astype(np.float64) / (out.count.astype(np.float64) * R.FIX)[:, None]).astype(np.float32)
        out.rgb = (out.C // np.maximum(out.count, 1)[:, None]).astype(np.uint8)
        return out


def assert_same_map(a, b, what=""):
    """Two read-outs (voxel_map_reference.Map fields) agree in every field."""
    assert len(a) == len(b), (what, len(a), len(b))
    for name in ("key", "count", "S", "C", "rgb"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)
    assert a.xyz.tobytes() == b.xyz.tobytes(), what
