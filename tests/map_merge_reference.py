"""numpy restatement of composing voxel maps (include/rgbd360_hip.h, "composing maps: merge at a pose, exact un-merge, table records";
csrc/map_merge.h) on top of voxel_map_reference.py and voxel_map_edit_reference.py.

The source of a merge: the live voxels (count >= min_count) of a map, given as any object with the attributes of voxel_map_reference.Map
(key, count, S, C, xyz).  Sum mode: the key is kept, the seven words are added.  Pose mode, per source voxel: c = its read-out centroid
(float32), w = pose c in float32 with every product and sum rounded on its own, dropped unless |w_k| < 4096 and n < 2^31, the destination
voxel floor(w * inv_leaf) at the DESTINATION's leaf, terms n, n rint(double(w) 2^20), the colour sums as they are.  Un-merge takes the same
terms off in removal's manner: a key that is not there makes its points missing; a voxel asked for more than it holds gives what it
holds, the rest is underflow and its sums are left alone.  Array operations only, no code shared with the library."""
import numpy as np

import voxel_map_edit_reference as E
import voxel_map_reference as R

DEFAULT_MIN_COUNT = 1
MAX_COUNT = 1 << 31            # a posed voxel's and a record's count stay below it
STAT_NAMES = ("n_voxels_read", "n_points_read", "n_voxels_below_min_count", "n_points_below_min_count", "n_voxels_out_of_range",
              "n_points_out_of_range", "n_voxels_added", "n_points_added", "n_voxels_new", "n_voxels_dropped", "n_points_dropped", "n_missing",
              "n_underflow", "n_voxels")
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def pack(key3):
    k = np.asarray(key3, np.int64).reshape(-1, 3)
    return ((k[:, 2] + R.BIAS) << 42) | ((k[:, 1] + R.BIAS) << 21) | (k[:, 0] + R.BIAS)


def records_of(m):
    """The live voxels of a Map-like object as rgbd360_map_records gives them: uint64 [n, 8], ascending key."""
    live = np.asarray(m.count) > 0
    rec = np.zeros((int(live.sum()), 8), np.int64)
    rec[:, 0] = pack(m.key[live])
    rec[:, 1] = m.count[live]
    rec[:, 2:5] = m.S[live]
    rec[:, 5:8] = m.C[live]
    return rec[np.argsort(rec[:, 0], kind="stable")].view(np.uint64)


def terms(src, pose, dst_leaf, min_count=DEFAULT_MIN_COUNT):
    """(packed destination keys [m], int64 rows [m, 7] = (n, n fix(w) or S, C), the counters of the source side) of a merge of `src`."""
    live = np.asarray(src.count) > 0
    n = np.asarray(src.count, np.int64)[live]
    st = dict(n_voxels_read=len(n), n_points_read=int(n.sum()))
    below = n < min_count
    st.update(n_voxels_below_min_count=int(below.sum()), n_points_below_min_count=int(n[below].sum()))
    rows = np.zeros((len(n), 7), np.int64)
    rows[:, 0] = n
    rows[:, 4:7] = np.asarray(src.C, np.int64)[live]
    if pose is None:
        keep = ~below
        keys = pack(src.key[live])
        rows[:, 1:4] = np.asarray(src.S, np.int64)[live]
    else:
        c = (np.asarray(src.S, np.int64)[live].astype(np.float64) / (n.astype(np.float64) * R.FIX)[:, None]).astype(np.float32)
        w = R.transform(c, pose)
        with np.errstate(invalid="ignore"):
            inrange = (np.isfinite(w) & (np.abs(w) < np.float32(4096.0))).all(axis=1) & (n < MAX_COUNT)
        keep = ~below & inrange
        safe = np.where(keep[:, None], w, np.float32(0.0))
        keys = pack(R.voxel_index(safe, dst_leaf))
        rows[:, 1:4] = n[:, None] * np.rint(safe.astype(np.float64) * R.FIX).astype(np.int64)
        out = ~below & ~inrange
        st.update(n_voxels_out_of_range=int(out.sum()), n_points_out_of_range=int(n[out].sum()))
    st.setdefault("n_voxels_out_of_range", 0)
    st.setdefault("n_points_out_of_range", 0)
    return keys[keep], rows[keep], st


class MergeMap(E.EditMap):
    """voxel_map_edit_reference.EditMap (insert, remove, rehash, census, read_out) with merge, unmerge and add_records; the table never
    fills."""

    def _add(self, keys, rows, st):
        new = 0
        for k, r in zip(keys.tolist(), rows):
            held = self.rows.get(k)
            new += 1 if held is None or held[0] == 0 else 0
            self.rows[k] = r.copy() if held is None else held + r
        st.update(n_voxels_added=len(keys), n_points_added=int(rows[:, 0].sum()) if len(keys) else 0, n_voxels_new=new, n_voxels_dropped=0,
                  n_points_dropped=0, n_missing=0, n_underflow=0, n_voxels=len(self))
        return st

    def merge(self, src, pose=None, min_count=DEFAULT_MIN_COUNT):
        return self._add(*terms(src, pose, self.leaf, min_count))

    def unmerge(self, src, pose=None, min_count=DEFAULT_MIN_COUNT):
        keys, rows, st = terms(src, pose, self.leaf, min_count)
        full = taken = emptied = short = missing = underflow = 0
        for k, r in zip(keys.tolist(), rows):
            held = self.rows.get(k)
            if held is None:
                missing += int(r[0])
                short += 1
                continue
            take = min(int(held[0]), int(r[0]))
            taken += take
            emptied += 1 if take and take == int(held[0]) else 0
            if take == int(r[0]):
                self.rows[k] = held - r
                full += 1
            else:               # the count is clamped, the sums are left alone
                underflow += int(r[0]) - take
                short += 1
                held = held.copy()
                held[0] -= take
                self.rows[k] = held
        st.update(n_voxels_added=full, n_points_added=taken, n_voxels_new=emptied, n_voxels_dropped=short, n_points_dropped=missing + underflow,
                  n_missing=missing, n_underflow=underflow, n_voxels=len(self))
        return st

    def add_records(self, records):
        rec = np.ascontiguousarray(records, np.uint64).reshape(-1, 8)
        if bad_records(rec).any():
            raise ValueError("%d bad records" % int(bad_records(rec).sum()))
        rows = rec[:, 1:].view(np.int64)
        st = dict(n_voxels_read=len(rec), n_points_read=int(rows[:, 0].sum()), n_voxels_below_min_count=0, n_points_below_min_count=0,
                  n_voxels_out_of_range=0, n_points_out_of_range=0)
        return self._add(rec[:, 0].view(np.int64), rows, st)


def bad_records(records):
    """Per record: it breaks a rule of rgbd360_map_add_records (the key is the empty marker or 2^63 and above, the count is outside
    1 .. 2^31 - 1, a colour sum exceeds 255 count, an |S_k| reaches count 2^32)."""
    rec = np.ascontiguousarray(records, np.uint64).reshape(-1, 8)
    key, count = rec[:, 0], rec[:, 1]
    bad = (key == EMPTY_KEY) | (key >> np.uint64(63) != 0) | (count == 0) | (count >= np.uint64(MAX_COUNT))
    n = np.minimum(count, np.uint64(MAX_COUNT)).astype(object)      # Python integers: no product wraps
    S = rec[:, 2:5].view(np.int64).astype(object)
    col = rec[:, 5:8].astype(object)
    for k in range(3):
        bad |= np.array([abs(s) >= c << 32 for s, c in zip(S[:, k], n)], bool) | np.array([v > 255 * c for v, c in zip(col[:, k], n)], bool)
    return bad


def check_stats_add_up(st):
    for unit in ("voxels", "points"):
        total = sum(st["n_%s_%s" % (unit, part)] for part in ("below_min_count", "out_of_range", "dropped", "added"))
        assert st["n_%s_read" % unit] == total, (unit, st)


def census_rules_hold(rows):
    """The census rules on int64 rows [m, 7] with count > 0: colour sums <= 255 count, |S_k| < count 2^32."""
    n = rows[:, 0]
    return bool((n > 0).all() and (rows[:, 4:7] <= 255 * n[:, None]).all() and (rows[:, 4:7] >= 0).all() and
                (np.abs(rows[:, 1:4]) < (n << 32)[:, None]).all())
