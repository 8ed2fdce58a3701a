"""numpy restatement of free-space observation and carving of the voxel map (include/rgbd360_hip.h, "free-space observation and carving
of the map"; csrc/map_carve.h).

Input: the map of tests/voxel_map_reference.py.  A measurement is a segment o -> w; d = w - o in float32, the measurement lies at t = 1.
The walk is that of tests/map_raycast_reference.py (the same float64 + - x / on the float64 values of the float32 inputs: g = o inv_leaf,
u = d inv_leaf, r = 1 / u, T_k(b) = (b - g_k) r_k, the clip against the box of the live keys, the start cell, t_out with the lowest axis
on ties, the advance) with t_max = 1, and it does not end at a candidate: every live cell of count >= min_count is tested for a
through-vote; the voxel that w would feed (voxel_map_reference.voxel_index) gets an end-vote.  Plain one-level traversal only: the
device's coarse layer has to give these bits too; n_lookups is restated for both forms (`layer`).  Independent of the library: array
operations only, all segments in lock step.
"""
import copy

import numpy as np

import map_raycast_reference as M
import voxel_map_reference as R

F = np.float32
D = np.float64
STAT_NAMES = ("n_rays", "n_valid", "n_skipped", "n_miss_box", "n_max_steps", "n_steps", "n_lookups", "n_through", "n_end", "n_voxels_voted")
CARVE_STAT_NAMES = ("n_voted", "n_voxels_carved", "n_points_carved", "n_protected_end", "n_protected_count", "n_voxels")
DEFAULTS = dict(min_count=1, near=None, margin_leaves=2.0, margin_rel=0.0, max_offset=0.5, max_steps=8192)       # near None: leaf


def _empty(ref, n=0):
    return dict(through=np.zeros(len(ref), np.int64), end=np.zeros(len(ref), np.int64), stats=dict.fromkeys(STAT_NAMES, 0))


def _observe(ref, leaf, o32, w32, pre_valid, min_count=1, near=None, margin_leaves=2.0, margin_rel=0.0, max_offset=0.5, max_steps=8192, layer=True):
    n = len(o32)
    out = _empty(ref)
    if n == 0 or len(ref) == 0:
        return out
    near = D(F(leaf)) if near is None else D(F(near))
    near2 = near * near
    mrel = D(F(margin_rel))
    margin = D(F(margin_leaves)) * D(F(leaf))
    margin2 = margin * margin
    off2_max = D(F(max_offset)) * D(F(max_offset))
    inv32 = F(1.0) / F(leaf)
    inv = D(inv32)
    keys = M.packed_keys(ref.key)
    lo = ref.key.min(axis=0).astype(np.int64)
    hi = ref.key.max(axis=0).astype(np.int64)
    with np.errstate(all="ignore"):
        d32 = (w32 - o32).astype(F)
        valid = pre_valid & np.isfinite(o32).all(axis=1) & (np.isfinite(w32) & (np.abs(w32) < F(4096.0))).all(axis=1)
        valid &= np.isfinite(d32).all(axis=1) & ~(d32 == 0).all(axis=1)
    through, end = out["through"], out["end"]
    status = np.full(n, -1, np.int64)
    status[~valid] = M.BAD
    steps = np.zeros(n, np.int64)
    lookups = np.zeros(n, np.int64)
    o = np.where(valid[:, None], o32.astype(D), 0.0)        # (the invalid ones run along as dummies and are masked out)
    d = np.where(valid[:, None], d32.astype(D), 1.0)
    with np.errstate(all="ignore"):
        g, u = o * inv, d * inv
        st = np.sign(u).astype(np.int64)
        r = np.where(st != 0, 1.0 / np.where(st != 0, u, 1.0), 0.0)
        up = (st > 0).astype(np.int64)

        def T_of(b):
            return np.where(st != 0, (b.astype(D) - g) * r, np.inf)

        ta, tc = T_of(np.broadcast_to(lo, (n, 3))), T_of(np.broadcast_to(hi + 1, (n, 3)))
        near_t = np.where(st != 0, np.minimum(ta, tc), -np.inf)
        far_t = np.where(st != 0, np.maximum(ta, tc), np.inf)
        t0 = np.maximum(0.0, near_t.max(axis=1))
        t1 = far_t.min(axis=1)
        inside = (st != 0) | ((g >= lo) & (g < hi + 1))
        miss = valid & (~inside.all(axis=1) | (t0 > t1))
        status[miss] = M.MISS_BOX
        p = np.floor(g + t0[:, None] * u)
        i = np.clip(np.where(np.isfinite(p), p, 0.0), lo, hi).astype(np.int64)
        T = T_of(i + up)
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        t_in = t0.copy()
        act = np.nonzero(status < 0)[0]
        while len(act):
            over = t_in[act] > 1.0
            status[act[over]] = M.T_MAX
            act = act[~over]
            full = steps[act] >= max_steps
            status[act[full]] = M.MAX_STEPS
            act = act[~full]
            if not len(act):
                break
            steps[act] += 1
            a = np.argmin(T[act], axis=1)              # the first of equal minima: the lowest axis index
            t_out = T[act, a]
            pk = ((i[act, 2] + R.BIAS) << 42) | ((i[act, 1] + R.BIAS) << 21) | (i[act, 0] + R.BIAS)
            pos = np.minimum(np.searchsorted(keys, pk), len(keys) - 1)
            live = keys[pos] == pk
            lookups[act] += live if layer else 1
            cand = live & (ref.count[pos] >= min_count)
            c = ref.xyz[pos].astype(D)
            e = c - o[act]
            s = ((e[:, 0] * d[act, 0] + e[:, 1] * d[act, 1]) + e[:, 2] * d[act, 2]) / dd[act]
            th = np.minimum(np.maximum(s, t_in[act]), t_out)
            f = e - s[:, None] * d[act]
            off2 = ((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]) * (inv * inv)
            q = (1.0 - th) - mrel
            vote = cand & ((th * th) * dd[act] >= near2) & (q >= 0.0) & ((q * q) * dd[act] >= margin2) & (off2 <= off2_max)
            np.add.at(through, pos[vote], 1)
            i[act, a] += st[act, a]
            left = (i[act, a] < lo[a]) | (i[act, a] > hi[a])
            T[act, a] = (((i[act, a] + up[act, a]).astype(D)) - g[act, a]) * r[act, a]
            t_in[act] = t_out
            status[act[left]] = M.LEFT_BOX
            act = act[~left]
        # the end-votes: the voxel the measurement would feed
        ie = np.floor(np.where(valid[:, None], w32, F(0.0)) * inv32).astype(np.int64)
    pk = ((ie[:, 2] + R.BIAS) << 42) | ((ie[:, 1] + R.BIAS) << 21) | (ie[:, 0] + R.BIAS)
    pos = np.minimum(np.searchsorted(keys, pk), len(keys) - 1)
    ends = valid & (keys[pos] == pk)
    np.add.at(end, pos[ends], 1)
    out["stats"] = dict(n_rays=n, n_valid=int(valid.sum()), n_skipped=int((~valid).sum()), n_miss_box=int((status == M.MISS_BOX).sum()),
                        n_max_steps=int((status == M.MAX_STEPS).sum()), n_steps=int(steps.sum()), n_lookups=int(lookups.sum()),
                        n_through=int(through.sum()), n_end=int(end.sum()), n_voxels_voted=int(((through + end) > 0).sum()))
    return out


def observe_rays(ref, leaf, origins, endpoints, **params):
    """ref: voxel_map_reference.Map.  dict(through [len(ref)], end [len(ref)], stats) of the n segments."""
    o32 = np.asarray(origins, F).reshape(-1, 3)
    w32 = np.asarray(endpoints, F).reshape(-1, 3)
    return _observe(ref, leaf, o32, w32, np.ones(len(o32), bool), **params)


def observe_cloud(ref, leaf, xyz, pose, **params):
    """A sphere frame as its cloud xyz [n, 3] float32 in the frame's coordinates (the pixel's point, step 1 of the map's definition) at
    `pose`: steps 3 and 4 of the map's definition, no box; o = the pose's translation."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    T = np.asarray(pose, F).reshape(4, 4)
    w32 = R.transform(xyz, T)
    o32 = np.broadcast_to(T[:3, 3], w32.shape).astype(F)
    return _observe(ref, leaf, o32, w32, np.isfinite(xyz).all(axis=1), **params)


def add(a, b):
    """The votes of observation `a` with those of `b` accumulated: the sums; the statistics of the two calls stay their own, but
    n_voxels_voted of the second counts the voxels it voted first."""
    out = dict(through=a["through"] + b["through"], end=a["end"] + b["end"], stats=dict(b["stats"]))
    out["stats"]["n_voxels_voted"] = int((((b["through"] + b["end"]) > 0) & ((a["through"] + a["end"]) == 0)).sum())
    return out


def votes(ref, ob, carved=None):
    """The read-out: (key3, through, end, count) of the voxels with a vote, ascending by (i_z, i_y, i_x) -- ref's order; carved: the mask
    of the voxels a carve erased (their count reads 0)."""
    has = (ob["through"] + ob["end"]) > 0
    count = ref.count.copy()
    if carved is not None:
        count[carved] = 0
    return ref.key[has].astype(np.int32), ob["through"][has].astype(np.int32), ob["end"][has].astype(np.int32), count[has].astype(np.int32)


def carve(ref, ob, min_through=1, max_end=0, max_count=0):
    """(mask [len(ref)] of the voxels erased, the statistics)."""
    voted = (ob["through"] + ob["end"]) > 0
    seen = voted & (ob["through"] >= min_through)
    end_ok = ob["end"] <= max_end
    count_ok = np.ones(len(ref), bool) if max_count == 0 else ref.count <= max_count
    erased = seen & end_ok & count_ok
    stats = dict(n_voted=int(voted.sum()), n_voxels_carved=int(erased.sum()), n_points_carved=int(ref.count[erased].sum()),
                 n_protected_end=int((seen & ~end_ok).sum()), n_protected_count=int((seen & end_ok & ~count_ok).sum()),
                 n_voxels=len(ref) - int(erased.sum()))
    return erased, stats


def without(ref, erased):
    """The map with the voxels of the mask deleted."""
    out = copy.copy(ref)
    keep = ~erased
    for name in ("count", "S", "C", "key", "xyz", "rgb"):
        setattr(out, name, getattr(ref, name)[keep])
    return out


def points_in(ref, erased, xyz, pose, leaf, box):
    """How many of a frame's points (steps 1-5 of the map's definition) fall in the voxels of the mask."""
    w, _, _ = R.passing(xyz, pose, box)
    i = R.voxel_index(w, leaf)
    pk = ((i[:, 2] + R.BIAS) << 42) | ((i[:, 1] + R.BIAS) << 21) | (i[:, 0] + R.BIAS)
    return int(np.isin(pk, M.packed_keys(ref.key[erased])).sum())


def assert_observation_equals(got_stats, got_votes, ref, want, what="", lookups=True):
    """got_stats: the device's statistics; got_votes: its read-out (key3, through, end, count); bit for bit."""
    names = [k for k in STAT_NAMES if lookups or k != "n_lookups"]
    assert {k: int(got_stats[k]) for k in names} == {k: want["stats"][k] for k in names}, (what, got_stats, want["stats"])
    key3, through, end, count = votes(ref, want)
    assert np.array_equal(got_votes[0], key3), what
    assert np.array_equal(got_votes[1], through), (what, np.nonzero(got_votes[1] != through)[0][:10])
    assert np.array_equal(got_votes[2], end), what
    assert np.array_equal(got_votes[3], count), what
