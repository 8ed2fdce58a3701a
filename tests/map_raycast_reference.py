"""numpy restatement of ray casting through the voxel map (include/rgbd360_hip.h, "ray casting through the map"; DESIGN.md 3.19;
csrc/map_raycast.h).

Input: the map of tests/voxel_map_reference.py (keys ascending, exact integer sums, read-out centroids).  All traversal arithmetic is
float64 + - x / on the float64 values of the float32 inputs, which numpy performs operation for operation as the device does (no fused
multiply-add).  Steps: the bad-ray test; g = o inv_leaf, u = d inv_leaf, r = 1 / u; the boundary times T_k(b) = (b - g_k) r_k; the clip
against the box of the live keys; the start cell; per cell the limits, t_out with the lowest axis on ties, the candidate test with the
centroid's projection, the advance.  Plain one-level traversal only: the device's coarse layer has to give these bits too.  The one
number that depends on the form of the traversal, n_lookups, is restated for both (`layer`).  Independent of the library: array
operations only, all rays in lock step.
"""
import math

import numpy as np

import voxel_map_reference as R

F = np.float32
D = np.float64
PI = 3.14159265359          # Miscellaneous.h:44 (level_geom.h)
MISS_BOX, HIT, LEFT_BOX, T_MAX, MAX_STEPS, BAD = range(6)
STAT_NAMES = ("n_rays", "n_hits", "n_miss_box", "n_left_box", "n_t_max", "n_max_steps", "n_bad_rays", "n_steps", "n_lookups")
DEFAULTS = dict(min_count=1, t_min=None, t_max=np.inf, max_offset=np.inf, max_steps=8192)       # t_min None: leaf


def packed_keys(key3):
    k = np.asarray(key3, np.int64) + R.BIAS
    return (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]


def sphere_rays(rows, cols, pose):
    """The rays of the panorama's pixels, row-major: (origins, dirs) [rows * cols, 3] float32.  The angles are the dense alignment's
    float32 expressions; sine and cosine are taken in double (the C library's, through math) and rounded to float32."""
    T = np.asarray(pose, F).reshape(4, 4)
    angle_res = F(2 * PI / cols)
    half = F(0.5 * rows - 0.5)
    theta = np.arange(cols).astype(F) * angle_res
    phi = (half - np.arange(rows).astype(F)) * angle_res
    st = np.array([math.sin(float(v)) for v in theta], F)
    ct = np.array([math.cos(float(v)) for v in theta], F)
    sp = np.array([math.sin(float(v)) for v in phi], F)
    cp = np.array([math.cos(float(v)) for v in phi], F)
    fx = np.broadcast_to(sp[:, None], (rows, cols)).ravel()
    fy = ((-cp)[:, None] * st[None, :]).ravel()
    fz = ((-cp)[:, None] * ct[None, :]).ravel()
    dirs = np.stack([(T[k, 0] * fx + T[k, 1] * fy) + T[k, 2] * fz for k in range(3)], axis=1).astype(F)
    origins = np.broadcast_to(T[:3, 3], (rows * cols, 3)).astype(F)
    return origins, dirs


def cast(ref, leaf, origins, dirs, min_count=1, t_min=None, t_max=np.inf, max_offset=np.inf, max_steps=8192, layer=True):
    """ref: voxel_map_reference.Map.  Returns dict(t, key3, count, rgb, status, stats) for the n rays."""
    o32 = np.asarray(origins, F).reshape(-1, 3)
    d32 = np.asarray(dirs, F).reshape(-1, 3)
    n = len(o32)
    out = dict(t=np.zeros(n, F), key3=np.zeros((n, 3), np.int32), count=np.zeros(n, np.int32), rgb=np.zeros((n, 3), np.uint8),
               status=np.zeros(n, np.int32), stats=dict.fromkeys(STAT_NAMES, 0))
    if n == 0 or len(ref) == 0:
        return out
    t_min = D(F(leaf)) if t_min is None else D(F(t_min))
    t_max = D(F(t_max))
    off2_max = D(F(max_offset)) * D(F(max_offset))
    inv = D(F(1.0) / F(leaf))
    keys = packed_keys(ref.key)
    lo = ref.key.min(axis=0).astype(np.int64)
    hi = ref.key.max(axis=0).astype(np.int64)
    o, d = o32.astype(D), d32.astype(D)
    status = np.full(n, -1, np.int64)
    steps = np.zeros(n, np.int64)
    lookups = np.zeros(n, np.int64)
    bad = ~(np.isfinite(o32).all(axis=1) & np.isfinite(d32).all(axis=1)) | (d32 == 0).all(axis=1)
    status[bad] = BAD
    ok = ~bad
    o, d = np.where(ok[:, None], o, 0.0), np.where(ok[:, None], d, 1.0)        # (the bad rays run along as dummies and are masked out)
    with np.errstate(all="ignore"):
        g, u = o * inv, d * inv
        st = np.sign(u).astype(np.int64)
        r = np.where(st != 0, 1.0 / np.where(st != 0, u, 1.0), 0.0)
        up = (st > 0).astype(np.int64)

        def T_of(b):
            """The times at the boundaries b [n, 3] (integers)."""
            return np.where(st != 0, (b.astype(D) - g) * r, np.inf)

        ta, tc = T_of(np.broadcast_to(lo, (n, 3))), T_of(np.broadcast_to(hi + 1, (n, 3)))
        near = np.where(st != 0, np.minimum(ta, tc), -np.inf)
        far = np.where(st != 0, np.maximum(ta, tc), np.inf)
        t0 = np.maximum(0.0, near.max(axis=1))
        t1 = far.min(axis=1)
        inside = (st != 0) | ((g >= lo) & (g < hi + 1))
        miss = ok & (~inside.all(axis=1) | (t0 > t1))
        status[miss] = MISS_BOX
        p = np.floor(g + t0[:, None] * u)
        i = np.clip(np.where(np.isfinite(p), p, 0.0), lo, hi).astype(np.int64)
        T = T_of(i + up)
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        t_in = t0.copy()
        hit_row = np.full(n, -1, np.int64)
        t_hit = np.zeros(n, D)
        act = np.nonzero(status < 0)[0]
        while len(act):
            over = t_in[act] > t_max
            status[act[over]] = T_MAX
            act = act[~over]
            full = steps[act] >= max_steps
            status[act[full]] = MAX_STEPS
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
            hit = cand & (th >= t_min) & ~(off2 > off2_max)
            status[act[hit]] = HIT
            hit_row[act[hit]] = pos[hit]
            t_hit[act[hit]] = th[hit]
            act, a, t_out = act[~hit], a[~hit], t_out[~hit]
            i[act, a] += st[act, a]
            left = (i[act, a] < lo[a]) | (i[act, a] > hi[a])
            T[act, a] = (((i[act, a] + up[act, a]).astype(D)) - g[act, a]) * r[act, a]
            t_in[act] = t_out
            status[act[left]] = LEFT_BOX
            act = act[~left]
    h = status == HIT
    out["status"] = status.astype(np.int32)
    out["t"][h] = t_hit[h].astype(F)
    out["key3"][h] = ref.key[hit_row[h]]
    out["count"][h] = ref.count[hit_row[h]]
    out["rgb"][h] = ref.rgb[hit_row[h]]
    out["stats"] = dict(n_rays=n, n_hits=int(h.sum()), n_miss_box=int((status == MISS_BOX).sum()), n_left_box=int((status == LEFT_BOX).sum()),
                        n_t_max=int((status == T_MAX).sum()), n_max_steps=int((status == MAX_STEPS).sum()), n_bad_rays=int((status == BAD).sum()),
                        n_steps=int(steps.sum()), n_lookups=int(lookups.sum()))
    return out


def cast_sphere(ref, leaf, rows, cols, pose, **params):
    """The panorama: dict(depth, rgb, count, key3, stats) in the shapes of map_render_reference.render."""
    out = dict(depth=np.zeros((rows, cols), F), rgb=np.zeros((rows, cols, 3), np.uint8), count=np.zeros((rows, cols), np.int32),
               key3=np.zeros((rows, cols, 3), np.int32), stats=dict.fromkeys(STAT_NAMES, 0))
    if rows * cols == 0 or len(ref) == 0:
        return out
    origins, dirs = sphere_rays(rows, cols, pose)
    got = cast(ref, leaf, origins, dirs, **params)
    out.update(depth=got["t"].reshape(rows, cols), rgb=got["rgb"].reshape(rows, cols, 3), count=got["count"].reshape(rows, cols),
               key3=got["key3"].reshape(rows, cols, 3), stats=got["stats"], status=got["status"].reshape(rows, cols))
    return out


def assert_cast_equals(got, want, what=""):
    """got: (t, key3, count, rgb, status, stats) of the device; bit for bit."""
    t, key3, count, rgb, status, stats = got
    assert np.array_equal(status, want["status"]), (what, np.nonzero(status != want["status"])[0][:10])
    assert {k: int(stats[k]) for k in STAT_NAMES} == want["stats"], (what, stats, want["stats"])
    assert np.array_equal(key3, want["key3"]), what
    assert np.array_equal(count, want["count"]), what
    assert t.tobytes() == want["t"].tobytes(), (what, np.nonzero(t != want["t"])[0][:10])
    assert np.array_equal(rgb, want["rgb"]), what


def assert_sphere_equals(got, want, what=""):
    """got: (depth, rgb, count, key3, stats) of the device; bit for bit."""
    depth, rgb, count, key3, stats = got
    assert {k: int(stats[k]) for k in STAT_NAMES} == want["stats"], (what, stats, want["stats"])
    assert np.array_equal(count, want["count"]), what
    assert np.array_equal(key3, want["key3"]), what
    assert depth.tobytes() == want["depth"].tobytes(), what
    assert np.array_equal(rgb, want["rgb"]), what
