"""numpy restatement of the voxel map's surface normals and of the surface cast (include/rgbd360_hip.h, "surface normals of the map";
DESIGN.md 3.20; csrc/map_normals.h), built from the restatements it extends: the 27 cells in map_align_reference.CELLS' order, the
covariance and the plane function of map_align_plane_reference, the traversal of map_raycast_reference.cast.

Input: the map of tests/voxel_map_reference.py (keys ascending, read-out centroids).  A row whose count is 0 stands for a tombstone: it
is absent everywhere.  All arithmetic is float64 + - x / sqrt on the float64 values of float32 inputs, operation for operation as the
device does it.  Independent of the library: array operations only."""
import numpy as np

import map_align_plane_reference as P
import map_align_reference as A
import map_raycast_reference as M
import voxel_map_reference as R

F = np.float32
D = np.float64
NONE, OK, UNSUPPORTED, NONPLANAR = P.NONE, P.KEPT, P.UNSUPPORTED, P.NONPLANAR
STAT_NAMES = ("n_voxels", "n_below_min_count", "n_unsupported", "n_nonplanar", "n_normals")
DEFAULTS = dict(min_count=1, min_support=5, max_flatness=0.05, max_shift=2.0)


def layer(ref, min_count=1, min_support=5, max_flatness=0.05):
    """Per row of `ref`: dict(status int32, normal [k, 3] float32 in the canonical sign, curvature float32, support int64, cov [k, 6]
    float64: the covariance handed to the plane function, zero where none was)."""
    k = len(ref)
    status = np.zeros(k, np.int32)
    normal = np.zeros((k, 3), F)
    curvature = np.zeros(k, F)
    support = np.zeros(k, np.int64)
    covs = np.zeros((k, 6), D)
    if k == 0:
        return dict(status=status, normal=normal, curvature=curvature, support=support, cov=covs)
    keys = A.packed_keys(ref.key)
    live = ref.count > 0
    rows = np.nonzero(live & (ref.count >= min_count))[0]
    i = ref.key[rows].astype(np.int64)          # the voxel's own key is the centre
    wd = ref.xyz[rows].astype(D)                # ... and its read-out centroid the point
    se, see, m = np.zeros((len(rows), 3), D), np.zeros((len(rows), 6), D), np.zeros(len(rows), np.int64)
    for d in A.CELLS:
        nb = i + np.array(d, np.int64) + R.BIAS
        ok = ((nb >= 0) & (nb < (1 << 21))).all(axis=1)
        pk = (nb[:, 2] << 42) | (nb[:, 1] << 21) | nb[:, 0]
        pos = np.minimum(np.searchsorted(keys, pk), len(keys) - 1)
        found = ok & (keys[pos] == pk) & (ref.count[pos] >= min_count) & (ref.count[pos] > 0)
        with np.errstate(invalid="ignore"):
            e = wd - ref.xyz[pos].astype(D)
        ex, ey, ez = e.T
        m += found
        se = se + np.where(found[:, None], e, 0.0)
        see = see + np.where(found[:, None], np.stack([ex * ex, ex * ey, ex * ez, ey * ey, ey * ez, ez * ez], axis=1), 0.0)
    support[rows] = m
    unsupported = m < min_support
    status[rows[unsupported]] = UNSUPPORTED
    fit = rows[~unsupported]
    _, cov = P.covariance(se[~unsupported], see[~unsupported], m[~unsupported])
    covs[fit] = cov
    n, planar, l0, _ = P.plane_fit(cov, max_flatness)
    c2 = (cov[:, 0] + cov[:, 3]) + cov[:, 5]
    with np.errstate(all="ignore"):
        curvature[fit] = np.where(c2 > 0.0, l0 / np.where(c2 > 0.0, c2, 1.0), 0.0).astype(F)
    status[fit] = np.where(planar, OK, NONPLANAR)
    n32 = n.astype(F)
    a = np.abs(n32)
    big = np.where(a[:, 1] > a[:, 0], 1, 0)
    big = np.where(a[:, 2] > a[np.arange(len(a)), big], 2, big)          # the earliest on a tie
    flip = n32[np.arange(len(a)), big] < 0
    n32 = np.where(flip[:, None], -n32, n32)
    normal[fit[planar]] = n32[planar]
    return dict(status=status, normal=normal, curvature=curvature, support=support, cov=covs)


def normals(ref, min_count=1, min_support=5, max_flatness=0.05, viewpoint=None):
    """The read-out: one record per row with count > 0, in the rows' order (keys ascending):
    dict(xyz, normal, curvature, status, count, key3, support, stats)."""
    L = layer(ref, min_count, min_support, max_flatness)
    live = np.nonzero(ref.count > 0)[0] if len(ref) else np.zeros(0, np.int64)
    nrm = L["normal"][live].copy()
    xyz = ref.xyz[live]
    st = L["status"][live]
    if viewpoint is not None and len(live):
        e = np.asarray(viewpoint, F).astype(D)[None, :] - xyz.astype(D)
        nd = nrm.astype(D)
        away = (st == OK) & (((nd[:, 0] * e[:, 0] + nd[:, 1] * e[:, 1]) + nd[:, 2] * e[:, 2]) < 0)
        nrm[away] = -nrm[away]
    cnt = ref.count[live]
    stats = dict(n_voxels=len(live), n_below_min_count=int((cnt < min_count).sum()), n_unsupported=int((st == UNSUPPORTED).sum()),
                 n_nonplanar=int((st == NONPLANAR).sum()), n_normals=int((st == OK).sum()))
    return dict(xyz=xyz, normal=nrm, curvature=L["curvature"][live], status=st, count=cnt.astype(np.int32), key3=ref.key[live],
                support=L["support"][live], stats=stats)


def cast_surface(ref, leaf, origins, dirs, min_support=5, max_flatness=0.05, max_shift=2.0, normal_min_count=1, **ray_params):
    """map_raycast_reference.cast with the surface: its dict (status, key3, count, rgb, stats unchanged) with `t` on the plane where it is
    taken, `normal` [n, 3] float32 facing the ray's origin, `on_plane` [n] bool and `n_on_plane`."""
    out = M.cast(ref, leaf, origins, dirs, **ray_params)
    n = len(out["t"])
    out["normal"] = np.zeros((n, 3), F)
    out["on_plane"] = np.zeros(n, bool)
    out["n_on_plane"] = 0
    hit = np.nonzero(out["status"] == M.HIT)[0]
    if not len(hit):
        return out
    L = layer(ref, normal_min_count, min_support, max_flatness)
    row = np.searchsorted(A.packed_keys(ref.key), A.packed_keys(out["key3"][hit]))
    ok = L["status"][row] == OK
    hit, row = hit[ok], row[ok]
    o = np.asarray(origins, F).reshape(-1, 3)[hit].astype(D)
    d = np.asarray(dirs, F).reshape(-1, 3)[hit].astype(D)
    c = ref.xyz[row].astype(D)
    n32 = L["normal"][row]
    nd = n32.astype(D)
    t_min = ray_params.get("t_min")
    t_min = D(F(leaf)) if t_min is None else D(F(t_min))
    inv = D(F(1.0) / F(leaf))
    shift2 = D(F(max_shift)) * D(F(max_shift))
    q = (nd[:, 0] * d[:, 0] + nd[:, 1] * d[:, 1]) + nd[:, 2] * d[:, 2]
    out["normal"][hit] = np.where((q > 0)[:, None], -n32, n32)
    with np.errstate(all="ignore"):
        tp = ((nd[:, 0] * (c[:, 0] - o[:, 0]) + nd[:, 1] * (c[:, 1] - o[:, 1])) + nd[:, 2] * (c[:, 2] - o[:, 2])) / q
        f = (o + tp[:, None] * d) - c
        taken = (q != 0) & (tp >= t_min) & ((((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]) * (inv * inv)) <= shift2)
        out["t"][hit[taken]] = tp[taken].astype(F)
    out["on_plane"][hit[taken]] = True
    out["n_on_plane"] = int(taken.sum())
    return out


def cast_surface_sphere(ref, leaf, rows, cols, pose, **params):
    """The panorama: dict(depth, normal, rgb, count, key3, status, on_plane, n_on_plane, stats)."""
    origins, dirs = M.sphere_rays(rows, cols, pose)
    got = cast_surface(ref, leaf, origins, dirs, **params)
    return dict(depth=got["t"].reshape(rows, cols), normal=got["normal"].reshape(rows, cols, 3), rgb=got["rgb"].reshape(rows, cols, 3),
                count=got["count"].reshape(rows, cols), key3=got["key3"].reshape(rows, cols, 3), status=got["status"].reshape(rows, cols),
                on_plane=got["on_plane"].reshape(rows, cols), n_on_plane=got["n_on_plane"], stats=got["stats"])
