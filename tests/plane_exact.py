"""Plain references for the plane stage of Frame360 (rgbd360_plane_fit and the chains that end in it), numpy only.

Independent of the library and of oracle/frame360_ref.cpp: the link predicate restated, connected components by union-find with
min-hooking, the region sums as exact int64 sums of 2^-28 m (m^2) terms, and the host's conversion of those sums into centroids and
covariances.  tests/test_plane_regions_exact.py holds the device against them.

Exactness:
- link_flags evaluates the predicate in float32, one rounding per operation.  The kernel may contract a product and a sum into an fma,
  so the tests build inputs on which both agree: dyadic coordinates and normals whose products are exact.
- region_sums: float32 coordinates make every float64 product x * y * 2^28 exact, np.rint rounds half to even like the kernel's
  magic-constant conversion, and the int64 sums wrap modulo 2^64 as the device's do.
- derived: (double)(long long)s / 2^28, / N, and the covariance of rgbd360_frame360.hip, operation for operation: centroids come out
  bit-exact.  Eigen-quantities come from float64 eigh; the host's solver is another one, so they agree to a stated bound only.
"""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

SCALE = float(1 << 28)          # kMomScale


def libc_cosf(angle: float) -> np.float32:
    """cosf of the C library, as the host evaluates cosf(angular_threshold)."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.cosf.restype = ctypes.c_float
    libm.cosf.argtypes = [ctypes.c_float]
    return np.float32(libm.cosf(np.float32(angle)))


def link_flags(xyz, nrm, rows, cols, angular_threshold, distance_threshold, depth_mode=0):
    """(left, up) booleans of k_f360_link_flags: both points finite, |w - w'| < dist_thr z^2 (z, the threshold, of the pixel itself,
    the right / lower one), n . n' > cosf(angular_threshold), w = p . n; strict compares."""
    p = np.asarray(xyz, np.float32).reshape(rows, cols, 3)
    q = np.asarray(nrm, np.float32).reshape(rows, cols, 3)
    cos_thr = libc_cosf(angular_threshold)
    dthr = np.float32(distance_threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(p).all(axis=2)
        w = (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]
        if depth_mode == 0:
            z = p[..., 2]
        else:
            z = np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])
        th = (dthr * z) * z

        def linked(a, b, o):      # a: the pixel itself, b: its neighbour, o: slices
            dot = (q[a][..., 0] * q[b][..., 0] + q[a][..., 1] * q[b][..., 1]) + q[a][..., 2] * q[b][..., 2]
            return fin[a] & fin[b] & (np.abs(w[a] - w[b]) < th[a]) & (dot > cos_thr)

        left = np.zeros((rows, cols), bool)
        up = np.zeros((rows, cols), bool)
        left[:, 1:] = linked((slice(None), slice(1, None)), (slice(None), slice(None, -1)), None)
        up[1:, :] = linked((slice(1, None), slice(None)), (slice(None, -1), slice(None)), None)
    return fin, left, up


def components(fin, left, up):
    """Labels of the link graph: per pixel the smallest flat index of its component, -1 where the point is not finite."""
    rows, cols = fin.shape
    n = rows * cols
    idx = np.arange(n, dtype=np.int64).reshape(rows, cols)
    a = np.concatenate([idx[left], idx[up]])
    b = np.concatenate([idx[left] - 1, idx[up] - cols])
    parent = np.arange(n, dtype=np.int64)
    while True:
        pa, pb = parent[a], parent[b]
        lo, hi = np.minimum(pa, pb), np.maximum(pa, pb)
        m = lo != hi
        if not m.any():
            break
        np.minimum.at(parent, hi[m], lo[m])          # roots hook to a smaller root: no cycles, the root ends up the smallest index
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        a, b = a[m], b[m]
    lab = parent.astype(np.int32)
    lab[~fin.reshape(-1)] = -1
    return lab.reshape(rows, cols)


def label_image(xyz, nrm, rows, cols, angular_threshold, distance_threshold, depth_mode=0):
    return components(*link_flags(xyz, nrm, rows, cols, angular_threshold, distance_threshold, depth_mode))


def terms(xyz):
    """The nine 2^-28 fixed-point terms of every point (x, y, z, xx, xy, xz, yy, yz, zz) as float64 (exact products, rounded half to even)."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.rint(np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], axis=1) * SCALE)


_PAIRS = [(0, None), (1, None), (2, None), (0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def terms_column(p, k):
    """Term k of terms() for float32 points p (N x 3)."""
    a, b = _PAIRS[k]
    v = p[:, a].astype(np.float64)
    if b is not None:
        v = v * p[:, b].astype(np.float64)
    return np.rint(v * SCALE)


def region_sums(xyz, labels, roots):
    """int64 sums (wrapping like the device's) and counts of the pixels labelled with each of `roots`."""
    lab = np.asarray(labels).reshape(-1)
    roots = np.asarray(roots, np.int64)
    sel = np.nonzero(np.isin(lab, roots))[0]
    slot = np.searchsorted(np.sort(roots), lab[sel])
    by = np.argsort(slot, kind="stable")
    sel, slot = sel[by], slot[by]
    p = np.asarray(xyz, np.float32).reshape(-1, 3)[sel]
    counts = np.bincount(slot, minlength=len(roots)).astype(np.int64)
    sums = np.zeros((len(roots), 9), np.int64)
    if sel.size:
        starts = np.searchsorted(slot, np.arange(len(roots)))
        has = counts > 0
        for k in range(9):             # one term at a time: a 4096 x 2048 frame is 8 M points
            t = terms_column(p, k)
            assert not (np.abs(t) >= 2.0 ** 63).any(), "a single term beyond int64: outside what these references model"
            with np.errstate(over="ignore"):
                sums[has, k] = np.add.reduceat(t.astype(np.int64), starts[has])
    order = np.argsort(roots)
    out_s, out_c = np.empty_like(sums), np.empty_like(counts)
    out_s[order], out_c[order] = sums, counts
    return out_s, out_c


def region_sums_exact(xyz, labels, root):
    """Python-integer sums of one region (no wrap): what the int64 sums must equal when they are in range."""
    lab = np.asarray(labels).reshape(-1)
    t = terms(np.asarray(xyz, np.float32).reshape(-1, 3)[lab == root])
    return [sum(int(v) for v in t[:, k]) for k in range(9)], int((lab == root).sum())


def regions(labels, min_inliers):
    """Roots (ascending: PCL's order) and counts of the components with more than min_inliers points."""
    lab = np.asarray(labels).reshape(-1)
    r, c = np.unique(lab[lab >= 0], return_counts=True)
    keep = c > min_inliers
    return r[keep], c[keep]


def derived(sums, count):
    """The host's decoding of one region's sums: centroid (float64, as the host rounds it to float), covariance C, and the
    descriptors from float64 eigh: curvature, area_moment, elongation, ppal_dir, normal and the eigenvalues (ascending)."""
    m = [float(int(s)) / SCALE for s in sums]
    N = float(count)
    cx, cy, cz = m[0] / N, m[1] / N, m[2] / N
    C = np.array([[m[3] / N - cx * cx, m[4] / N - cx * cy, m[5] / N - cx * cz],
                  [m[4] / N - cx * cy, m[6] / N - cy * cy, m[7] / N - cy * cz],
                  [m[5] / N - cx * cz, m[7] / N - cy * cz, m[8] / N - cz * cz]])
    ev, vec = np.linalg.eigh(C)
    tr = C[0, 0] + C[1, 1] + C[2, 2]
    l1, l2 = max(ev[1], 0.0), max(ev[2], 0.0)
    v = vec[:, 0].copy()
    if -(cx * v[0] + cy * v[1] + cz * v[2]) < 0:
        v = -v
    return dict(centroid=np.array([cx, cy, cz]), C=C, ev=ev, curvature=abs(ev[0] / tr) if tr != 0 else 0.0,
                area_moment=12.0 * np.sqrt(l1 * l2), elongation=np.sqrt(l2 / l1) if l1 > 0 else np.inf,
                ppal_dir=vec[:, 2], normal=v)


def mom_in_range(count, max_abs):
    """The library's a-priori bound (f360_mom_in_range): every term and every sum of the region stays exact."""
    t = float(np.float32(max_abs)) ** 2 * SCALE
    return t < 2.0 ** 51 and count * (t + 1.0) < 2.0 ** 63
