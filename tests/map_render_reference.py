"""numpy restatement of the map rendered as a spherical frame (include/rgbd360_hip.h, "the map rendered as a spherical frame";
DESIGN.md 3.14; csrc/map_render.h).

Input: the map of tests/voxel_map_reference.py (keys ascending, exact integer sums).  Steps: the inverse pose formed in double and
rounded to float32; per voxel with count >= min_count the read-out's centroid; the dense alignment's warp in the DEVICE arithmetic
(csrc/photo_icp_kernels.h warp_pixel_rc with libm == 0: float32 fused multiply-adds, correctly rounded square root and reciprocal, the
odd polynomial for the arc tangent, round half up) restated here operation for operation; dist, the footprint, the smallest
(dist bits, packed key) per pixel; the four planes and the statistics.  Independent of the library: array operations only.
A fused multiply-add is not a numpy operation: fma32 forms the exact product and sum in float64 with the rounding error of the sum
(TwoSum), rounds the float64 sum to odd and then to float32 -- the correctly rounded float32 result of a * b + c.
"""
import numpy as np

import voxel_map_reference as R

F = np.float32
PI = 3.14159265359          # Miscellaneous.h:44 (level_geom.h)
STAT_NAMES = ("n_voxels", "n_below_min_count", "n_near", "n_splatted", "n_pixels_covered")
DEFAULTS = dict(min_count=1, near=None, splat=1.0, max_half=8)       # near None: leaf


def fma32(a, b, c):
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                   # exact: 24 x 24 bits
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)               # s + e == p + c exactly
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (e != 0) & even      # round to odd: the neighbour on e's side
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def atan_unit(t):
    q = [F(v) for v in (-0.3333333195069166, 0.19999765993465415, -0.14279110844310372, 0.11037993832882714, -0.08673169371217875,
                        0.06284358078457526, -0.03627014369584507, 0.01375026672953864, -0.00244702708829393)]
    s = t * t
    p = fma32(s, q[8], q[7])
    for k in range(6, -1, -1):
        p = fma32(s, p, q[k])
    return fma32(t * s, p, t)


def level_consts(rows, cols):
    """level_geom.h: angle_res_inv, half_nRows, pi_k of a level of rows x cols."""
    angle_res = F(2 * PI / cols)
    angle_res_inv = F(1) / angle_res
    return angle_res_inv, F(0.5 * rows - 0.5), F(PI * np.float64(angle_res_inv))


def inverse_pose(pose):
    """Step 1: the 12 floats (Rinv 3x3, tinv 3) of the definition."""
    T = np.asarray(pose, F).reshape(4, 4)
    Rinv = T[:3, :3].T.copy()
    t = T[:3, 3].astype(np.float64)
    tinv = np.zeros(3, F)
    for k in range(3):
        s = np.float64(T[0, k]) * t[0]
        s = s + np.float64(T[1, k]) * t[1]
        s = s + np.float64(T[2, k]) * t[2]
        tinv[k] = F(-s)
    return Rinv, tinv


def warp_device(xyz, Rm, t, rows, cols):
    """warp_pixel_rc (libm == 0) of the points xyz [n, 3] float32 at the pose (Rm, t): target row, column (int64), d2, visibility."""
    k_inv, half, pi_k = level_consts(rows, cols)
    px, py, pz = (np.ascontiguousarray(xyz[:, k], F) for k in range(3))
    with np.errstate(all="ignore"):
        X = fma32(Rm[0, 2], pz, fma32(Rm[0, 1], py, fma32(Rm[0, 0], px, t[0])))
        Y = fma32(Rm[1, 2], pz, fma32(Rm[1, 1], py, fma32(Rm[1, 0], px, t[1])))
        Z = fma32(Rm[2, 2], pz, fma32(Rm[2, 1], py, fma32(Rm[2, 0], px, t[2])))
        rho2 = fma32(Z, Z, Y * Y)
        d2 = fma32(X, X, rho2)
        rho = np.sqrt(rho2)
        ax, ay, az = np.abs(X), np.abs(Y), np.abs(Z)
        mxp, mnp = np.maximum(np.maximum(ax, rho), F(1e-9)), np.minimum(ax, rho)
        mxt, mnt = np.maximum(np.maximum(ay, az), F(1e-9)), np.minimum(ay, az)
        r = F(1) / (mxp * mxt)
        tp = mnp * (r * mxt)
        tt = mnt * (r * mxp)
        phi = atan_unit(tp)
        phi = np.where(ax > rho, F(1.57079637) - phi, phi)
        phi = np.copysign(phi, X)
        th = atan_unit(tt)
        th = np.where(ay > az, F(1.57079637) - th, th)
        th = np.where(np.signbit(Z), F(3.14159274) - th, th)
        th = np.copysign(th, Y)
        fr = fma32(phi, -k_inv, half).astype(np.float64)
        fc = fma32(th, k_inv, pi_k).astype(np.float64)
        finite = np.isfinite(fr) & np.isfinite(fc)
        tr = np.where(finite, np.floor(fr + 0.5), -1).astype(np.int64)
        tc = np.where(finite, np.floor(fc + 0.5), -1).astype(np.int64)
    vis = (tr >= 0) & (tr < rows) & (tc >= 0) & (tc < cols)
    return tr, tc, d2, vis


def packed_keys(key3):
    k = np.asarray(key3, np.int64) + R.BIAS
    return (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]


def footprint(tr, tc, h, rows, cols):
    """Step 4 for one voxel: the flat pixel indices it covers (rows clipped, columns modulo cols, every column once when 2 h + 1 >= cols)."""
    rr = np.arange(max(tr - h, 0), min(tr + h, rows - 1) + 1)
    cc = np.arange(cols) if 2 * h + 1 >= cols else np.arange(tc - h, tc + h + 1) % cols
    return (rr[:, None] * cols + cc[None, :]).ravel()


def half_width(dist, leaf, cols, splat, max_half):
    k_inv, _, _ = level_consts(1, cols)
    foot = (F(splat) * F(leaf)) * k_inv
    with np.errstate(all="ignore"):
        q = foot * (F(1) / dist)
        return np.where(q >= F(max_half), max_half, np.where(q > 0, np.trunc(q), 0)).astype(np.int64)


def resolve(pix, bits, keys):
    """Step 5: per pixel the candidate of smallest (bits, key); returns (pixels, index of the winner among the candidates)."""
    order = np.lexsort((keys, bits, pix))
    first = np.ones(len(order), bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    return pix[order][first], order[first]


def render(ref, leaf, rows, cols, pose, min_count=1, near=None, splat=1.0, max_half=8):
    """ref: voxel_map_reference.Map.  Returns dict(depth, rgb, count, key3, stats)."""
    near = F(leaf) if near is None else F(near)
    n = rows * cols
    out = dict(depth=np.zeros((rows, cols), F), rgb=np.zeros((rows, cols, 3), np.uint8), count=np.zeros((rows, cols), np.int32),
               key3=np.zeros((rows, cols, 3), np.int32), stats=dict.fromkeys(STAT_NAMES, 0))
    if n == 0 or len(ref) == 0:
        return out
    takes = ref.count >= min_count
    idx = np.nonzero(takes)[0]
    Rinv, tinv = inverse_pose(pose)
    tr, tc, d2, vis = warp_device(ref.xyz[idx], Rinv, tinv, rows, cols)
    with np.errstate(all="ignore"):
        dist = np.sqrt(d2)
        on = vis & np.isfinite(dist) & (dist >= near)
    h = half_width(dist, leaf, cols, splat, max_half)
    keys = packed_keys(ref.key[idx])
    bits = dist.view(np.uint32).astype(np.int64)
    sel = np.nonzero(on)[0]
    pixels = [footprint(int(tr[j]), int(tc[j]), int(h[j]), rows, cols) for j in sel]
    stats = out["stats"]
    stats.update(n_voxels=len(ref), n_below_min_count=int((~takes).sum()), n_near=int((~on).sum()), n_splatted=len(sel))
    out["n_atomics"] = int(sum(len(p) for p in pixels))
    if len(sel):
        which = np.repeat(sel, [len(p) for p in pixels])
        pix, win = resolve(np.concatenate(pixels), bits[which], keys[which])
        v = idx[which[win]]
        out["depth"].reshape(-1)[pix] = dist[which[win]]
        out["rgb"].reshape(-1, 3)[pix] = ref.rgb[v]
        out["count"].reshape(-1)[pix] = ref.count[v]
        out["key3"].reshape(-1, 3)[pix] = ref.key[v]
        stats["n_pixels_covered"] = len(pix)
    return out


def assert_render_equals(got, want, what=""):
    """got: (depth, rgb, count, key3, stats) of the device; bit for bit."""
    depth, rgb, count, key3, stats = got
    assert {k: int(stats[k]) for k in STAT_NAMES} == want["stats"], (what, stats, want["stats"])
    assert np.array_equal(count, want["count"]), what
    assert np.array_equal(key3, want["key3"]), what
    assert depth.tobytes() == want["depth"].tobytes(), what
    assert np.array_equal(rgb, want["rgb"]), what
