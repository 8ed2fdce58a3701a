"""numpy restatement of the depth-model trainer (include/rgbd360_hip.h, "training the depth model"; csrc/depth_train.h):
steps 1-6 of an example, the gates of the two routes, the pinhole rays in float32, the finalisation and the file writer.  The cast is
tests/map_normals_reference.cast_surface, imported.  All example arithmetic is float64 + - x / floor on the float64 values of float32
inputs, operation for operation as the device does it.  Independent of the library: array operations only."""
import struct

import numpy as np

import map_normals_reference as N
import map_raycast_reference as M

F = np.float32
D = np.float64
FIX = 1048576.0
STAT_NAMES = ("n_pixels", "n_no_measurement", "n_no_hit", "n_off_plane", "n_grazing", "n_out_of_range", "n_mult_rejected", "n_examples")
DEFAULTS = dict(require_plane=1, min_cos_incidence=0.0, min_mult=0.7, max_mult=1.3, max_range=10.0)


def num_bins(bin_depth):
    return int(np.ceil(10.0 / bin_depth))


def shape_of(width, height, bin_width, bin_height, bin_depth):
    assert width % bin_width == 0 and height % bin_height == 0
    return (height // bin_height, width // bin_width, num_bins(bin_depth))


def metres(img):
    """An image as float32 metres: uint16 millimetres are scaled 0.001f * (float)v in float32."""
    a = np.asarray(img)
    return F(0.001) * a.astype(F) if a.dtype == np.uint16 else a.astype(F)


def measured(meas32):
    with np.errstate(invalid="ignore"):
        return np.isfinite(meas32) & (meas32 > 0)


class Sums:
    def __init__(self, width, height, bin_width=8, bin_height=6, bin_depth=2.0, smoothing=1):
        self.width, self.height, self.bin_width, self.bin_height, self.bin_depth, self.smoothing = width, height, bin_width, bin_height, bin_depth, smoothing
        self.shape = shape_of(width, height, bin_width, bin_height, bin_depth)
        self.count, self.num, self.den = (np.zeros(self.shape, np.int64) for _ in range(3))

    def examples(self, gt32, meas32, reached, min_mult=0.7, max_mult=1.3, max_range=10.0, **_):
        """Steps 2-6 over the pixels of `reached` (they passed step 1 and their route's gates): (n_out_of_range, n_mult_rejected,
        n_examples)."""
        nby, nbx, nb = self.shape
        v, u = np.nonzero(reached)
        gt, meas = gt32[v, u].astype(D), meas32[v, u].astype(D)
        rng = (meas > D(F(max_range))) | (gt > D(F(max_range)))
        with np.errstate(all="ignore"):
            mult = gt / meas
        rej = ~rng & ((mult > D(F(max_mult))) | (mult < D(F(min_mult))))
        keep = ~rng & ~rej
        v, u, gt, meas = v[keep], u[keep], gt[keep], meas[keep]
        idx = np.minimum(nb - 1, np.floor(meas / D(self.bin_depth)).astype(np.int64))
        by, bx = np.minimum(v // self.bin_height, nby - 1), np.minimum(u // self.bin_width, nbx - 1)
        np.add.at(self.count, (by, bx, idx), 1)
        np.add.at(self.num, (by, bx, idx), np.rint(gt * gt * FIX).astype(np.int64))
        np.add.at(self.den, (by, bx, idx), np.rint(gt * meas * FIX).astype(np.int64))
        return int(rng.sum()), int(rej.sum()), int(keep.sum())

    def accumulate_images(self, gt, meas, **params):
        """The image route: the statistics as a dict."""
        gt32, meas32 = metres(gt), metres(meas)
        assert gt32.shape == meas32.shape == (self.height, self.width)
        with np.errstate(invalid="ignore"):
            has_gt = np.isfinite(gt32) & (gt32 > 0)
        has_meas = measured(meas32)
        n_rng, n_rej, n_ex = self.examples(gt32, meas32, has_gt & has_meas, **params)
        return dict(n_pixels=gt32.size, n_no_measurement=int((has_gt & ~has_meas).sum()), n_no_hit=int((~has_gt).sum()), n_off_plane=0, n_grazing=0,
                    n_out_of_range=n_rng, n_mult_rejected=n_rej, n_examples=n_ex)

    def accumulate_map(self, cast, meas, require_plane=1, min_cos_incidence=0.0, **params):
        """The map route on the cast of the image's rays (cast_pinhole below): (gt_out, the statistics)."""
        meas32 = metres(meas)
        assert meas32.shape == (self.height, self.width)
        has_meas = measured(meas32)
        hit = has_meas & cast["hit"]
        off_plane = hit & ~cast["on_plane"] if require_plane else np.zeros_like(hit)
        rest = hit & ~off_plane
        mc = D(F(min_cos_incidence))
        grazing = rest & (~cast["has_normal"] | (np.abs(cast["q"]) < mc * np.sqrt(cast["dd"]))) if mc > 0 else np.zeros_like(hit)
        reached = rest & ~grazing
        n_rng, n_rej, n_ex = self.examples(cast["t"], meas32, reached, **params)
        stats = dict(n_pixels=meas32.size, n_no_measurement=int((~has_meas).sum()), n_no_hit=int((has_meas & ~cast["hit"]).sum()),
                     n_off_plane=int(off_plane.sum()), n_grazing=int(grazing.sum()), n_out_of_range=n_rng, n_mult_rejected=n_rej, n_examples=n_ex)
        return np.where(reached, cast["t"], F(0)).astype(F), stats

    def add(self, other):
        self.count += other.count
        self.num += other.num
        self.den += other.den

    def model_bytes(self):
        return model_bytes(self.width, self.height, self.bin_width, self.bin_height, self.bin_depth, self.smoothing, self.count, self.num, self.den)


def pinhole_rays(rows, cols, fx, fy, cx, cy, pose):
    """The rays of a sensor's pixels, row-major: (origins, dirs) [rows * cols, 3] float32; f = ((u - cx) / fx, (v - cy) / fy, 1) and the
    rotation in float32, every operation rounded on its own."""
    T = np.asarray(pose, F).reshape(4, 4)
    u = np.arange(cols).astype(F)
    v = np.arange(rows).astype(F)
    fxs = np.broadcast_to(((u - F(cx)) / F(fx))[None, :], (rows, cols)).ravel().astype(F)
    fys = np.broadcast_to(((v - F(cy)) / F(fy))[:, None], (rows, cols)).ravel().astype(F)
    fzs = np.ones(rows * cols, F)
    dirs = np.stack([(T[k, 0] * fxs + T[k, 1] * fys) + T[k, 2] * fzs for k in range(3)], axis=1).astype(F)
    origins = np.broadcast_to(T[:3, 3], (rows * cols, 3)).astype(F)
    return origins, dirs


def cast_pinhole(ref, leaf, rows, cols, fx, fy, cx, cy, pose, **cast_params):
    """The surface cast of every pixel's ray (the gates pick afterwards; a ray is a function of its pixel alone) as image planes:
    t float32, hit, on_plane, has_normal bool, q = n . d and dd = |d|^2 float64."""
    o, d = pinhole_rays(rows, cols, fx, fy, cx, cy, pose)
    got = N.cast_surface(ref, leaf, o, d, **cast_params)
    n32 = got["normal"]
    nd, dd = n32.astype(D), d.astype(D)
    q = (nd[:, 0] * dd[:, 0] + nd[:, 1] * dd[:, 1]) + nd[:, 2] * dd[:, 2]       # (|q| is that of the canonical normal: a negation is exact)
    d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    sh = (rows, cols)
    return dict(t=got["t"].reshape(sh), hit=(got["status"] == M.HIT).reshape(sh), on_plane=got["on_plane"].reshape(sh),
                has_normal=(n32 != 0).any(axis=1).reshape(sh), q=q.reshape(sh), dd=d2.reshape(sh), origins=o, dirs=d)


def finalise(count, num, den, smoothing):
    """(counts, numerators, denominators, multipliers) float32, of the sums' shape."""
    N_ = D(smoothing) + num.astype(D) * D(1.0 / FIX)
    D_ = D(smoothing) + den.astype(D) * D(1.0 / FIX)
    with np.errstate(all="ignore"):
        mult = np.where(D_ == 0, F(1), (N_ / np.where(D_ == 0, 1.0, D_)).astype(F)).astype(F)
    return (D(smoothing) + count.astype(D)).astype(F), N_.astype(F), D_.astype(F), mult


def model_bytes(width, height, bin_width, bin_height, bin_depth, smoothing, count, num, den):
    """The model file of the sums: DiscreteDepthDistortionModel::serialize's layout."""
    nby, nbx, nb = shape_of(width, height, bin_width, bin_height, bin_depth)
    vecs = finalise(np.asarray(count), np.asarray(num), np.asarray(den), smoothing)
    out = [b"DiscreteDepthDistortionModel v01\n", struct.pack("<iiii", width, height, bin_width, bin_height), struct.pack("<d", bin_depth),
           struct.pack("<ii", nbx, nby)]
    for y in range(nby):
        for x in range(nbx):
            out.append(struct.pack("<d", 10.0) + struct.pack("<i", nb) + struct.pack("<d", bin_depth))
            for vec in vecs:
                out.append(struct.pack("<iii", 4, nb, 1) + vec[y, x].astype("<f4").tobytes())
    return b"".join(out)
