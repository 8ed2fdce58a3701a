"""numpy restatement of applying a depth model (include/rgbd360_hip.h, "applying the depth models on the device"; DESIGN.md 3.30;
csrc/depth_apply.h): the model file read and written by the layout csrc/depth_model.h states, DiscreteFrustum's index / undistort /
interpolatedUndistort as a SCALAR float64 loop, operation for operation, the two millimetre conversions, the cloud formation of the rig
calibration, and the evaluation's integer sums.  Independent of the library.  Also the models and depth images the tests share."""
import lzma
import os
import struct

import numpy as np

import depth_train_reference as T

F = np.float32
D = np.float64
EVAL_FIX = 1073741824.0          # 2^30
EVAL_NAMES = ("n", "raw_e", "raw_ee", "cor_e", "cor_ee")
GOLDEN_MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_models")
MAGIC = b"DiscreteDepthDistortionModel v01\n"


# ---- the file
def read_model(path, downsample=1):
    """{width, height, bin_width, bin_height, nbx, nby, bin_depth, frustums: [(bin_depth, num_bins, counts f32, multipliers f32)]} of a
    model file, sizes divided by `downsample` as DiscreteDepthDistortionModel::downsampleParams does."""
    raw = open(path, "rb").read()
    assert raw.startswith(MAGIC)
    at = len(MAGIC)
    w, h, bw, bh = struct.unpack_from("<iiii", raw, at)
    bd, = struct.unpack_from("<d", raw, at + 16)
    nbx, nby = struct.unpack_from("<ii", raw, at + 24)
    at += 32
    frustums = []
    for _ in range(nbx * nby):
        _, nb, fbd = struct.unpack_from("<did", raw, at)
        at += 20
        vecs = []
        for _ in range(4):
            four, r, c = struct.unpack_from("<iii", raw, at)
            assert four == 4
            vecs.append(np.frombuffer(raw, "<f4", r * c, at + 12).copy())
            at += 12 + 4 * r * c
        frustums.append((fbd, nb, vecs[0], vecs[3]))
    assert at == len(raw) and bw % downsample == 0 and bh % downsample == 0
    return dict(width=w // downsample, height=h // downsample, bin_width=bw // downsample, bin_height=bh // downsample, nbx=nbx, nby=nby, bin_depth=bd,
                frustums=frustums)


def model_bytes(width, height, bin_width, bin_height, bin_depth, nbx, nby, frustums):
    """A model file whose frustums are (bin_depth, counts, multipliers): every frustum its own num_bins and bin_depth."""
    out = [MAGIC, struct.pack("<iiii", width, height, bin_width, bin_height), struct.pack("<d", bin_depth), struct.pack("<ii", nbx, nby)]
    for fbd, counts, mult in frustums:
        nb = len(counts)
        out.append(struct.pack("<d", 10.0) + struct.pack("<i", nb) + struct.pack("<d", fbd))
        for vec in (counts, np.ones(nb), np.ones(nb), mult):
            out.append(struct.pack("<iii", 4, nb, 1) + np.asarray(vec, "<f4").tobytes())
    return b"".join(out)


# ---- the per-pixel arithmetic
def undistort_px(frustum, z):
    """depthmodel::slice_of + undistort_px on one float32 z > 0."""
    fbd, nb, counts, mult = frustum
    bd = D(fbd)
    with np.errstate(all="ignore"):
        q = np.floor(D(z) / bd)
        if not (q < D(nb - 1)):
            idx = nb - 1
        else:
            idx = -1 if q < 0 else int(q)
        start = F(bd * D(idx))
        idx1 = idx if D(F(z - start)) < bd / D(2) else idx + 1
        idx0 = idx1 - 1
        if idx0 < 0 or idx1 >= nb or counts[idx0] < 50 or counts[idx1] < 50:
            return F(z * mult[max(idx, 0)])
        z0 = D(idx0 + 1) * bd - bd * D(0.5)
        coeff1 = (D(z) - z0) / bd
        coeff0 = D(1.0) - coeff1
        m = coeff0 * D(mult[idx0]) + coeff1 * D(mult[idx1])
        return F(D(z) * m)


def undistort(model, depth):
    """depthmodel::undistort: the corrected copy of a float32 image of the model's size; 0, negative and NaN pixels keep their bits."""
    depth = np.asarray(depth, F)
    assert depth.shape == (model["height"], model["width"])
    out = depth.copy()
    for v in range(depth.shape[0]):
        yb = min(v // model["bin_height"], model["nby"] - 1)
        for u in range(depth.shape[1]):
            z = depth[v, u]
            if z == 0 or not (z > 0):
                continue
            out[v, u] = undistort_px(model["frustums"][yb * model["nbx"] + min(u // model["bin_width"], model["nbx"] - 1)], z)
    return out


# ---- the two millimetre conversions
def metres_convert_to(raw):
    """rgbd360_depth_undistort: (float)(0.001 * (double)raw), Frame360::undistort's and OpenCV's convertTo(.., 0.001)."""
    return (D(0.001) * np.asarray(raw, np.uint16).astype(D)).astype(F)


def metres_map_entries(raw):
    """rgbd360_rig_depth_clouds, _calibrate_rig_depth_models and _depth_evaluate_map: 0.001f * (float)raw, as every map entry scales."""
    return F(0.001) * np.asarray(raw, np.uint16).astype(F)


# ---- the rig calibration's cloud formation (k_rig_pinhole_cloud)
def pinhole_cloud(z, pin):
    """The points of a float32 metre image, float32 with every operation rounded on its own; NaN triples where z is not finite and positive."""
    fx, fy, cx, cy = (F(v) for v in pin)
    rows, cols = z.shape
    v, u = np.meshgrid(np.arange(rows, dtype=F), np.arange(cols, dtype=F), indexing="ij")
    f0, f1 = (u - cx) / fx, (v - cy) / fy
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(z) & (z > 0)
        pts = np.stack([z * f0, z * f1, z], axis=-1).astype(F)
    pts[~ok] = np.nan
    return np.ascontiguousarray(pts.reshape(-1, 3))


# ---- the evaluation's sums
def eval_terms(gt, meas, cor):
    """The five sums over examples (gt, meas, corrected z: float32 arrays), float64 without contraction."""
    gt, meas, cor = (np.asarray(a, F).astype(D).ravel() for a in (gt, meas, cor))
    e_raw, e_cor = meas - gt, cor - gt
    r = lambda x: int(np.rint(x).astype(np.int64).sum())
    return dict(n=len(gt), raw_e=r(e_raw * EVAL_FIX), raw_ee=r(e_raw * e_raw * EVAL_FIX), cor_e=r(e_cor * EVAL_FIX), cor_ee=r(e_cor * e_cor * EVAL_FIX))


def eval_map(cast, meas, model, require_plane=1, min_cos_incidence=0.0, min_mult=0.7, max_mult=1.3, max_range=10.0):
    """rgbd360_depth_evaluate_map on the cast of the image's rays (depth_train_reference.cast_pinhole): (sums, statistics).  The gates are
    the trainer's, on the raw measurement; model None: the corrected depth is the raw one."""
    meas32 = T.metres(meas)
    params = dict(require_plane=require_plane, min_cos_incidence=min_cos_incidence, min_mult=min_mult, max_mult=max_mult, max_range=max_range)
    gt_out, stats = T.Sums(meas32.shape[1], meas32.shape[0], meas32.shape[1], meas32.shape[0]).accumulate_map(cast, meas32, **params)
    gt, m = gt_out.astype(D), meas32.astype(D)
    with np.errstate(all="ignore"):
        mult = gt / m
        keep = (gt_out != 0) & ~((m > D(F(max_range))) | (gt > D(F(max_range)))) & ~((mult > D(F(max_mult))) | (mult < D(F(min_mult))))
    assert int(keep.sum()) == stats["n_examples"]
    cor = meas32 if model is None else undistort(model, np.where(keep, meas32, F(0)))
    return eval_terms(gt_out[keep], meas32[keep], cor[keep]), stats


def add_sums(a, b):
    return {k: a[k] + b[k] for k in EVAL_NAMES}


# ---- the models and images the tests share
SHAPES = ((64, 48, 8, 6), (66, 45, 6, 5), (8, 6, 8, 6))      # width, height, bin_width, bin_height: the trainer's own


def sums_for(shape, smoothing, seed, spread=0.1):
    """Training sums whose slices alternate below and at or above 50 examples (both branches of the correction run); with smoothing 0 a
    third of the slices is empty: D == 0 -> multiplier 1.  The multipliers lie within 1 -+ spread."""
    width, height, bw, bh = shape
    rng = np.random.default_rng(seed)
    sh = T.shape_of(width, height, bw, bh, 2.0)
    count = np.where((np.arange(sh[2])[None, None, :] + rng.integers(0, 2, size=sh[:2])[..., None]) % 2 == 0, rng.integers(50, 400, size=sh),
                     rng.integers(1, 49, size=sh)).astype(np.int64)
    count[rng.random(sh) < 0.15] = 49 - smoothing          # counts of exactly 49 and (elsewhere) 50 as the file holds them
    count[rng.random(sh) < 0.15] = 50 - smoothing
    num = (count * rng.uniform(0.3, 80.0, size=sh) * T.FIX).astype(np.int64)
    den = (num * rng.uniform(1.0 - spread, 1.0 + spread, size=sh)).astype(np.int64)
    if smoothing == 0:
        empty = rng.random(sh) < 0.33
        count[empty] = num[empty] = den[empty] = 0
    return count, num, den


def varied_model_bytes(shape, seed):
    """A written file whose frustums have different num_bins (1 .. 9) and bin_depth (0.5 .. 3)."""
    width, height, bw, bh = shape
    rng = np.random.default_rng(seed)
    nbx, nby = width // bw, height // bh
    frustums = []
    for k in range(nbx * nby):
        nb = 1 + (k * 5) % 9
        counts = np.where(rng.random(nb) < 0.5, 49.0, 50.0).astype(F) + rng.integers(-1, 2, size=nb).astype(F) * F(40)
        frustums.append((float(rng.choice([0.5, 0.75, 1.0, 2.0, 3.0])), counts, rng.uniform(0.8, 1.2, size=nb).astype(F)))
    return model_bytes(width, height, bw, bh, 2.0, nbx, nby, frustums)


def golden_model_bytes(k=1):
    return lzma.decompress(open(os.path.join(GOLDEN_MODELS, "distortion_model%d.xz" % k), "rb").read())


NAN_PAYLOAD = np.array([0x7FC12345], np.uint32).view(F)[0]


def depth_image(model, seed):
    """Random depths in (0, 12) m, then, from the first pixel on: per slice boundary of the pixel's own frustum the boundary, the
    half-slice point and their float32 neighbours on both sides; values below bin_depth / 2 and beyond the last slice; 0, -1, a NaN with
    a payload and +Inf."""
    rng = np.random.default_rng(seed)
    h, w = model["height"], model["width"]
    img = rng.uniform(0.01, 12.0, size=(h, w)).astype(F)
    flat = img.ravel()
    at = 0
    for stride in (1, 7):           # twice: the specials land in different frustums
        k = 0
        while at < flat.size:
            v, u = divmod(at, w)
            fbd, nb, _, _ = model["frustums"][min(v // model["bin_height"], model["nby"] - 1) * model["nbx"] + min(u // model["bin_width"], model["nbx"] - 1)]
            if k > nb + 1:
                break
            base = F(k * fbd) if (at // stride) % 2 == 0 else F((k + 0.5) * fbd)
            flat[at] = (base, np.nextafter(base, F(0)), np.nextafter(base, F(99)))[(at // (2 * stride)) % 3]
            if (at // (2 * stride)) % 3 == 2:
                k += 1
            at += stride
    tail = [F(1e-4), F(0.2), F(11.9), F(25.0), F(0), F(-1), NAN_PAYLOAD, F(np.inf), np.nextafter(F(0), F(1))]
    flat[flat.size - len(tail):] = tail
    flat[rng.integers(0, flat.size - len(tail), size=max(flat.size // 20, 1))] = 0
    return img


def raw_image(h, w, seed):
    """uint16 millimetres: random values, holes, and 0, 1, 5, 9, 65535 (5 and 9: the first values the two conversions disagree on)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(1, 12000, size=(h, w)).astype(np.uint16)
    img[rng.random((h, w)) < 0.1] = 0
    img.ravel()[:5] = (0, 1, 5, 9, 65535)
    return img
