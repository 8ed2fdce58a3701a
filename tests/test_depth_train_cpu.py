"""The host half of the depth-model trainer (rgbd360_depth_model_from_sums / _save, the loader that keeps every vector; csrc/depth_model.h)
and its numpy restatement (tests/depth_train_reference.py), without a GPU: the reference's own model files survive load -> save byte for
byte, the model of integer sums equals the restatement's file and corrects images like the oracle's numpy model, the restatement agrees
with a literal sequential loop of CLAMS' addExample, and what is refused.  (The refusals that need a trainer, and so a device, are in
tests/test_depth_train_gpu.py.)

Restatement against CLAMS' loop, 32 x 24 images with depths in 0.5 .. 9.5 m: the counts are equal; the multipliers of a float64 loop agree
within 2^-21 / gt_min^2 + 2^-21 / (gt_min meas_min) + 2^-23 relative -- every term of either integer sum is rounded by at most 2^-21 m^2
and is at least gt_min^2 resp. gt_min meas_min, so each sum is off by at most that fraction of itself; the float64 loop's own rounding
(n 2^-53) is far below; both multipliers are then rounded to float32 (2^-24 each).  With meas_min = 0.5 and gt_min = 0.7 meas_min (the
multiplier gate) that is 6.7e-6; measured 1.2e-7 (one float32 step).  A record, not a bound: the same loop with float32 running sums, as
CLAMS keeps them, differs from the exact multipliers by at most 9.4e-7 relative on these 768-pixel images (40 frames, about 260 examples
per bin; it grows with the number of examples as the sums outgrow 24 bits)."""
import ctypes as C
import lzma
import os

import numpy as np
import pytest

import depth_train_reference as T
from oracle import oracle as O
from rgbd360_amd import _lib
from rgbd360_amd.register import DepthModel, Rgbd360Error

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_models")
F = np.float32


def random_sums(rng, shape, empty=0.2):
    """Sums a trainer can hold: count examples per bin with terms gt^2, gt meas below 2^28 each; some bins empty."""
    count = rng.integers(0, 5000, size=shape).astype(np.int64)
    count[rng.random(shape) < empty] = 0
    num = (count * rng.uniform(0.3, 80.0, size=shape) * T.FIX).astype(np.int64)
    den = (num * rng.uniform(0.9, 1.1, size=shape)).astype(np.int64)
    return count, num, den


@pytest.mark.parametrize("k", [1, 5])
def test_reference_model_files_survive_load_and_save(tmp_path, k):
    raw = lzma.decompress(open(os.path.join(MODELS, "distortion_model%d.xz" % k), "rb").read())
    src, dst = tmp_path / "in", tmp_path / "out"
    src.write_bytes(raw)
    m = DepthModel(src, downsample=1)
    m.save(dst)
    assert dst.read_bytes() == raw
    # ... and load followed by downsample behaves as before: the loader's bins halve, the file's do not
    half = DepthModel(src, downsample=2)
    assert (half.width, half.bin_width, m.width, m.bin_width) == (m.width // 2, m.bin_width // 2, 640, 8)


@pytest.mark.parametrize("shape", [(64, 48, 8, 6, 2.0, 1), (8, 6, 8, 6, 2.0, 0), (64, 48, 8, 6, 1.5, 3)])
def test_model_from_sums_equals_the_restatement(tmp_path, shape):
    W, H, bw, bh, bd, smoothing = shape
    rng = np.random.default_rng(11)
    count, num, den = random_sums(rng, T.shape_of(W, H, bw, bh, bd))
    path = tmp_path / "model"
    m = DepthModel.from_sums(W, H, bw, bh, bd, smoothing, count, num, den)
    assert (m.width, m.height, m.bin_width, m.bin_height, m.num_bins_x, m.num_bins_y, m.bin_depth) == (W, H, bw, bh, W // bw, H // bh, bd)
    m.save(path)
    assert path.read_bytes() == T.model_bytes(W, H, bw, bh, bd, smoothing, count, num, den)
    # the file reads back, in the library and in the oracle's parser (which asserts that no byte is left over), and both correct alike
    back, ref = DepthModel(path, 1), O.depth_model_read(path, 1)
    counts, _, _, mult = T.finalise(count, num, den, smoothing)
    assert np.array_equal(np.stack(ref["multipliers"]).reshape(mult.shape), mult) and np.array_equal(np.stack(ref["counts"]).reshape(mult.shape), counts)
    depth = rng.uniform(0.2, 11.0, size=(H, W)).astype(F)
    depth[rng.random((H, W)) < 0.1] = 0.0
    want = O.depth_model_undistort(ref, depth)
    assert np.array_equal(m.undistort(depth), want) and np.array_equal(back.undistort(depth), want) and not np.array_equal(want, depth)


def test_empty_bins_without_smoothing_have_multiplier_one(tmp_path):
    shape = T.shape_of(8, 6, 8, 6, 2.0)
    zero = np.zeros(shape, np.int64)
    m = DepthModel.from_sums(8, 6, 8, 6, 2.0, 0, zero, zero, zero)
    m.save(tmp_path / "m")
    ref = O.depth_model_read(tmp_path / "m", 1)
    assert np.array_equal(ref["multipliers"][0], np.ones(5, F)) and not ref["counts"][0].any()
    depth = np.full((6, 8), 3.25, F)
    assert np.array_equal(m.undistort(depth), depth)
    # with smoothing 1 an empty bin is CLAMS' fresh frustum: counts, numerators, denominators and multipliers all one
    one = T.finalise(zero, zero, zero, 1)
    assert all(np.array_equal(v, np.ones(shape, F)) for v in one)


def clams_loop(frames, W, H, bw, bh, bd, smoothing, dtype):
    """DiscreteDepthDistortionModel::accumulate + DiscreteFrustum::addExample (discrete_depth_distortion_model.cpp:193-217, 21-36),
    example after example in pixel order, with running sums of `dtype`."""
    nby, nbx, nb = T.shape_of(W, H, bw, bh, bd)
    counts = np.full((nby, nbx, nb), smoothing, dtype)
    nums, dens = counts.copy(), counts.copy()
    mults = np.ones((nby, nbx, nb), dtype)
    for gt_img, meas_img in frames:
        for v in range(H):
            for u in range(W):
                if gt_img[v, u] == 0 or meas_img[v, u] == 0:
                    continue
                gt, meas = float(gt_img[v, u]), float(meas_img[v, u])
                mult = gt / meas
                if mult > float(F(1.3)) or mult < float(F(0.7)):
                    continue
                idx = min(nb - 1, int(np.floor(meas / bd)))
                f = (v // bh, u // bw, idx)
                nums[f] = dtype(float(nums[f]) + gt * gt)           # (a float32 coefficient += a double: one rounding)
                dens[f] = dtype(float(dens[f]) + gt * meas)
                counts[f] = dtype(counts[f] + dtype(1))
                mults[f] = dtype(nums[f] / dens[f])
    return counts, mults


def test_restatement_against_a_literal_clams_loop():
    W, H, bw, bh, bd, smoothing = 32, 24, 8, 6, 2.0, 1
    rng = np.random.default_rng(5)
    frames = []
    for _ in range(40):
        meas = rng.uniform(0.5, 9.5, size=(H, W)).astype(F)
        gt = (meas * rng.uniform(0.65, 1.35, size=(H, W))).astype(F)        # some beyond the multiplier gate
        meas[rng.random((H, W)) < 0.1] = 0
        gt[rng.random((H, W)) < 0.1] = 0
        frames.append((gt, meas))
    S = T.Sums(W, H, bw, bh, bd, smoothing)
    n = sum(S.accumulate_images(gt, meas, max_range=16.0)["n_examples"] for gt, meas in frames)      # (CLAMS has no range gate: gt reaches 12.8)
    counts, _, _, mult = T.finalise(S.count, S.num, S.den, smoothing)
    c64, m64 = clams_loop(frames, W, H, bw, bh, bd, smoothing, np.float64)
    assert n > 15000 and np.array_equal(counts.astype(np.float64), c64) and int(S.count.sum()) == n
    gt_min = 0.7 * 0.5
    bound = 2.0 ** -21 / gt_min ** 2 + 2.0 ** -21 / (gt_min * 0.5) + 2.0 ** -23
    err64 = np.abs(mult.astype(np.float64) / m64.astype(F).astype(np.float64) - 1).max()
    c32, m32 = clams_loop(frames, W, H, bw, bh, bd, smoothing, F)
    err32 = np.abs(m32.astype(np.float64) / mult.astype(np.float64) - 1).max()
    print("float64 loop: %.3g (bound %.3g); float32 running sums: %.3g" % (err64, bound, err32))
    assert err64 <= bound
    assert np.array_equal(c32.astype(np.float64), c64)      # (counts of a few hundred are exact in float32)


def test_refusals():
    L = _lib.load()
    shape = T.shape_of(64, 48, 8, 6, 2.0)
    z = np.zeros(shape, np.int64)
    for bad in (dict(width=65), dict(height=47), dict(bin_width=7), dict(smoothing=-1), dict(bin_depth=0.0), dict(bin_depth=-2.0), dict(width=0)):
        a = dict(width=64, height=48, bin_width=8, bin_height=6, bin_depth=2.0, smoothing=1)
        a.update(bad)
        h = C.c_void_p(1)
        rc = L.rgbd360_depth_model_from_sums(a["width"], a["height"], a["bin_width"], a["bin_height"], a["bin_depth"], a["smoothing"], z.ctypes.data,
                                             z.ctypes.data, z.ctypes.data, C.byref(h))
        assert rc == -1 and h.value is None, bad
    neg = z.copy()
    neg[0, 0, 0] = -1
    for trio in ((neg, z, z), (z, neg, z), (z, z, neg)):
        with pytest.raises(Rgbd360Error):
            DepthModel.from_sums(64, 48, 8, 6, 2.0, 1, *trio)
    with pytest.raises(Rgbd360Error):
        DepthModel.from_sums(64, 48, 8, 6, 2.0, 1, z[:-1], z[:-1], z[:-1])
    # NULL pointers: every entry answers -1 (or does nothing) without touching a device
    h = C.c_void_p()
    assert L.rgbd360_depth_model_from_sums(64, 48, 8, 6, 2.0, 1, None, z.ctypes.data, z.ctypes.data, C.byref(h)) == -1
    assert L.rgbd360_depth_model_from_sums(64, 48, 8, 6, 2.0, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, None) == -1
    assert L.rgbd360_depth_model_save(None, b"/nonexistent/x") == -1
    m = DepthModel.from_sums(64, 48, 8, 6, 2.0, 1, z, z, z)
    assert L.rgbd360_depth_model_save(m._h, None) == -1
    with pytest.raises(Rgbd360Error):
        m.save("/nonexistent-directory/model")
    assert L.rgbd360_depth_trainer_create(None, 64, 48, 8, 6, 2.0, 1, C.byref(h)) == -1 and h.value is None
    st = _lib.DepthTrainStats()
    assert L.rgbd360_depth_trainer_clear(None) == -1 and L.rgbd360_depth_trainer_model(None, C.byref(h)) == -1
    assert L.rgbd360_depth_trainer_sums(None, None, None, None) == -1 and L.rgbd360_depth_trainer_add_sums(None, None, None, None) == -1
    assert L.rgbd360_depth_trainer_accumulate_images(None, None, 0, None, 0, 1, 0, 0, 0, None, C.byref(st)) == -1
    assert L.rgbd360_depth_trainer_accumulate_map(None, None, None, 0, 1, 0, 0, 1.0, 1.0, 0.0, 0.0, None, 0, None, None, C.byref(st)) == -1
    L.rgbd360_depth_trainer_destroy(None)
    assert L.rgbd360_depth_trainer_last_error(None) == b"null trainer"
    L.rgbd360_depth_default_train_params(None, None)
    p = _lib.DepthTrainParams()
    L.rgbd360_depth_default_train_params(None, C.byref(p))
    assert (p.require_plane, p.min_cos_incidence, p.min_mult, p.max_mult, p.max_range) == (1, 0.0, F(0.7), F(1.3), 10.0)
    assert (p.ray.min_count, p.ray.max_steps, p.normal.min_support, p.normal.max_shift) == (1, 8192, 5, 2.0)


def test_calibrate_depth_example_compiles_and_checks_its_inputs(tmp_path):
    """examples/calibrate_depth.cpp (include/rgbd360/DepthTrainer.hpp: DepthTrainer with DiscreteDepthDistortionModel's constructor,
    DepthTrainerRig over a Frame360's eight sensors) compiles warning-free against the C ABI; missing inputs are reported."""
    import subprocess
    from rgbd360_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = build.build()
    exe = str(tmp_path / "calibrate_depth")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "calibrate_depth.cpp"), "-L" + os.path.dirname(lib), "-lrgbd360_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    assert subprocess.call([exe], stderr=subprocess.DEVNULL) == 2
    args = [exe, str(tmp_path), "1", str(tmp_path / "poses.txt"), str(tmp_path), str(tmp_path)]
    assert subprocess.call(args, stderr=subprocess.DEVNULL) == 3                                # no poses
    np.savetxt(tmp_path / "poses.txt", np.eye(4))
    assert subprocess.call(args, stderr=subprocess.DEVNULL) == 3                                # no Rt_0N.txt
    assert subprocess.call(args + ["--bogus", "1"], stderr=subprocess.DEVNULL) == 2


def test_restatement_gate_cases_with_representable_limits():
    """min_mult 0.75 and max_mult 1.25 are float32 values: gt 3 against meas 4 and gt 5 against meas 4 sit on the limits and are kept
    (CLAMS rejects `mult > MAX_MULT || mult < MIN_MULT`); one float32 step outside is rejected.  The clamp of step 4: a measurement beyond
    the last slice lands in it."""
    gt = np.array([[3.0, 5.0, np.nextafter(F(3.0), F(0)), np.nextafter(F(5.0), F(9)), 10.9, 0.0, 1.0, 1.0]], F)
    meas = np.array([[4.0, 4.0, 4.0, 4.0, 11.6, 1.0, 0.0, np.nan]], F)
    S = T.Sums(8, 1, 1, 1, 2.0, 0)
    st = S.accumulate_images(gt, meas, min_mult=0.75, max_mult=1.25, max_range=12.0)
    assert st == dict(n_pixels=8, n_no_measurement=2, n_no_hit=1, n_off_plane=0, n_grazing=0, n_out_of_range=0, n_mult_rejected=2, n_examples=3)
    assert S.count[0, :, :].tolist() == [[0, 0, 1, 0, 0], [0, 0, 1, 0, 0]] + [[0] * 5] * 2 + [[0, 0, 0, 0, 1]] + [[0] * 5] * 3
    assert S.num[0, 0, 2] == 9 << 20 and S.den[0, 0, 2] == 12 << 20 and S.num[0, 1, 2] == 25 << 20 and S.den[0, 1, 2] == 20 << 20
