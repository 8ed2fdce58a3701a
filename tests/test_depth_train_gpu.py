"""The depth-model trainer on the device (rgbd360_depth_trainer_*, csrc/depth_train.h) against the numpy restatement
(tests/depth_train_reference.py), bit for bit: the image route on ragged shapes in every input form and every accumulation form, the map
route on a three-wall corner next to rgbd360_map_raycast_surface on the same rays, order / split / run independence, the recovery of a
known distortion, the loop end to end (train from the map, save, load, undistort held-out images), empty inputs and refusals.

Shapes: sensors of 64 x 48 pixels (bins 8 x 6: 64 frustums of five 2 m slices), 66 x 45 (bins 6 x 5: 2970 pixels, ragged against the
8 x 8 tile of a wave and the 16 x 16 tile of a workgroup) and 8 x 6 (one frustum: every lane on at most five words).  The map: three walls
of 3 m at leaf 0.1, about 2700 voxels, inserted as one cloud.

Recovery bound (set by the definition): a multiplier m constant per (frustum, slice) comes back within 2^-21 / (z_min^2 0.9) + 2^-23
relative, z_min = 0.5 the closest surface: the fixed-point rounding of a sum of llrint terms of at least z_min z_min / 1.1 2^20, and the
float32 roundings of meas and of the multiplier.  Measured: 2.4e-7 over 431 slices against the bound's 2.2e-6.
End to end: gt / meas = 1 + 0.012 z (0.5 + 4 r^2), r the pixel's distance from the image centre over the half diagonal; 40 training poses,
10 held-out ones.  The restatement (whose model file the device's equals byte for byte) brings the RMS depth error of the held-out images
from 0.0884 m down to 0.0147 m, a ratio of 6.03 (fed analytic ground truth through the image route: 6.02 -- what is left is the model's
resolution, 8 x 6-pixel bins and 2 m slices, not the map); the bound asserted is half the restatement's ratio: 3.0."""
import ctypes as C

import numpy as np
import pytest

import depth_train_reference as T
import map_align_plane_reference as P
import voxel_map_reference as R
from map_input_forms import hip_runtime

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
LEAF = 0.1
EYE = np.eye(4, dtype=F)
W, H = 64, 48
PINHOLE = dict(fx=60.0, fy=60.0, cx=31.5, cy=23.5)
RATIO_RESTATEMENT = 6.0      # measured on the restatement (the docstring); the bound is half of it


def look_at(eye, target):
    """world <- sensor for a sensor at `eye` whose z axis points at `target` (x right, y down), float32."""
    eye, target = np.asarray(eye, D), np.asarray(target, D)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T4 = np.eye(4)
    T4[:3, 0], T4[:3, 1], T4[:3, 2], T4[:3, 3] = x, y, z, eye
    return T4.astype(F)


POSES = dict(corner=look_at((1.2, 1.0, 0.9), (0.0, 0.0, 0.0)),           # facing the corner
             outward=look_at((1.2, 1.0, 0.9), (2.4, 2.0, 1.8)),          # looking out of the map: every ray misses
             grazing_floor=look_at((1.0, 1.2, 0.08), (0.5, 0.6, 0.0)))   # less than a leaf above the floor: hits below t_min are passed through


def analytic_depth(pose, size=3.0):
    """The true z of every pixel's ray against the three walls x = 0, y = 0, z = 0 (each size x size from the corner); 0: none."""
    o, d = T.pinhole_rays(H, W, pose=pose, **PINHOLE)
    o, d = o.astype(D), d.astype(D)
    best = np.full(len(o), np.inf)
    for k in range(3):
        with np.errstate(all="ignore"):
            t = -o[:, k] / d[:, k]
        p = o + t[:, None] * d
        ok = (d[:, k] < 0) & (t > 0) & (p >= -1e-9).all(axis=1) & (p <= size).all(axis=1)
        best = np.where(ok & (t < best), t, best)
    return np.where(np.isfinite(best), best, 0.0).reshape(H, W)


def radius2():
    v, u = np.mgrid[0:H, 0:W]
    return (((u - PINHOLE["cx"]) ** 2 + (v - PINHOLE["cy"]) ** 2) / (PINHOLE["cx"] ** 2 + PINHOLE["cy"] ** 2)).astype(D)


def distort(z):
    """The measurement of a true depth image under gt / meas = 1 + 0.012 z (0.5 + 4 r^2); float32, 0 stays 0."""
    return (z / (1.0 + 0.012 * z * (0.5 + 4.0 * radius2()))).astype(F)


def random_poses(seed, n):
    rng = np.random.default_rng(seed)
    return [look_at(rng.uniform(0.8, 2.2, 3), rng.uniform(0.0, 0.8, 3)) for _ in range(n)]


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scene():
    """The corner cloud, the restatement's map of it and the restatement's cast of the three poses; computed once, never changed."""
    cloud = P.corner_scene(3, size=3.0, step=0.02)
    ref = R.Map([(cloud, None, EYE)], LEAF, None)
    assert 2000 < len(ref) < 4000
    casts = {name: T.cast_pinhole(ref, LEAF, H, W, pose=pose, **PINHOLE) for name, pose in POSES.items()}
    rng = np.random.default_rng(21)
    meas = {}
    for name, c in casts.items():       # measurements around the cast depth, some beyond the multiplier gate, some holes; a miss gets a plain depth
        m = (np.where(c["hit"], c["t"], F(1.5)) * rng.uniform(0.65, 1.35, size=(H, W))).astype(F)
        m[rng.random((H, W)) < 0.1] = 0
        m[0, :4] = (np.nan, np.inf, -1.0, 11.0)
        meas[name] = m
    return dict(cloud=cloud, ref=ref, casts=casts, meas=meas)


@pytest.fixture()
def gmap(reg, scene):
    from rgbd360_amd.voxel_map import VoxelMap
    with VoxelMap(reg, LEAF, 1 << 13) as m:
        m.set_box(None, None)
        m.insert_cloud(scene["cloud"], None, EYE)
        assert not m.full and len(m) == len(scene["ref"])
        yield m


def trainer(reg, *shape, **kw):
    from rgbd360_amd.depth_train import DepthTrainer
    return DepthTrainer(reg, *shape, **kw)


def assert_sums_equal(t, S, what=""):
    for name, got, want in zip(("count", "num", "den"), t.sums(), (S.count, S.num, S.den)):
        assert np.array_equal(got, want), (what, name, int((got != want).sum()))


# ---- the image route
def image_case(width, height, u16):
    """gt and meas with every special value, the clamp of step 4 (max_range 12), measurements beyond max_range and the gate cases."""
    rng = np.random.default_rng(width * 100 + height)
    gt = rng.uniform(0.4, 11.5, size=(height, width)).astype(F)
    meas = (gt * rng.uniform(0.7, 1.3, size=(height, width))).astype(F)
    g, m = gt.ravel(), meas.ravel()          # (views: the images are written through them)
    n = g.size
    g[5 % n], m[7 % n] = 0.0, 0.0
    g[11 % n], m[11 % n] = 3.0, 4.0          # mult 0.75 == min_mult: kept
    g[12 % n], m[12 % n] = 5.0, 4.0          # mult 1.25 == max_mult: kept
    g[13 % n], m[13 % n] = np.nextafter(F(3.0), F(0)), 4.0       # one float32 step outside: rejected
    g[14 % n], m[14 % n] = np.nextafter(F(5.0), F(9)), 4.0
    g[15 % n], m[15 % n] = 10.9, 11.6        # beyond the last slice, inside max_range 12: the clamp of step 4
    g[16 % n], m[16 % n] = 11.0, 12.5        # beyond max_range
    g[17 % n], m[17 % n] = 12.5, 11.0
    if u16:
        return np.round(gt * 1000).astype(np.uint16), np.round(meas * 1000).astype(np.uint16)
    for k, bad in enumerate((np.nan, np.inf, -np.inf, -2.0)):
        g[(20 + k) % n] = bad
        m[(30 + k) % n] = bad
    g[40 % n], m[40 % n] = np.nan, np.nan
    return gt, meas


def padded(a, pad=3):
    buf = np.full((a.shape[0], a.shape[1] + pad), 77, a.dtype)
    buf[:, :a.shape[1]] = a
    return buf[:, :a.shape[1]]


IMAGE_PARAMS = dict(min_mult=0.75, max_mult=1.25, max_range=12.0)


@pytest.mark.parametrize("shape", [(64, 48, 8, 6), (66, 45, 6, 5), (8, 6, 8, 6)])
def test_image_route_equals_the_restatement(reg, shape):
    from rgbd360_amd import _lib
    width, height, bw, bh = shape
    hip = hip_runtime()
    for u16 in (False, True):
        gt, meas = image_case(width, height, u16)
        S = T.Sums(width, height, bw, bh, 2.0, 1)
        want = S.accumulate_images(gt, meas, **IMAGE_PARAMS)
        print(shape, "u16" if u16 else "f32", want)
        assert want["n_examples"] > 0.5 * gt.size and want["n_mult_rejected"] >= 2 and want["n_out_of_range"] >= 2 and want["n_no_hit"] >= 1
        assert S.count[..., 4].sum() > 0 and sum(want.values()) == 2 * want["n_pixels"]
        if not u16:
            assert want["n_no_hit"] >= 5 and want["n_no_measurement"] >= 4
        with trainer(reg, width, height, bw, bh, 2.0, 1) as t:
            for form in (2, 1, 0):                  # the three ways the kernel adds: one result
                t.set_form(form)
                t.clear()
                assert t.accumulate(gt, meas, **IMAGE_PARAMS) == want, form
                assert_sums_equal(t, S, "form %d" % form)
            t.set_form(2)
            # a padded row step, host memory
            t.clear()
            assert t.accumulate(padded(gt), padded(meas, 5), **IMAGE_PARAMS) == want
            assert_sums_equal(t, S, "padded")
            # device memory, padded
            t.clear()
            dev = []
            for a in (padded(gt), padded(meas, 5)):
                whole = np.ascontiguousarray(a.base)
                p = C.c_void_p()
                assert hip.hipMalloc(C.byref(p), whole.nbytes) == 0
                assert hip.hipMemcpy(p, whole.ctypes.data_as(C.c_void_p), whole.nbytes, 1) == 0
                dev.append((p, whole.strides[0]))
            st = _lib.DepthTrainStats()
            params = t.params(**IMAGE_PARAMS)
            rc = t._L.rgbd360_depth_trainer_accumulate_images(t._handle(), dev[0][0], dev[0][1], dev[1][0], dev[1][1], 0 if u16 else 1, height, width, 1,
                                                              C.byref(params), C.byref(st))
            for p, _ in dev:
                hip.hipFree(p)
            assert rc == 0 and {k: getattr(st, k) for k in T.STAT_NAMES} == want
            assert_sums_equal(t, S, "device")


# ---- the map route
@pytest.mark.parametrize("require_plane", [1, 0])
@pytest.mark.parametrize("min_cos", [0.0, 0.5])
def test_map_route_equals_the_restatement_and_the_surface_cast(reg, scene, gmap, require_plane, min_cos):
    params = dict(require_plane=require_plane, min_cos_incidence=min_cos)
    S = T.Sums(W, H, 8, 6, 2.0, 1)
    with trainer(reg, W, H, 8, 6, 2.0, 1) as t:
        for name, pose in POSES.items():
            cast, meas = scene["casts"][name], scene["meas"][name]
            want_gt, want = S.accumulate_map(cast, meas, **params)
            gt, got = t.accumulate_map(gmap, meas, PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"], PINHOLE["cy"], pose, **params)
            print(name, params, got)
            assert got == want and sum(got.values()) == 2 * got["n_pixels"], name
            assert gt.tobytes() == want_gt.tobytes(), name
            # ... and gt is the device's own surface cast of the rays formed in numpy by the definition, wherever the gates pass
            dev_t = gmap.raycast_surface(cast["origins"], cast["dirs"])[0].reshape(H, W)
            reached = gt != 0
            assert np.array_equal(gt[reached], dev_t[reached]) and reached.sum() == got["n_out_of_range"] + got["n_mult_rejected"] + got["n_examples"]
            if name == "outward":
                assert got["n_no_hit"] == got["n_pixels"] - got["n_no_measurement"] and got["n_examples"] == 0
            else:
                assert got["n_examples"] > 200 and got["n_mult_rejected"] > 50
        assert_sums_equal(t, S, str(params))
    # not vacuous: each gate acts somewhere in the three poses
    tot = {k: 0 for k in T.STAT_NAMES}
    S2 = T.Sums(W, H, 8, 6, 2.0, 1)
    for name in POSES:
        for k, v in S2.accumulate_map(scene["casts"][name], scene["meas"][name], **params)[1].items():
            tot[k] += v
    assert (tot["n_off_plane"] > 0) == bool(require_plane) and (tot["n_grazing"] > 0) == (min_cos > 0) and tot["n_out_of_range"] > 0


def frames_of(scene):
    return [(name, POSES[name], scene["meas"][name]) for name in ("corner", "grazing_floor", "outward")]


def run_map(t, gmap, frames):
    for _, pose, meas in frames:
        t.accumulate_map(gmap, meas, PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"], PINHOLE["cy"], pose, want_gt=False)


def test_order_split_and_run_change_no_bit(reg, scene, gmap):
    frames = frames_of(scene)
    with trainer(reg, W, H, 8, 6, 2.0, 1) as a, trainer(reg, W, H, 8, 6, 2.0, 1) as b, trainer(reg, W, H, 8, 6, 2.0, 1) as c:
        run_map(a, gmap, frames)
        first = a.sums()
        assert first[0].sum() > 1000
        run_map(b, gmap, frames[::-1])                      # another order
        assert all(np.array_equal(x, y) for x, y in zip(first, b.sums()))
        b.clear()                                           # clear zeroes the state ...
        assert not any(x.any() for x in b.sums())
        run_map(b, gmap, frames)                            # ... and a second run gives the same bits
        assert all(np.array_equal(x, y) for x, y in zip(first, b.sums()))
        b.clear()
        run_map(b, gmap, frames[:1])                        # the frames split over two trainers, joined by add_sums
        run_map(c, gmap, frames[1:])
        b.add_sums(*c.sums())
        assert all(np.array_equal(x, y) for x, y in zip(first, b.sums()))
        assert a.model().undistort(np.full((H, W), 1.7, F)).tobytes() == b.model().undistort(np.full((H, W), 1.7, F)).tobytes()


def test_a_known_distortion_is_recovered(reg, scene, gmap):
    rng = np.random.default_rng(8)
    bd, nb = 2.0, 5
    m_true = rng.uniform(0.9, 1.1, size=(H // 6, W // 8, nb))
    v, u = np.mgrid[0:H, 0:W]
    z_min = 0.5
    bound = 2.0 ** -21 / (z_min ** 2 * 0.9) + 2.0 ** -23
    wide = dict(min_mult=0.0, max_mult=100.0)
    with trainer(reg, W, H, 8, 6, bd, 0) as t:
        worst, slices = 0.0, 0
        for pose in (POSES["corner"],) + tuple(random_poses(3, 5)):
            gt, _ = t.accumulate_map(gmap, np.ones((H, W), F), PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"], PINHOLE["cy"], pose, **wide)     # first pass: gt_out
            t.clear()
            assert gt[gt > 0].min() >= z_min
            s = np.minimum(nb - 1, np.floor(gt.astype(D) / bd).astype(int))
            m = m_true[v // 6, u // 8, s]
            meas = (gt.astype(D) / m).astype(F)
            meas[np.minimum(nb - 1, np.floor(meas.astype(D) / bd).astype(int)) != s] = 0       # meas left the slice of its m
            meas[gt == 0] = 0
            t.accumulate_map(gmap, meas, PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"], PINHOLE["cy"], pose, want_gt=False)
            count, num, den = t.sums()
            got = T.finalise(count, num, den, 0)[3].astype(D)
            seen = count > 0
            err = np.abs(got[seen] / m_true[seen] - 1)
            worst, slices = max(worst, float(err.max())), slices + int(seen.sum())
            assert (err <= bound).all(), (float(err.max()), bound)
            t.clear()
        print("recovery: worst relative error %.3g over %d slices (bound %.3g)" % (worst, slices, bound))
        assert slices > 300


def end_to_end_inputs():
    train = [(p, analytic_depth(p)) for p in random_poses(40, 40)]
    held = [(p, analytic_depth(p)) for p in random_poses(41, 10)]
    return train, held


def rms_ratio(model_undistort, held):
    before = after = n = 0.0
    for _, z in held:
        meas = distort(z)
        fixed = model_undistort(meas)
        ok = z > 0
        before += float(((meas.astype(D) - z)[ok] ** 2).sum())
        after += float(((fixed.astype(D) - z)[ok] ** 2).sum())
        n += int(ok.sum())
    return np.sqrt(before / n), np.sqrt(after / n)


def test_the_loop_end_to_end(reg, scene, gmap, tmp_path):
    from rgbd360_amd.register import DepthModel
    train, held = end_to_end_inputs()
    S = T.Sums(W, H, 8, 6, 2.0, 1)
    with trainer(reg, W, H, 8, 6, 2.0, 1) as t:
        for pose, z in train:
            meas = distort(z)
            _, got = t.accumulate_map(gmap, meas, PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"], PINHOLE["cy"], pose, want_gt=False)
            _, want = S.accumulate_map(T.cast_pinhole(scene["ref"], LEAF, H, W, pose=pose, **PINHOLE), meas)
            assert got == want
        path = tmp_path / "distortion_model1"
        t.save(path)
    assert path.read_bytes() == S.model_bytes()                 # the device's model file is the restatement's, byte for byte
    model = DepthModel(path, 1)
    before, after = rms_ratio(model.undistort, held)
    print("held-out RMS depth error: %.4f m before, %.4f m after, ratio %.2f" % (before, after, before / after))
    assert after < before
    assert before / after >= 0.5 * RATIO_RESTATEMENT


# ---- empty inputs and refusals
def test_empty_inputs(reg, scene):
    from rgbd360_amd import _lib
    from rgbd360_amd.voxel_map import VoxelMap
    zero = {k: 0 for k in T.STAT_NAMES}
    with trainer(reg, W, H, 8, 6, 2.0, 1) as t, VoxelMap(reg, LEAF, 1 << 10) as empty:
        gt, got = t.accumulate_map(empty, scene["meas"]["corner"], PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"], PINHOLE["cy"], POSES["corner"])
        assert got == zero and not gt.any()
        st = _lib.DepthTrainStats(n_pixels=5)
        img = np.zeros((H, W), F)
        pose = np.ascontiguousarray(POSES["corner"].T.reshape(16))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        for rows, cols in ((0, W), (H, 0), (0, 0)):
            assert t._L.rgbd360_depth_trainer_accumulate_images(t._handle(), vp(img), W * 4, vp(img), W * 4, 1, rows, cols, 0, None, C.byref(st)) == 0
            assert {k: getattr(st, k) for k in T.STAT_NAMES} == zero
            st.n_pixels = 5
            assert t._L.rgbd360_depth_trainer_accumulate_map(t._handle(), empty._handle(), vp(img), W * 4, 1, rows, cols, 60.0, 60.0, 31.5, 23.5, vp(pose), 0,
                                                             None, None, C.byref(st)) == 0
            assert {k: getattr(st, k) for k in T.STAT_NAMES} == zero
            st.n_pixels = 5
        assert not any(x.any() for x in t.sums())


def test_refusals(reg, scene, gmap):
    from rgbd360_amd.depth_train import DepthTrainer
    from rgbd360_amd.register import Rgbd360Error
    for bad in ((65, 48, 8, 6), (64, 47, 8, 6), (64, 48, 8, 6, 2.0, -1), (64, 48, 8, 6, 0.0), (64, 48, 0, 6)):
        with pytest.raises(Rgbd360Error):
            DepthTrainer(reg, *bad)
    gt, meas = image_case(W, H, False)
    pin = (PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"], PINHOLE["cy"])
    with trainer(reg, W, H, 8, 6, 2.0, 1) as t:
        for params in (dict(max_range=0.0), dict(max_range=16.5), dict(max_range=np.nan), dict(min_mult=1.2, max_mult=1.1), dict(min_mult=-0.1),
                       dict(max_mult=np.nan)):
            with pytest.raises(Rgbd360Error):
                t.accumulate(gt, meas, **params)
            with pytest.raises(Rgbd360Error):
                t.accumulate_map(gmap, meas, *pin, POSES["corner"], **params)
        with pytest.raises(Rgbd360Error):
            t.accumulate(gt[:-1], meas[:-1])                    # not the trainer's size
        with pytest.raises(Rgbd360Error):
            t.accumulate_map(gmap, meas[:, :-1], *pin, POSES["corner"])
        for params in (dict(min_cos_incidence=1.5), dict(min_cos_incidence=-0.1), dict(max_steps=0), dict(min_support=0), dict(t_min=-1.0)):
            with pytest.raises(Rgbd360Error):
                t.accumulate_map(gmap, meas, *pin, POSES["corner"], **params)
        with pytest.raises(Rgbd360Error):
            t.accumulate_map(gmap, meas, 0.0, 60.0, 31.5, 23.5, POSES["corner"])
        bad_pose = POSES["corner"].copy()
        bad_pose[0, 3] = np.nan
        with pytest.raises(Rgbd360Error):
            t.accumulate_map(gmap, meas, *pin, bad_pose)
        st = t._L.rgbd360_depth_trainer_accumulate_images(t._handle(), None, W * 4, None, W * 4, 1, H, W, 0, None, None)
        assert st == -1 and b"null" in t._L.rgbd360_depth_trainer_last_error(t._handle())
        z = np.zeros(t.shape, np.int64)
        neg = z.copy()
        neg[0, 0, 0] = -1
        for trio in ((neg, z, z), (z, neg, z), (z, z, neg)):
            with pytest.raises(Rgbd360Error):
                t.add_sums(*trio)
        one = z.copy()
        one[0, 0, 0] = 1
        with pytest.raises(Rgbd360Error):
            t.add_sums(one, one * (1 << 29), one)               # a term no trainer can hold
        with pytest.raises(Rgbd360Error):
            t.add_sums(one * (1 << 34), z, z)                   # a full trainer
        assert not any(x.any() for x in t.sums())               # nothing was added by a refused call
