"""Applying the depth models on the device (rgbd360_depth_models_*, rgbd360_depth_undistort, rgbd360_rig_depth_clouds,
rgbd360_map_calibrate_rig_depth_models, rgbd360_depth_evaluate_map; csrc/depth_apply.h) against the host call and the numpy restatement
(tests/depth_apply_reference.py), byte for byte and bit for bit.

Shapes: the trainer's own sensors, 64 x 48 with bins 8 x 6, 66 x 45 with bins 6 x 5 (ragged against the 8 x 8 tile of a wave and the
16 x 16 tile of a workgroup) and 8 x 6 (one frustum); the reference's distortion_model1 at 320 x 240 once.  A set of four sensors: a model
of sums with smoothing 1, none (identity), a model with smoothing 0 and empty slices, and a written file whose frustums differ in
num_bins and bin_depth.  The evaluation runs in the three-wall corner of tests/test_depth_train_gpu.py, the calibration in the closed cube
of tests/test_rig_calib_gpu.py at its smallest size.

The loop end to end (train from the map, models to the device, held-out images judged on the device): the bound is that file's own,
sqrt(raw_ee / cor_ee) >= 3.0, half of the ratio 6.0 measured on the restatement; the device's sums equal the restatement's, so its ratio
is the restatement's."""
import ctypes as C

import numpy as np
import pytest

import depth_apply_reference as A
import depth_train_reference as T
import map_input_forms as MF
import rig_calib_reference as RC
import test_depth_train_gpu as TG
import test_rig_calib_gpu as RG
from test_depth_apply_cpu import from_sums, loaded
from test_depth_train_gpu import gmap, scene      # noqa: F401  (fixtures: the corner map and its restatement's casts)

pytestmark = pytest.mark.gpu

F = np.float32
W, H, PINHOLE, POSES = TG.W, TG.H, TG.PINHOLE, TG.POSES
PIN = (PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"], PINHOLE["cy"])
SENTINEL = 0xEE


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip():
    return MF.hip_runtime()


class Device:
    """Device copies of host arrays, freed on exit."""

    def __init__(self, hip):
        self.hip, self.ptrs = hip, []

    def __enter__(self):
        return self

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 4)) == 0 and self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        self.ptrs.append(p)
        return p.value

    def get(self, ptr, like):
        out = np.zeros_like(np.ascontiguousarray(like))
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0
        return out

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.hip.hipFree(p)


def rig_of(tmp_path, shape):
    """[(DepthModel or None, restatement model or None)] of the four sensors."""
    return [from_sums(tmp_path, shape, 1, 31), (None, None), from_sums(tmp_path, shape, 0, 32),
            loaded(tmp_path, "varied_%d" % shape[0], A.varied_model_bytes(shape, 33))]


def models_of(reg, rig):
    from rgbd360_amd.depth_train import DepthModels
    return DepthModels(reg, [m for m, _ in rig])


def host_undistort(rig, sensor, metres):
    return metres.copy() if rig[sensor][0] is None else rig[sensor][0].undistort(metres)


def undistort_call(L, reg, models, frames, sensors, depth_type, rows, cols, on_device, outs, out_step):
    I = (_frames_type() * max(len(frames), 1))()
    for k, (addr, step) in enumerate(frames):
        I[k].depth, I[k].depth_step = addr, step
    sen = None if sensors is None else (C.c_int * max(len(sensors), 1))(*sensors)
    out = None if outs is None else (C.c_void_p * max(len(outs), 1))(*outs)
    return L.rgbd360_depth_undistort(reg._ctx(), None if models is None else models._handle(), I, sen, len(frames), depth_type, rows, cols, on_device, out, out_step)


def _frames_type():
    from rgbd360_amd import _lib
    return _lib.MapBatchFrame


def padded(a, pad):
    """`a` as a view of a buffer whose rows carry `pad` sentinel bytes behind them: (view, whole buffer as bytes)."""
    rows = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
    buf = np.full((rows.shape[0], rows.shape[1] + pad), SENTINEL, np.uint8)
    buf[:, :rows.shape[1]] = rows
    return buf


def unpadded(buf, like):
    n = like.shape[1] * like.itemsize
    assert (buf[:, n:] == SENTINEL).all()              # beyond cols nothing was written
    return np.ascontiguousarray(buf[:, :n]).view(like.dtype).reshape(like.shape)


# ---- 1: the stand-alone undistort
@pytest.mark.parametrize("depth_type", (0, 1))
@pytest.mark.parametrize("shape", A.SHAPES)
def test_undistort_equals_the_host_call_byte_for_byte(hip_lib, hip, reg, tmp_path, shape, depth_type):
    L = hip_lib
    width, height = shape[:2]
    rig = rig_of(tmp_path, shape)
    sensors = [3, 0, 2, 1, 0]
    if depth_type == 0:
        images = [A.raw_image(height, width, 50 + i) for i in range(5)]
        metres = [A.metres_convert_to(img) for img in images]
        assert any((m != A.metres_map_entries(img)).any() for m, img in zip(metres, images))
    else:
        images = [A.depth_image(rig[s][1] or rig[0][1], 60 + i) for i, s in enumerate(sensors)]
        metres = images
    want = [host_undistort(rig, s, m) for s, m in zip(sensors, metres)]
    assert all(w.tobytes() != m.tobytes() for w, m, s in zip(want, metres, sensors) if s != 1)
    with models_of(reg, rig) as models, Device(hip) as dev:
        assert models.nbytes > 600
        # host memory, five images in one launch under a permutation of the sensors (the Python mirror)
        got = models.undistort(images, sensors)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        # one image; padded row steps on both sides, host memory
        for k in (0, 3):
            src, dst = padded(images[k], 8), padded(np.zeros((height, width), F), 12)
            assert undistort_call(L, reg, models, [(src.ctypes.data, src.shape[1])], [sensors[k]], depth_type, height, width, 0, [dst.ctypes.data], dst.shape[1]) == 0
            assert unpadded(dst, want[k]).tobytes() == want[k].tobytes()
        # device memory, padded, five images
        srcs = [padded(img, 8) for img in images]
        dsts = [padded(np.zeros((height, width), F), 12) for _ in images]
        d_src, d_dst = [dev.put(s) for s in srcs], [dev.put(d) for d in dsts]
        assert undistort_call(L, reg, models, [(p, s.shape[1]) for p, s in zip(d_src, srcs)], sensors, depth_type, height, width, 1, d_dst, dsts[0].shape[1]) == 0
        for p, d, w in zip(d_dst, dsts, want):
            assert unpadded(dev.get(p, d), w).tobytes() == w.tobytes()
        if depth_type == 1:
            # in place: host memory (padded) and device memory
            bufs = [padded(img, 8) for img in images]
            assert undistort_call(L, reg, models, [(b.ctypes.data, b.shape[1]) for b in bufs], sensors, 1, height, width, 0, [b.ctypes.data for b in bufs],
                                  bufs[0].shape[1]) == 0
            assert all(unpadded(b, w).tobytes() == w.tobytes() for b, w in zip(bufs, want))
            d_io = [dev.put(img) for img in images]
            assert undistort_call(L, reg, models, [(p, width * 4) for p in d_io], sensors, 1, height, width, 1, d_io, width * 4) == 0
            assert all(dev.get(p, w).tobytes() == w.tobytes() for p, w in zip(d_io, want))


def test_undistort_with_the_reference_model(reg, tmp_path):
    model, ref = loaded(tmp_path, "golden1", A.golden_model_bytes(1), 2)
    assert (ref["width"], ref["height"]) == (320, 240)
    depth = A.depth_image(ref, 71)
    raw = A.raw_image(240, 320, 72)
    raw.ravel()[8:8 + 65535] = np.arange(1, 65536, dtype=np.uint16)          # a block of all 65535 non-zero raw values
    from rgbd360_amd.depth_train import DepthModels
    with DepthModels(reg, [model]) as models:
        assert models.undistort([depth], [0])[0].tobytes() == model.undistort(depth).tobytes()
        assert models.undistort([raw], [0])[0].tobytes() == model.undistort(A.metres_convert_to(raw)).tobytes()


# ---- 2: no model
def clouds_call(L, reg, models, images, n_frames, n_sensors, pin, dev, on_device=0):
    """rgbd360_rig_depth_clouds: (rc, the clouds [n images, rows cols, 3] copied back)."""
    rows, cols = images[0].shape
    I = (_frames_type() * len(images))()
    for k, img in enumerate(images):
        I[k].depth, I[k].depth_step = (dev.put(img) if on_device else img.ctypes.data), img.strides[0]
    out = np.full((len(images), rows * cols, 3), 7.0, F)
    p = dev.put(out)
    rc = L.rgbd360_rig_depth_clouds(reg._ctx(), None if models is None else models._handle(), I, n_frames, n_sensors, 0 if images[0].dtype == np.uint16 else 1, rows,
                                    cols, *[C.c_float(v) for v in pin], on_device, C.c_void_p(p))
    return rc, dev.get(p, out)


def test_without_a_model_the_output_is_the_converted_input(hip_lib, hip, reg, tmp_path):
    from rgbd360_amd.depth_train import DepthModels
    L = hip_lib
    shape = A.SHAPES[1]
    width, height = shape[:2]
    rig = rig_of(tmp_path, shape)
    raw, depth = A.raw_image(height, width, 80), A.depth_image(rig[0][1], 81)
    pin = (0.7 * width, 0.65 * width, (width - 1) / 2.0 + 0.25, (height - 1) / 2.0)
    with models_of(reg, rig) as models, DepthModels(reg, [None, None]) as identity, Device(hip) as dev:
        for img, metres in ((raw, A.metres_convert_to(raw)), (depth, depth)):
            depth_type = 0 if img.dtype == np.uint16 else 1
            assert models.undistort([img], [1])[0].tobytes() == metres.tobytes()              # a sensor without a model
            assert identity.undistort([img, img], [0, 1]).tobytes() == metres.tobytes() * 2
            out = np.full((height, width), 9.0, F)
            assert undistort_call(L, reg, None, [(img.ctypes.data, img.strides[0])], None, depth_type, height, width, 0, [out.ctypes.data], width * 4) == 0   # no set
            assert out.tobytes() == metres.tobytes()
        for img in (raw, depth):
            z = A.metres_map_entries(img) if img.dtype == np.uint16 else img
            want = np.stack([A.pinhole_cloud(z, pin)] * 2)
            for on_device in (0, 1):
                rc, got = clouds_call(L, reg, None, [img, img], 1, 2, pin, dev, on_device)          # no set: k_rig_pinhole_cloud's bytes
                assert rc == 0 and got.tobytes() == want.tobytes()
            rc, got = clouds_call(L, reg, identity, [img, img], 1, 2, pin, dev)
            assert rc == 0 and got.tobytes() == want.tobytes()
        assert (A.metres_map_entries(raw) != A.metres_convert_to(raw)).any()


# ---- 3: the cloud formation with models
@pytest.mark.parametrize("dtype", ("uint16", "float32"))
def test_rig_depth_clouds_with_models(hip_lib, hip, reg, tmp_path, dtype):
    L = hip_lib
    shape = A.SHAPES[1]
    width, height = shape[:2]
    rig = [rig_of(tmp_path, shape)[k] for k in (0, 1, 3)]          # a model of sums, none, the varied file
    K, S = 2, 3
    pin = (0.7 * width, 0.65 * width, (width - 1) / 2.0 + 0.25, (height - 1) / 2.0)
    images = [A.raw_image(height, width, 90 + i) if dtype == "uint16" else A.depth_image(rig[0][1], 90 + i) for i in range(K * S)]
    want = []
    for i, img in enumerate(images):
        z = A.metres_map_entries(img) if dtype == "uint16" else img
        want.append(A.pinhole_cloud(host_undistort(rig, i % S, z), pin))            # restated conversion -> host undistort -> restated ray product
    want = np.stack(want)
    plain = np.stack([A.pinhole_cloud(A.metres_map_entries(img) if dtype == "uint16" else img, pin) for img in images])
    assert want[0].tobytes() != plain[0].tobytes() and want[1].tobytes() == plain[1].tobytes()
    with models_of(reg, rig) as models, Device(hip) as dev:
        for on_device in (0, 1):
            rc, got = clouds_call(L, reg, models, images, K, S, pin, dev, on_device)
            assert rc == 0 and got.tobytes() == want.tobytes(), on_device
        # the Python mirror writes the same clouds
        out = np.zeros_like(want)
        p = dev.put(out)
        models.rig_clouds(images, pin, K, p)
        assert dev.get(p, out).tobytes() == want.tobytes()


# ---- 4: the calibration on corrected depth
def test_calibrate_rig_depth_models(hip_lib, hip, reg, tmp_path):
    from rgbd360_amd.voxel_map import VoxelMap
    L = hip_lib
    sc = RC.scene()
    shape = A.SHAPES[2]
    rows, cols = 6, 8
    K, S = 2, 2
    pin = (0.7 * cols, 0.7 * cols, (cols - 1) / 2.0 + 0.25, (rows - 1) / 2.0)
    Tt, E = sc["T"][:K], sc["E"][:S]
    E0 = np.stack([RG.A.perturbed(E[s], 0.01, 0.005, 40 + s) for s in range(S)])
    images = []
    for k in range(K):
        for s in range(S):
            img = np.round(RG.cast_depth(Tt[k].astype(float) @ E[s].astype(float), rows, cols, pin) * 1000.0).astype(np.uint16)
            img[0, 0] = 0
            images.append(img)
    rig = [from_sums(tmp_path, shape, 1, 41, 0.01), (None, None)]
    kw = dict(max_iters=3, eps=0.0, max_flatness=RC.MAX_FLATNESS, min_input_matches=1)
    frames = [(img.ctypes.data, img.strides[0]) for img in images]

    def depth_call(m, models):
        from rgbd360_amd import _lib
        p = m.rig_calib_params(**kw)
        Tc, Ec = RG.CPU.cm(Tt), RG.CPU.cm(E0)
        res, sen = _lib.RigCalibResult(), (_lib.RigCalibSensor * S)()
        I = (_lib.MapBatchFrame * len(frames))()
        for k, (addr, step) in enumerate(frames):
            I[k].depth, I[k].depth_step = addr, step
        rc = L.rgbd360_map_calibrate_rig_depth_models(m._handle(), None if models is None else models._handle(), I, 0, rows, cols, *[C.c_float(v) for v in pin], K, S,
                                                      0, RG.vp(Tc), RG.vp(Ec), C.byref(p), C.byref(res), sen)
        return (rc, Tc.tobytes(), Ec.tobytes(), bytes(res), bytes(sen)), m.rig_calib_trace()

    with VoxelMap(reg, 0.1, 1 << 16) as m, models_of(reg, rig) as models, Device(hip) as dev:
        m.set_box(None, None)
        m.insert_cloud(np.ascontiguousarray(sc["map_cloud"]), None, np.eye(4, dtype=F))
        # with a set: rig_depth_clouds followed by calibrate_rig_clouds on device memory
        rc, clouds = clouds_call(L, reg, models, images, K, S, pin, dev)
        assert rc == 0
        addrs = [dev.put(c) for c in clouds]
        want = RG.Call(L, m, list(clouds), Tt, E0, on_device=1, addresses=addrs, **kw)
        want_trace = m.rig_calib_trace()
        got, got_trace = depth_call(m, models)
        assert want.rc == RG.OK and want.res.iterations == 3 and want.res.n_matched > 0.5 * K * S * rows * cols
        assert got == want.bytes and got_trace == want_trace and len(got_trace) == 3
        # without a set: rgbd360_map_calibrate_rig_depth
        plain = RG.Call(L, m, None, Tt, E0, depth=(frames, 0, rows, cols, pin), **kw)
        plain_trace = m.rig_calib_trace()
        got0, got0_trace = depth_call(m, None)
        assert got0 == plain.bytes and got0_trace == plain_trace
        assert got0 != got                                        # the correction reaches the result
        # the Python mirror
        T1, E1, res = m.calibrate_rig_depth(images, pin, Tt, E0, models=models, **kw)
        assert RG.CPU.cm(E1).tobytes() == got[2] and res["n_matched"] == want.res.n_matched


# ---- 5: a model judged against the map
def evaluate(reg, gmap, models, sensor, meas, pose, **kw):
    from rgbd360_amd.depth_train import evaluate_map
    return evaluate_map(reg, gmap, models, sensor, meas, *PIN, pose, **kw)


@pytest.mark.parametrize("name", ("corner", "outward", "grazing_floor"))
def test_evaluate_map_equals_the_restatement_bit_for_bit(reg, scene, gmap, tmp_path, name):
    from rgbd360_amd.depth_train import DepthTrainer
    rig = rig_of(tmp_path, A.SHAPES[0])
    cast, meas, pose = scene["casts"][name], scene["meas"][name], POSES[name]
    with models_of(reg, rig) as models, DepthTrainer(reg, W, H, 8, 6, 2.0, 1) as trainer:
        for sensor in (0, 1, 3):
            for params in (dict(), dict(require_plane=0, min_cos_incidence=0.5)):
                want, want_stats = A.eval_map(cast, meas, rig[sensor][1], **params)
                got, stats = evaluate(reg, gmap, models, sensor, meas, pose, **params)
                trainer.clear()
                assert stats == trainer.accumulate_map(gmap, meas, *PIN, pose, want_gt=False, **params)[1] == want_stats
                print(name, sensor, params, got)
                assert got == want and got["n"] == stats["n_examples"]
                if rig[sensor][1] is None:
                    assert (got["cor_e"], got["cor_ee"]) == (got["raw_e"], got["raw_ee"])
                    assert evaluate(reg, gmap, None, 0, meas, pose, **params)[0] == got        # no set at all
                assert evaluate(reg, gmap, models, sensor, meas, pose, **params) == (got, stats)      # a second run: the same bits
        if name == "outward":
            assert got["n"] == 0
            return
        assert got["n"] > 200 and got["raw_ee"] > 0 and got["cor_ee"] != got["raw_ee"]
        # the image split into two calls (the halves masked with zeros), the sums added
        whole, _ = evaluate(reg, gmap, models, 0, meas, pose)
        top, bottom = meas.copy(), meas.copy()
        top[H // 2:], bottom[:H // 2] = 0, 0
        assert A.add_sums(evaluate(reg, gmap, models, 0, top, pose)[0], evaluate(reg, gmap, models, 0, bottom, pose)[0]) == whole
        if name == "corner":
            # uint16 millimetres: 0.001f * (float)raw, here and in the restatement
            raw = np.round(np.where(np.isfinite(meas) & (meas > 0), meas, 0) * 1000).astype(np.uint16)
            got, stats = evaluate(reg, gmap, models, 0, raw, pose)
            assert (got, stats) == A.eval_map(cast, raw, rig[0][1]) and got["n"] > 200
            top, bottom = raw.copy(), raw.copy()
            top[H // 2:], bottom[:H // 2] = 0, 0
            assert A.add_sums(evaluate(reg, gmap, models, 0, top, pose)[0], evaluate(reg, gmap, models, 0, bottom, pose)[0]) == got


# ---- 6: the loop end to end
def test_the_loop_end_to_end_on_the_device(reg, scene, gmap, tmp_path):
    from rgbd360_amd.depth_train import DepthModels, DepthTrainer, eval_figures
    train, held = TG.end_to_end_inputs()
    with DepthTrainer(reg, W, H, 8, 6, 2.0, 1) as t:
        for pose, z in train:
            t.accumulate_map(gmap, TG.distort(z), *PIN, pose, want_gt=False)
        model = t.model()
        t.save(tmp_path / "model")
    ref = A.read_model(tmp_path / "model")
    total, want = {k: 0 for k in A.EVAL_NAMES}, {k: 0 for k in A.EVAL_NAMES}
    with DepthModels(reg, [model]) as models:
        for pose, z in held:
            meas = TG.distort(z)
            sums, _ = models.evaluate(gmap, 0, meas, *PIN, pose)
            total = A.add_sums(total, sums)
            want = A.add_sums(want, A.eval_map(T.cast_pinhole(scene["ref"], TG.LEAF, H, W, pose=pose, **PINHOLE), meas, ref)[0])
    raw_rms, cor_rms, raw_bias, cor_bias = eval_figures(total)
    ratio = np.sqrt(total["raw_ee"] / total["cor_ee"])
    print("held-out images against the map: RMS %.4f m raw, %.4f m corrected (ratio %.2f); bias %.4f m raw, %.4f m corrected; %d examples"
          % (raw_rms, cor_rms, ratio, raw_bias, cor_bias, total["n"]))
    assert total == want and total["n"] > 10000
    assert ratio >= 0.5 * TG.RATIO_RESTATEMENT


# ---- 7: refusals
def test_refusals(hip_lib, hip, reg, scene, gmap, tmp_path):
    from rgbd360_amd import _lib
    from rgbd360_amd.depth_train import DepthModels
    from rgbd360_amd.register import RegisterPhotoICP, Rgbd360Error
    L = hip_lib
    shape = A.SHAPES[0]
    rig = rig_of(tmp_path, shape)
    small = from_sums(tmp_path, A.SHAPES[2], 1, 1)[0]
    err = lambda: L.rgbd360_last_error(reg._ctx())
    for bad in ([rig[0][0], small], [], [None] * 17):
        with pytest.raises(Rgbd360Error):
            DepthModels(reg, bad)
    h = C.c_void_p(5)
    assert L.rgbd360_depth_models_create(None, None, 1, C.byref(h)) == -1 and h.value is None
    assert L.rgbd360_depth_models_create(reg._ctx(), None, 1, C.byref(h)) == -1 and b"null" in err()
    assert L.rgbd360_depth_models_bytes(None) == 0 and L.rgbd360_depth_models_set(None, 0, None) == -1
    L.rgbd360_depth_models_destroy(None)
    depth = A.depth_image(rig[0][1], 3)
    other = RegisterPhotoICP(device=0)
    try:
        with models_of(reg, rig) as models, models_of(other, rig) as foreign, Device(hip) as dev:
            for sensor, model in ((4, rig[0][0]), (-1, rig[0][0]), (0, small)):
                with pytest.raises(Rgbd360Error):
                    models.set(sensor, model)
            # rgbd360_depth_undistort
            out = np.full((H, W), 9.0, F)
            frame, outs = [(depth.ctypes.data, W * 4)], [out.ctypes.data]
            call = lambda *a: undistort_call(L, reg, *a)
            cases = dict(null_ctx=lambda: L.rgbd360_depth_undistort(None, models._handle(), None, None, 1, 1, H, W, 0, None, W * 4),
                         null_images=lambda: L.rgbd360_depth_undistort(reg._ctx(), models._handle(), None, (C.c_int * 1)(0), 1, 1, H, W, 0, (C.c_void_p * 1)(*outs), W * 4),
                         null_image=lambda: call(models, [(None, W * 4)], [0], 1, H, W, 0, outs, W * 4),
                         null_out=lambda: call(models, frame, [0], 1, H, W, 0, None, W * 4),
                         null_sensors=lambda: call(models, frame, None, 1, H, W, 0, outs, W * 4),
                         size=lambda: call(models, frame, [0], 1, H - 1, W, 0, outs, W * 4),
                         in_step=lambda: call(models, [(depth.ctypes.data, W * 4 - 1)], [0], 1, H, W, 0, outs, W * 4),
                         out_step=lambda: call(models, frame, [0], 1, H, W, 0, outs, W * 4 - 1),
                         depth_type=lambda: call(models, frame, [0], 2, H, W, 0, outs, W * 4),
                         sensor_high=lambda: call(models, frame, [4], 1, H, W, 0, outs, W * 4),
                         sensor_low=lambda: call(models, frame, [-1], 1, H, W, 0, outs, W * 4),
                         foreign=lambda: call(foreign, frame, [0], 1, H, W, 0, outs, W * 4))
            for name, f in cases.items():
                assert f() == -1 and (name == "null_ctx" or len(err()) > 0), name
                assert (out == 9.0).all(), name
            assert call(models, [], [], 1, H, W, 0, [], W * 4) == 0 and call(models, frame, [0], 1, 0, 0, 0, outs, W * 4) == 0 and (out == 9.0).all()
            # rgbd360_rig_depth_clouds
            pin = PIN
            imgs = [depth] * 4
            for name, args in dict(null_ctx=None, foreign=(foreign, imgs, 1, 4, pin), size=(models, [depth[:-1]] * 4, 1, 4, pin), sensors=(models, imgs[:2], 1, 2, pin),
                                   too_many=(None, imgs, 1, 17, pin), no_frames=(models, imgs, 0, 4, pin), fx=(models, imgs, 1, 4, (0.0,) + pin[1:]),
                                   nan=(models, imgs, 1, 4, pin[:3] + (np.nan,))).items():
                if args is None:
                    assert L.rgbd360_rig_depth_clouds(None, None, None, 1, 1, 1, H, W, *[C.c_float(v) for v in pin], 0, None) == -1
                    continue
                rc, got = clouds_call(L, reg, args[0], args[1], args[2], args[3], args[4], dev)
                assert rc == -1 and len(err()) > 0 and (got == 7.0).all(), name
            I = (_lib.MapBatchFrame * 4)()
            for k in range(4):
                I[k].depth, I[k].depth_step = depth.ctypes.data, W * 4
            fpin = [C.c_float(v) for v in pin]
            assert L.rgbd360_rig_depth_clouds(reg._ctx(), models._handle(), I, 1, 4, 1, H, W, *fpin, 0, None) == -1          # no output
            assert L.rgbd360_rig_depth_clouds(reg._ctx(), models._handle(), None, 1, 4, 1, H, W, *fpin, 0, None) == -1
            assert L.rgbd360_rig_depth_clouds(reg._ctx(), models._handle(), I, 1, 4, 3, H, W, *fpin, 0, None) == -1          # a bad depth_type
            I[2].depth_step = W * 4 - 2
            assert L.rgbd360_rig_depth_clouds(reg._ctx(), models._handle(), I, 1, 4, 1, H, W, *fpin, 0, None) == -1 and b"row step" in err()
            # rgbd360_map_calibrate_rig_depth_models
            Tc, Ec = np.tile(np.eye(4, dtype=F).reshape(1, 16), (1, 1)), np.tile(np.eye(4, dtype=F).reshape(1, 16), (4, 1))
            before = (Tc.tobytes(), Ec.tobytes())
            I[2].depth_step = W * 4
            for set_, rows, S in ((foreign, H, 4), (models, H - 1, 4), (models, H, 3)):
                assert L.rgbd360_map_calibrate_rig_depth_models(gmap._handle(), set_._handle(), I, 1, rows, W, *fpin, 1, S, 0, RG.vp(Tc), RG.vp(Ec), None, None,
                                                                None) == -1
                assert len(L.rgbd360_map_last_error(gmap._handle())) > 0 and (Tc.tobytes(), Ec.tobytes()) == before
            assert L.rgbd360_map_calibrate_rig_depth_models(None, None, I, 1, H, W, *fpin, 1, 4, 0, RG.vp(Tc), RG.vp(Ec), None, None, None) == -1
            # rgbd360_depth_evaluate_map: those above and what accumulate_map refuses
            meas, pose = scene["meas"]["corner"], POSES["corner"]
            for kw in (dict(max_range=0.0), dict(max_range=16.5), dict(min_mult=1.2, max_mult=1.1), dict(min_cos_incidence=1.5), dict(max_steps=0), dict(min_support=0)):
                with pytest.raises(Rgbd360Error):
                    evaluate(reg, gmap, models, 0, meas, pose, **kw)
            bad_pose = pose.copy()
            bad_pose[0, 3] = np.nan
            for args in ((models, 4, meas, pose), (models, -1, meas, pose), (foreign, 0, meas, pose), (models, 0, meas[:-1], pose), (models, 0, meas, bad_pose)):
                with pytest.raises(Rgbd360Error):
                    evaluate(reg, gmap, *args)
            from rgbd360_amd.depth_train import evaluate_map
            with pytest.raises(Rgbd360Error):
                evaluate_map(reg, gmap, models, 0, meas, 0.0, *PIN[1:], pose)
            st, sums = _lib.DepthTrainStats(n_pixels=5), _lib.DepthEvalSums(n=5)
            g = np.ascontiguousarray(pose.T.reshape(16))
            tail = (*fpin, RG.vp(g), 0, None, C.byref(st), C.byref(sums))
            assert L.rgbd360_depth_evaluate_map(reg._ctx(), None, models._handle(), 0, RG.vp(meas), W * 4, 1, H, W, *tail) == -1 and b"map" in err()
            assert L.rgbd360_depth_evaluate_map(reg._ctx(), gmap._handle(), models._handle(), 0, None, W * 4, 1, H, W, *tail) == -1
            assert L.rgbd360_depth_evaluate_map(reg._ctx(), gmap._handle(), models._handle(), 0, RG.vp(meas), W * 4 - 1, 1, H, W, *tail) == -1
            assert L.rgbd360_depth_evaluate_map(reg._ctx(), gmap._handle(), models._handle(), 0, RG.vp(meas), W * 4, 2, H, W, *tail) == -1
            assert L.rgbd360_depth_evaluate_map(reg._ctx(), gmap._handle(), None, 0, RG.vp(meas), 8192 * 4, 1, 4096, 8192, *tail) == -1 and b"2^24" in err()
            assert L.rgbd360_depth_evaluate_map(None, gmap._handle(), None, 0, RG.vp(meas), W * 4, 1, H, W, *tail) == -1
            assert (st.n_pixels, sums.n) == (5, 5)                                     # outputs untouched by every refusal
            assert L.rgbd360_depth_evaluate_map(reg._ctx(), gmap._handle(), models._handle(), 0, RG.vp(meas), W * 4, 1, 0, 0, *tail) == 0
            assert (st.n_pixels, sums.n) == (0, 0)
    finally:
        other.close()


# ---- 8: a sensor's model replaced
def test_set_equals_a_fresh_set(reg, tmp_path):
    from rgbd360_amd.depth_train import DepthModels
    shape = A.SHAPES[1]
    rig = rig_of(tmp_path, shape)
    newer = from_sums(tmp_path, shape, 1, 77)
    images = [A.depth_image(rig[0][1], 100 + i) for i in range(4)]
    with models_of(reg, rig) as models:
        before = models.undistort(images, range(4))
        for sensor, (model, ref) in ((1, newer), (3, (None, None)), (0, rig[3])):
            models.set(sensor, model)
            rig[sensor] = (model, ref)
            with DepthModels(reg, [m for m, _ in rig]) as fresh:
                assert models.nbytes == fresh.nbytes
                got = models.undistort(images, range(4))
                assert got.tobytes() == fresh.undistort(images, range(4)).tobytes()
                assert got[sensor].tobytes() == host_undistort(rig, sensor, images[sensor]).tobytes() != before[sensor].tobytes()
