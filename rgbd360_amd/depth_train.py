"""Training the sensors' intrinsic depth models against the resident voxel map.

Mirror of rgbd360_depth_trainer_* (include/rgbd360_hip.h, "training the depth model"; csrc/depth_train.h): the training half of CLAMS'
DiscreteDepthDistortionModel (addExample / accumulate, discrete_depth_distortion_model.cpp:21-36, 193-217) with exact integer sums on the
device and the ground truth cast out of the map:

    trainer = DepthTrainer(reg, 320, 240, bin_width=4, bin_height=3)
    gmap.set_box(near_lo, near_hi); gmap.insert_sphere(...)          # the map from trusted short-range data
    gt, stats = trainer.accumulate_map(gmap, raw_depth, fx, fy, cx, cy, frame_pose @ Rt_sensor)
    trainer.save(path)                                               # what DepthModel(path, 1) and Calib360 load
    corrected = trainer.model().undistort(raw_depth_m)

and of rgbd360_depth_models_* (csrc/depth_apply.h): DepthModels keeps the trained models on the device, corrects images there (undistort,
rig_clouds, VoxelMap.calibrate_rig_depth(models=...)) and judges them against the map (evaluate, eval_figures).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .register import DepthModel, Rgbd360Error, _ptr, pose_to_cm
from .voxel_map import _as_dict

_RAY_FIELDS = ("min_count", "t_min", "t_max", "max_offset", "max_steps")
_NORMAL_FIELDS = {"normal_min_count": "min_count", "min_support": "min_support", "max_flatness": "max_flatness", "max_shift": "max_shift"}
_OWN_FIELDS = ("require_plane", "min_cos_incidence", "min_mult", "max_mult", "max_range")


class DepthTrainer:
    def __init__(self, reg, width: int, height: int, bin_width: int = 8, bin_height: int = 6, bin_depth: float = 2.0, smoothing: int = 1):
        """reg: the RegisterPhotoICP whose context (device, stream) the trainer lives on; the arguments are those of
        DiscreteDepthDistortionModel's constructor.  close() the trainer before the context goes."""
        self._L = _lib.load()
        self._reg = reg
        ctx = reg._ctx()
        h = C.c_void_p()
        rc = self._L.rgbd360_depth_trainer_create(ctx, int(width), int(height), int(bin_width), int(bin_height), float(bin_depth), int(smoothing), C.byref(h))
        if rc != 0:
            raise Rgbd360Error(f"rgbd360_depth_trainer_create failed ({rc}): {self._L.rgbd360_last_error(ctx).decode()}")
        self._h = h
        self._ctx_value = ctx.value
        self.width, self.height, self.bin_width, self.bin_height = int(width), int(height), int(bin_width), int(bin_height)
        self.bin_depth, self.smoothing = float(bin_depth), int(smoothing)
        self.shape = (self.height // self.bin_height, self.width // self.bin_width, int(np.ceil(10.0 / self.bin_depth)))

    # ---- lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None:
            if self._reg._h is not None and self._reg._h.value == self._ctx_value:
                self._L.rgbd360_depth_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if self._h is None:
            raise Rgbd360Error("DepthTrainer is closed")
        if self._reg._h is None or self._reg._h.value != self._ctx_value:
            raise Rgbd360Error("DepthTrainer: the registration context was closed or recreated after the trainer was made")
        return self._h

    def _check(self, rc: int):
        if rc != 0:
            raise Rgbd360Error(f"rgbd360_depth_trainer call failed ({rc}): {self._L.rgbd360_depth_trainer_last_error(self._h).decode()}")

    # ---- parameters
    def params(self, gmap=None, **fields):
        """rgbd360_depth_default_train_params (of `gmap`, a VoxelMap, for the map route) with the given fields replaced: raycast_params'
        fields, normal_min_count / min_support / max_flatness / max_shift, and require_plane, min_cos_incidence, min_mult, max_mult,
        max_range."""
        p = _lib.DepthTrainParams()
        self._L.rgbd360_depth_default_train_params(None if gmap is None else gmap._handle(), C.byref(p))
        for name, v in fields.items():
            if v is None:
                continue
            if name in _RAY_FIELDS:
                setattr(p.ray, name, v)
            elif name in _NORMAL_FIELDS:
                setattr(p.normal, _NORMAL_FIELDS[name], v)
            elif name in _OWN_FIELDS:
                setattr(p, name, v)
            else:
                raise TypeError(f"DepthTrainParams has no field {name!r}")
        return p

    @staticmethod
    def _image(a, what):
        a = np.asarray(a)
        if a.ndim != 2 or a.strides[1] != a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
            a = np.ascontiguousarray(a)
        if a.ndim != 2:
            raise Rgbd360Error(f"DepthTrainer: {what} must be a 2-d image")
        if a.dtype == np.uint16:
            return a, 0
        if a.dtype != np.float32:
            a = np.ascontiguousarray(a, np.float32)
        return a, 1

    # ---- the two routes
    def accumulate(self, gt, meas, **fields):
        """CLAMS' accumulate(ground_truth, measurement): two images of the trainer's size, both uint16 millimetres or both float32 metres.
        Returns the statistics as a dict."""
        g, gt_type = self._image(gt, "gt")
        m, m_type = self._image(meas, "meas")
        if gt_type != m_type:
            raise Rgbd360Error("DepthTrainer.accumulate: gt and meas must have one dtype (uint16 millimetres or float32 metres)")
        if g.shape != m.shape:
            raise Rgbd360Error("DepthTrainer.accumulate: gt and meas must have the same shape")
        p = self.params(**fields)
        st = _lib.DepthTrainStats()
        self._check(self._L.rgbd360_depth_trainer_accumulate_images(self._handle(), _ptr(g), g.strides[0], _ptr(m), m.strides[0], m_type, m.shape[0],
                                                                    m.shape[1], 0, C.byref(p), C.byref(st)))
        return _as_dict(st)

    def accumulate_map(self, gmap, meas, fx, fy, cx, cy, sensor_pose, want_gt=True, **fields):
        """The ground truth cast out of `gmap` (a VoxelMap of the same context) along the pinhole rays of a sensor at sensor_pose (4x4
        world <- sensor).  Returns (gt_out [rows, cols] float32 or None, the statistics as a dict)."""
        m, m_type = self._image(meas, "meas")
        p = self.params(gmap, **fields)
        g = pose_to_cm(sensor_pose)
        gt = np.zeros(m.shape, np.float32) if want_gt else None
        st = _lib.DepthTrainStats()
        self._check(self._L.rgbd360_depth_trainer_accumulate_map(self._handle(), gmap._handle(), _ptr(m), m.strides[0], m_type, m.shape[0], m.shape[1],
                                                                 float(fx), float(fy), float(cx), float(cy), _ptr(g), 0, C.byref(p),
                                                                 None if gt is None else _ptr(gt), C.byref(st)))
        return gt, _as_dict(st)

    # ---- sums, merge, model, file
    def clear(self):
        self._check(self._L.rgbd360_depth_trainer_clear(self._handle()))

    def sums(self):
        """(count, num, den): int64 arrays [num_bins_y][num_bins_x][num_bins]; num and den in units of 2^-20 m^2."""
        out = [np.zeros(self.shape, np.int64) for _ in range(3)]
        self._check(self._L.rgbd360_depth_trainer_sums(self._handle(), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return tuple(out)

    def add_sums(self, count, num, den):
        """The sums of another trainer of this shape (another process, another GPU, a checkpoint) added to this one."""
        arrs = [np.ascontiguousarray(a, np.int64) for a in (count, num, den)]
        if any(a.shape != self.shape for a in arrs):
            raise Rgbd360Error("DepthTrainer.add_sums: count, num and den must have the shape %s" % (self.shape,))
        self._check(self._L.rgbd360_depth_trainer_add_sums(self._handle(), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2])))

    def model(self) -> DepthModel:
        h = C.c_void_p()
        self._check(self._L.rgbd360_depth_trainer_model(self._handle(), C.byref(h)))
        return DepthModel._from_handle(h)

    def save(self, path):
        m = self.model()
        try:
            m.save(path)
        finally:
            m.close()

    def set_form(self, form: int):
        """Measurement: how the kernel adds (0 per-lane atomics, 1 per-wave merge, 2 per-block LDS table, the default); same bits."""
        self._check(self._L.rgbd360_depth_trainer_set_form(self._handle(), int(form)))


EVAL_SUM_NAMES = ("n", "raw_e", "raw_ee", "cor_e", "cor_ee")
EVAL_FIX = 1073741824.0      # the sums' unit: 2^-30 m (bias) and 2^-30 m^2 (mean square)


def eval_figures(sums):
    """(raw RMS, corrected RMS, raw bias, corrected bias) in metres of evaluation sums (a dict; sums of several images added)."""
    n = max(int(sums["n"]), 1)
    return (float(np.sqrt(sums["raw_ee"] / EVAL_FIX / n)), float(np.sqrt(sums["cor_ee"] / EVAL_FIX / n)), sums["raw_e"] / EVAL_FIX / n,
            sums["cor_e"] / EVAL_FIX / n)


def _frames(images, what):
    """Images of one size and type (uint16 millimetres or float32 metres; rows may be strided) as (arrays, MapBatchFrame array, depth_type)."""
    ds = []
    for img in images:
        d = np.asarray(img)
        if d.ndim != 2 or d.dtype not in (np.uint16, np.float32):
            raise Rgbd360Error(f"{what}: an image must be HxW uint16 millimetres or float32 metres")
        if d.size and d.strides[1] != d.itemsize:
            d = np.ascontiguousarray(d)
        if ds and (d.shape != ds[0].shape or d.dtype != ds[0].dtype):
            raise Rgbd360Error(f"{what}: the images of a call share one size and depth type")
        ds.append(d)
    if not ds:
        raise Rgbd360Error(f"{what}: no images")
    I = (_lib.MapBatchFrame * len(ds))()
    for k, d in enumerate(ds):
        I[k].depth, I[k].depth_step = d.ctypes.data, d.strides[0]
    return ds, I, 0 if ds[0].dtype == np.uint16 else 1


class DepthModels:
    """rgbd360_depth_models_*: the depth models of a rig's sensors resident on the device (csrc/depth_apply.h), and what runs on them:
    undistort (Frame360::undistort's step, one launch over all images), rig_clouds (the rig calibration's cloud formation with the
    correction), evaluate (raw against corrected error of a sensor's image against the map).  VoxelMap.calibrate_rig_depth(models=...)
    takes one.

        models = DepthModels(reg, [trainer.model() for trainer in trainers])
        corrected = models.undistort(raw_depths, sensors=range(8))
        sums, stats = models.evaluate(gmap, s, held_out_depth, fx, fy, cx, cy, frame_pose @ Rt_sensor)
    """

    def __init__(self, reg, models):
        """models: one DepthModel or None (identity) per sensor; the objects are not kept.  close() before the context goes."""
        self._L = _lib.load()
        self._reg = reg
        ctx = reg._ctx()
        arr = (C.c_void_p * max(len(models), 1))(*[None if m is None else m._h for m in models])
        h = C.c_void_p()
        rc = self._L.rgbd360_depth_models_create(ctx, arr, len(models), C.byref(h))
        if rc != 0:
            raise Rgbd360Error(f"rgbd360_depth_models_create failed ({rc}): {self._L.rgbd360_last_error(ctx).decode()}")
        self._h = h
        self._ctx_value = ctx.value
        self.n_sensors = len(models)

    def close(self):
        if getattr(self, "_h", None) is not None:
            if self._reg._h is not None and self._reg._h.value == self._ctx_value:
                self._L.rgbd360_depth_models_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if self._h is None:
            raise Rgbd360Error("DepthModels is closed")
        if self._reg._h is None or self._reg._h.value != self._ctx_value:
            raise Rgbd360Error("DepthModels: the registration context was closed or recreated after the set was made")
        return self._h

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise Rgbd360Error(f"{what} failed ({rc}): {self._L.rgbd360_last_error(self._reg._ctx()).decode()}")

    @property
    def nbytes(self) -> int:
        """Device memory of the packed models."""
        return int(self._L.rgbd360_depth_models_bytes(self._handle()))

    def set(self, sensor: int, model):
        """Replaces one sensor's model (None: identity), e.g. after a training round; the size rules of the constructor hold."""
        self._check(self._L.rgbd360_depth_models_set(self._handle(), int(sensor), None if model is None else model._h), "rgbd360_depth_models_set")

    def undistort(self, images, sensors):
        """The corrected float32-metre copies of host images (uint16 millimetres, converted (float)(0.001 * (double)raw) as
        Frame360::undistort does, or float32 metres), image i by the model of sensors[i]: one launch, one synchronisation."""
        ds, I, depth_type = _frames(images, "DepthModels.undistort")
        sensors = [int(s) for s in sensors]
        if len(sensors) != len(ds):
            raise Rgbd360Error("DepthModels.undistort: one sensor per image")
        rows, cols = ds[0].shape
        out = np.zeros((len(ds), rows, cols), np.float32)
        outs = (C.c_void_p * len(ds))(*[out[i].ctypes.data for i in range(len(ds))])
        sen = (C.c_int * len(ds))(*sensors)
        self._check(self._L.rgbd360_depth_undistort(self._reg._ctx(), self._handle(), I, sen, len(ds), depth_type, rows, cols, 0, outs, cols * 4),
                    "rgbd360_depth_undistort")
        return out

    def rig_clouds(self, depths, K4, n_frames, out_ptr):
        """rgbd360_rig_depth_clouds on host images, flat frame-major (n_frames x n_sensors): the corrected clouds in the sensors' frames
        (NaN triples without a measurement) into device memory at out_ptr (a raw device pointer, e.g. torch_tensor.data_ptr(), with
        room for n_frames * n_sensors * rows * cols * 3 float32), ready for VoxelMap.calibrate_rig_clouds / insert_cloud on device memory."""
        rig_depth_clouds(self._reg, self, depths, K4, n_frames, self.n_sensors, out_ptr)

    def evaluate(self, gmap, sensor, meas, fx, fy, cx, cy, sensor_pose, **fields):
        """rgbd360_depth_evaluate_map: (sums dict over EVAL_SUM_NAMES, the trainer's statistics dict) of one sensor image against `gmap`;
        fields: DepthTrainer.params'.  Add the sums of several images and hand them to eval_figures."""
        return evaluate_map(self._reg, gmap, self, sensor, meas, fx, fy, cx, cy, sensor_pose, **fields)


def rig_depth_clouds(reg, models, depths, K4, n_frames, n_sensors, out_ptr):
    """rgbd360_rig_depth_clouds with `models` a DepthModels or None (then the clouds rgbd360_map_calibrate_rig_depth forms)."""
    L = _lib.load()
    ds, I, depth_type = _frames(depths, "rig_depth_clouds")
    if len(ds) != n_frames * n_sensors:
        raise Rgbd360Error("rig_depth_clouds: one image per frame and sensor")
    rows, cols = ds[0].shape
    fx, fy, cx, cy = (float(v) for v in K4)
    rc = L.rgbd360_rig_depth_clouds(reg._ctx(), None if models is None else models._handle(), I, n_frames, n_sensors, depth_type, rows, cols, fx, fy, cx, cy, 0,
                                    C.c_void_p(int(out_ptr)))
    if rc != 0:
        raise Rgbd360Error(f"rgbd360_rig_depth_clouds failed ({rc}): {L.rgbd360_last_error(reg._ctx()).decode()}")


def evaluate_map(reg, gmap, models, sensor, meas, fx, fy, cx, cy, sensor_pose, **fields):
    """rgbd360_depth_evaluate_map with `models` a DepthModels or None (then the corrected sums equal the raw ones)."""
    L = _lib.load()
    m, m_type = DepthTrainer._image(meas, "meas")
    p = _lib.DepthTrainParams()
    L.rgbd360_depth_default_train_params(gmap._handle(), C.byref(p))
    for name, v in fields.items():
        if v is None:
            continue
        if name in _RAY_FIELDS:
            setattr(p.ray, name, v)
        elif name in _NORMAL_FIELDS:
            setattr(p.normal, _NORMAL_FIELDS[name], v)
        elif name in _OWN_FIELDS:
            setattr(p, name, v)
        else:
            raise TypeError(f"DepthTrainParams has no field {name!r}")
    g = pose_to_cm(sensor_pose)
    st, sums = _lib.DepthTrainStats(), _lib.DepthEvalSums()
    rc = L.rgbd360_depth_evaluate_map(reg._ctx(), gmap._handle(), None if models is None else models._handle(), int(sensor), _ptr(m), m.strides[0], m_type,
                                      m.shape[0], m.shape[1], float(fx), float(fy), float(cx), float(cy), _ptr(g), 0, C.byref(p), C.byref(st), C.byref(sums))
    if rc != 0:
        raise Rgbd360Error(f"rgbd360_depth_evaluate_map failed ({rc}): {L.rgbd360_last_error(reg._ctx()).decode()}")
    return _as_dict(sums), _as_dict(st)
