"""Training the sensors' intrinsic depth models against the resident voxel map.

Mirror of rgbd360_depth_trainer_* (include/rgbd360_hip.h, "training the depth model"; csrc/depth_train.h): the training half of CLAMS'
DiscreteDepthDistortionModel (addExample / accumulate, discrete_depth_distortion_model.cpp:21-36, 193-217) with exact integer sums on the
device and the ground truth cast out of the map:

    trainer = DepthTrainer(reg, 320, 240, bin_width=4, bin_height=3)
    gmap.set_box(near_lo, near_hi); gmap.insert_sphere(...)          # the map from trusted short-range data
    gt, stats = trainer.accumulate_map(gmap, raw_depth, fx, fy, cx, cy, frame_pose @ Rt_sensor)
    trainer.save(path)                                               # what DepthModel(path, 1) and Calib360 load
    corrected = trainer.model().undistort(raw_depth_m)
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
