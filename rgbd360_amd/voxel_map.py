"""Resident voxel-grid global map: posed frames accumulated into a hash grid in HBM, read out as one point per voxel.

Mirror of rgbd360_map_* (include/rgbd360_hip.h, csrc/voxel_map.h): the map half of the reference's odometry loop
(OdometryRGBD360.cpp:242-268: filterEuclidean, transformPointCloud at currentPose, globalMap +=, filterVoxel):

    gmap = VoxelMap(reg, leaf=0.05, capacity=1 << 20)
    stats = gmap.insert_sphere(rgb, depth, currentPose, convention=0)
    xyz, rgb, count, key = gmap.extract()          # sorted by (i_z, i_y, i_x)

Every point has weight one and the sums are integers: the map does not depend on the order of the frames.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from .register import Rgbd360Error, _ptr, pose_to_cm

MAP_FULL = 3      # RGBD360_MAP_FULL


class VoxelMap:
    def __init__(self, reg, leaf: float = 0.05, capacity: int = 1 << 20):
        """reg: the RegisterPhotoICP whose context (device, stream) the map lives on; its setters recreate the context, so configure
        it first and close() the map before it."""
        self._L = _lib.load()
        self._reg = reg
        ctx = reg._ctx()
        h = C.c_void_p()
        rc = self._L.rgbd360_map_create(ctx, float(leaf), int(capacity), C.byref(h))
        if rc != 0:
            raise Rgbd360Error(f"rgbd360_map_create failed ({rc}): {self._L.rgbd360_last_error(ctx).decode()}")
        self._h = h
        self._ctx_value = ctx.value
        self.full = False        # the last insert dropped points of new voxels (RGBD360_MAP_FULL)

    # ---- lifecycle
    def close(self):
        if self._h is not None:
            if self._reg._h is not None and self._reg._h.value == self._ctx_value:
                self._L.rgbd360_map_destroy(self._h)
            else:        # the map's stream is gone with its context: the table cannot be freed safely any more
                warnings.warn("VoxelMap.close: the registration context was closed or recreated before the map; its device memory "
                              "is not freed (close the map first)", ResourceWarning, stacklevel=2)
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
            raise Rgbd360Error("VoxelMap is closed")
        if self._reg._h is None or self._reg._h.value != self._ctx_value:
            raise Rgbd360Error("VoxelMap: the registration context was closed or recreated (a setter was called) after the map was made")
        return self._h

    def _check(self, rc: int):
        if rc < 0:
            raise Rgbd360Error(f"rgbd360_map call failed ({rc}): {self._L.rgbd360_map_last_error(self._h).decode()}")
        return rc

    # ---- parameters
    @property
    def bytes(self) -> int:
        return int(self._L.rgbd360_map_bytes(self._handle()))

    def set_box(self, lo=None, hi=None):
        """lo, hi: three floats each, limits included; both None: no box."""
        if (lo is None) != (hi is None):
            raise Rgbd360Error("VoxelMap.set_box: both limits or none")
        if lo is None:
            self._check(self._L.rgbd360_map_set_box(self._handle(), None, None))
            return
        lo = np.ascontiguousarray(lo, np.float32).reshape(3)
        hi = np.ascontiguousarray(hi, np.float32).reshape(3)
        self._check(self._L.rgbd360_map_set_box(self._handle(), _ptr(lo), _ptr(hi)))

    # ---- insertion
    def _stats(self, rc, st):
        self.last_status = self._check(rc)
        self.full = rc == MAP_FULL
        return {name: int(getattr(st, name)) for name, _ in _lib.MapStats._fields_}

    def insert_sphere(self, rgb, depth, pose, convention: int = 0):
        """rgb: HxWx3 uint8 or None; depth: HxW uint16 millimetres or float32 metres (rows may be strided); pose: 4x4 world <- frame.
        Returns the call's statistics; self.full tells whether points were dropped."""
        d = np.asarray(depth)
        if d.dtype not in (np.uint16, np.float32) or d.ndim != 2:
            raise Rgbd360Error("VoxelMap.insert_sphere: depth must be HxW uint16 millimetres or float32 metres")
        if d.size and d.strides[1] != d.dtype.itemsize:
            d = np.ascontiguousarray(d)
        c = None
        if rgb is not None:
            c = np.asarray(rgb)
            if c.dtype != np.uint8 or c.shape != d.shape + (3,):
                raise Rgbd360Error("VoxelMap.insert_sphere: rgb must be HxWx3 uint8 of the depth image's size")
            if c.size and c.strides[1:] != (3, 1):
                c = np.ascontiguousarray(c)
        p = pose_to_cm(pose)
        st = _lib.MapStats()
        rc = self._L.rgbd360_map_insert_sphere(self._handle(), None if c is None else _ptr(c), 0 if c is None else c.strides[0], _ptr(d),
                                               d.strides[0], 0 if d.dtype == np.uint16 else 1, d.shape[0], d.shape[1], int(convention),
                                               _ptr(p), 0, C.byref(st))
        return self._stats(rc, st)

    def insert_cloud(self, xyz, rgb3, pose):
        """xyz: n x 3 float32 in the frame's coordinates; rgb3: n x 3 uint8 or None."""
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        c = None
        if rgb3 is not None:
            c = np.ascontiguousarray(rgb3, np.uint8).reshape(-1, 3)
            if c.shape != x.shape:
                raise Rgbd360Error("VoxelMap.insert_cloud: one colour per point")
        p = pose_to_cm(pose)
        st = _lib.MapStats()
        rc = self._L.rgbd360_map_insert_cloud(self._handle(), _ptr(x), None if c is None else _ptr(c), x.shape[0], _ptr(p), 0, C.byref(st))
        return self._stats(rc, st)

    # ---- read-out
    def __len__(self) -> int:
        return int(self._L.rgbd360_map_size(self._handle()))

    def clear(self):
        self._check(self._L.rgbd360_map_clear(self._handle()))

    def extract(self, max_out=None):
        """(xyz [k,3] float32, rgb [k,3] uint8, count [k] int32, key [k,3] int32 = (i_x, i_y, i_z)) of the first k = min(len, max_out)
        voxels in ascending (i_z, i_y, i_x) order."""
        n = len(self)
        k = n if max_out is None else min(n, int(max_out))
        xyz = np.zeros((k, 3), np.float32)
        rgb = np.zeros((k, 3), np.uint8)
        count = np.zeros(k, np.int32)
        key = np.zeros((k, 3), np.int32)
        got = self._L.rgbd360_map_extract(self._handle(), k, _ptr(xyz), _ptr(rgb), _ptr(count), _ptr(key))
        if got != n:
            raise Rgbd360Error(f"rgbd360_map_extract failed ({got}): {self._L.rgbd360_map_last_error(self._h).decode()}")
        return xyz, rgb, count, key
