"""Resident frame store: frames prepared once in HBM, arbitrary (target, source, guess) triples aligned in lock step.

Mirror of rgbd360_store_* (include/rgbd360_hip.h, csrc/frame_store.h).  The call pattern of the reference's keyframe odometry
(OdometryKeyFrame360.cpp:244-253: one keyframe against every following frame, guess = the previous result), of its SLAM front end
(KFsphere_SLAM.cpp:146-150, 370-375) and of loop closure (LoopClosure360.h:309-312, 348-351: one new keyframe against several old
ones in both roles, one PbMap guess per candidate):

    store = FrameStore(reg, capacity=16, rows=512, cols=1024)
    store.put([0, 1, 2], [(rgb0, d0), (rgb1, d1), (rgb2, d2)])
    poses, status, iters, results = store.align([(0, 1), (0, 2), (2, 0)], guesses=[G01, G02, G20], method=reg.PHOTO_DEPTH)

Every pair's pose / status / iters / hessian carry the bits reg.alignFrames360 gives for the same two frames and guess.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .register import Rgbd360Error, pose_from_cm, pose_to_cm


class FrameStore:
    def __init__(self, reg, capacity: int, rows: int, cols: int):
        """reg: the RegisterPhotoICP whose parameters, device and index arithmetic the store uses.  Its setters recreate the context:
        configure it first.  close() the store before the registration object.  The native store is created at the first use (or open())."""
        capacity, rows, cols = int(capacity), int(rows), int(cols)
        if capacity < 1:
            raise Rgbd360Error("FrameStore: capacity must be >= 1")
        if rows < 2 or cols < 8:
            raise Rgbd360Error("FrameStore: image too small")
        self._L = _lib.load()
        self._reg = reg
        self.capacity, self.rows, self.cols = capacity, rows, cols
        self._h = None
        self._ctx_value = None
        self._closed = False

    def open(self):
        """Creates the native store (HBM for `capacity` entries) now instead of at the first put; like the registration object's
        context it needs a HIP device, and fails loudly without one."""
        if self._h is None:
            ctx = self._reg._ctx()
            h = C.c_void_p()
            rc = self._L.rgbd360_store_create(ctx, self.capacity, self.rows, self.cols, C.byref(h))
            if rc != 0:
                raise Rgbd360Error(f"rgbd360_store_create failed ({rc}): {self._L.rgbd360_last_error(ctx).decode()}")
            self._h = h
            self._ctx_value = ctx.value
        return self

    # ---- lifecycle
    def close(self):
        if self._h is not None:
            if self._reg._h is not None and self._reg._h.value == self._ctx_value:
                self._L.rgbd360_store_destroy(self._h)
            self._h = None
        self._closed = True

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
        if self._closed:
            raise Rgbd360Error("FrameStore is closed")
        self.open()
        if self._reg._h is None or self._reg._h.value != self._ctx_value:
            raise Rgbd360Error("FrameStore: the registration context was closed or recreated (a setter was called) after the store was made")
        return self._h

    def _check(self, rc: int):
        if rc != 0:
            raise Rgbd360Error(f"rgbd360_store call failed ({rc}): {self._L.rgbd360_store_last_error(self._h).decode()}")

    @property
    def entry_bytes(self) -> int:
        return int(self._L.rgbd360_store_entry_bytes(self._handle()))

    def occupied(self, entry: int) -> bool:
        rc = self._L.rgbd360_store_occupied(self._handle(), int(entry))
        if rc < 0:
            raise Rgbd360Error(f"FrameStore: entry {entry} is outside the store (capacity {self.capacity})")
        return bool(rc)

    # ---- frames
    def _entries(self, entries, n_frames):
        e = np.asarray(entries)
        if e.ndim != 1 or e.size != n_frames:
            raise Rgbd360Error("FrameStore.put: one entry per frame")
        if e.size and not np.issubdtype(e.dtype, np.integer):
            raise Rgbd360Error("FrameStore.put: entries must be integers")
        e = np.ascontiguousarray(e, np.int32)
        if e.size and (e.min() < 0 or e.max() >= self.capacity):
            raise Rgbd360Error(f"FrameStore.put: entries must lie in 0..{self.capacity - 1}")
        if len(set(e.tolist())) != e.size:
            raise Rgbd360Error("FrameStore.put: entries must be distinct")
        return e

    def put(self, entries, frames):
        """frames[k] = (rgb HxWx3 uint8, depth HxW uint16 mm | float32 m) -> entry entries[k].  Row-padded arrays travel as they are
        when all frames share the row steps; otherwise they are packed first."""
        frames = list(frames)
        e = self._entries(entries, len(frames))
        if not frames:
            return
        rgbs, deps = [], []
        for f in frames:
            rgb, d = np.asarray(f[0]), np.asarray(f[1])
            if rgb.dtype != np.uint8 or rgb.shape != (self.rows, self.cols, 3):
                raise Rgbd360Error(f"FrameStore.put: imgRGB must be {self.rows}x{self.cols}x3 uint8")
            if d.dtype not in (np.uint16, np.float32):
                raise Rgbd360Error("FrameStore.put: imgDepth must be uint16 millimetres or float32 metres")
            if d.shape != (self.rows, self.cols):
                raise Rgbd360Error(f"FrameStore.put: imgDepth must be {self.rows}x{self.cols}")
            rgbs.append(rgb)
            deps.append(d)
        dtype = deps[0].dtype
        if any(d.dtype != dtype for d in deps):
            raise Rgbd360Error("FrameStore.put: all frames of a call must share one depth type")

        def same_steps(arrs, inner):
            s0 = arrs[0].strides
            return all(a.strides == s0 for a in arrs) and s0[1:] == inner and s0[0] >= inner[0] * self.cols

        if not same_steps(rgbs, (3, 1)):
            rgbs = [np.ascontiguousarray(r) for r in rgbs]
        if not same_steps(deps, (dtype.itemsize,)):
            deps = [np.ascontiguousarray(d) for d in deps]
        rp = (C.c_void_p * len(frames))(*[r.ctypes.data for r in rgbs])
        dp = (C.c_void_p * len(frames))(*[d.ctypes.data for d in deps])
        self._check(self._L.rgbd360_store_put(self._handle(), len(frames), e.ctypes.data_as(C.c_void_p), rp, rgbs[0].strides[0], dp,
                                              deps[0].strides[0], 0 if dtype == np.uint16 else 1, 0))

    def put_dev(self, entries, rgb_ptrs, depth_ptrs, depth_type: int, rgb_step: int = 0, depth_step: int = 0):
        """Frames already in HBM on the store's device: raw device pointers (e.g. torch_tensor.data_ptr()), steps in bytes (0 = packed)."""
        if len(rgb_ptrs) != len(depth_ptrs):
            raise Rgbd360Error("FrameStore.put_dev: rgb_ptrs and depth_ptrs must have the same length")
        if depth_type not in (0, 1):
            raise Rgbd360Error("FrameStore.put_dev: depth_type must be 0 (uint16 mm) or 1 (float32 m)")
        e = self._entries(entries, len(rgb_ptrs))
        if not len(rgb_ptrs):
            return
        rp = (C.c_void_p * len(rgb_ptrs))(*[int(x) for x in rgb_ptrs])
        dp = (C.c_void_p * len(depth_ptrs))(*[int(x) for x in depth_ptrs])
        self._check(self._L.rgbd360_store_put(self._handle(), len(rgb_ptrs), e.ctypes.data_as(C.c_void_p), rp, rgb_step or self.cols * 3, dp,
                                              depth_step or self.cols * (2 if depth_type == 0 else 4), int(depth_type), 1))

    # ---- alignment
    def align(self, pairs, guesses=None, method: int = 0, n_inflight: int = 32, occlusion: int = 0):
        """pairs: [(target entry, source entry), ...]; guesses: None (identity) or one 4x4 per pair.
        Returns (poses [n,4,4] float32, status [n] int32, iters [n, n_pyr] int32, results [n] of _lib.Result), in list order."""
        n_pyr = self._reg.nPyrLevels
        p = np.asarray(pairs)
        if p.size == 0:
            p = np.zeros((0, 2), np.int32)
        if p.ndim != 2 or p.shape[1] != 2:
            raise Rgbd360Error("FrameStore.align: pairs must be (target entry, source entry) tuples")
        if not np.issubdtype(p.dtype, np.integer):
            raise Rgbd360Error("FrameStore.align: entries must be integers")
        n = p.shape[0]
        if n and (p.min() < 0 or p.max() >= self.capacity):
            raise Rgbd360Error(f"FrameStore.align: entries must lie in 0..{self.capacity - 1}")
        if method not in (0, 1, 2):
            raise Rgbd360Error("FrameStore.align: method must be 0, 1 or 2")
        if not 1 <= int(n_inflight) <= 64:
            raise Rgbd360Error("FrameStore.align: n_inflight must be in 1..64")
        g = None
        if guesses is not None:
            G = np.asarray(guesses, np.float32)
            if G.shape != (n, 4, 4):
                raise Rgbd360Error("FrameStore.align: guesses must be one 4x4 pose per pair")
            g = np.ascontiguousarray(np.stack([pose_to_cm(T) for T in G]).reshape(-1)) if n else None
        trg = np.ascontiguousarray(p[:, 0], np.int32)
        src = np.ascontiguousarray(p[:, 1], np.int32)
        out = np.zeros(max(n, 1) * 16, np.float32)
        res = (_lib.Result * max(n, 1))()
        self._check(self._L.rgbd360_store_align(self._handle(), n, trg.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p),
                                                None if g is None else g.ctypes.data_as(C.c_void_p), int(method), int(occlusion),
                                                int(n_inflight), out.ctypes.data_as(C.c_void_p), res))
        poses = np.zeros((n, 4, 4), np.float32)
        status = np.zeros(n, np.int32)
        iters = np.zeros((n, n_pyr), np.int32)
        for k in range(n):
            poses[k] = pose_from_cm(out[16 * k:16 * k + 16])
            status[k] = res[k].status
            iters[k] = [int(res[k].iters[l]) for l in range(n_pyr)]
        return poses, status, iters, [res[k] for k in range(n)]

    # ---- sensed-space overlap (rgbd360_store_overlap*, csrc/store_overlap.h)
    def _overlap_params(self, level, tol_abs, tol_rel):
        p = _lib.OverlapParams()
        self._L.rgbd360_store_overlap_default_params(self._handle(), C.byref(p))
        if level is not None:
            p.level = int(level)
        if tol_abs is not None:
            p.tol_abs = float(tol_abs)
        if tol_rel is not None:
            p.tol_rel = float(tol_rel)
        return p

    def overlap(self, pairs, poses=None, level=None, tol_abs=None, tol_rel=None):
        """pairs: [(target entry, source entry), ...]; poses: None (identity) or one 4x4 (source in target) per pair; level: None = the
        coarsest; tolerances: None = the defaults (0.05 m, 0.02).  Returns a structured array (OVERLAP_DTYPE) in list order."""
        p = np.asarray(pairs)
        if p.size == 0:
            p = np.zeros((0, 2), np.int32)
        if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
            raise Rgbd360Error("FrameStore.overlap: pairs must be (target entry, source entry) integer tuples")
        n = p.shape[0]
        g = None
        if poses is not None:
            G = np.asarray(poses, np.float32)
            if G.shape != (n, 4, 4):
                raise Rgbd360Error("FrameStore.overlap: poses must be one 4x4 pose per pair")
            g = np.ascontiguousarray(G.transpose(0, 2, 1).reshape(-1)) if n else None
        trg = np.ascontiguousarray(p[:, 0], np.int32)
        src = np.ascontiguousarray(p[:, 1], np.int32)
        out = np.zeros(n, OVERLAP_DTYPE)
        par = self._overlap_params(level, tol_abs, tol_rel)
        self._check(self._L.rgbd360_store_overlap(self._handle(), n, trg.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p),
                                                  None if g is None else g.ctypes.data_as(C.c_void_p), C.byref(par),
                                                  out.ctypes.data_as(C.c_void_p)))
        return out

    def overlap_matrix(self, entries, world_poses, max_translation: float = 0.0, level=None, tol_abs=None, tol_rel=None):
        """entries: n distinct occupied entries; world_poses: [n,4,4] (world <- frame).  Returns (matrix [n,n] of OVERLAP_DTYPE with
        matrix[a, b] = target entries[a], source entries[b]; rel_poses [n,n,4,4] float32, W_a^-1 W_b as the library formed them).
        Pairs farther apart than max_translation (> 0) and the diagonal are not evaluated (all zero)."""
        e = np.ascontiguousarray(np.asarray(entries), np.int32)
        n = e.size
        W = np.asarray(world_poses, np.float32)
        if e.ndim != 1 or W.shape != (n, 4, 4):
            raise Rgbd360Error("FrameStore.overlap_matrix: one 4x4 world pose per entry")
        w = np.ascontiguousarray(W.transpose(0, 2, 1).reshape(-1))
        out = np.zeros((n, n), OVERLAP_DTYPE)
        rel = np.zeros((n, n, 16), np.float32)
        par = self._overlap_params(level, tol_abs, tol_rel)
        self._check(self._L.rgbd360_store_overlap_all(self._handle(), n, e.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                                                      float(max_translation), C.byref(par), out.ctypes.data_as(C.c_void_p),
                                                      rel.ctypes.data_as(C.c_void_p)))
        return out, np.ascontiguousarray(rel.reshape(n, n, 4, 4).transpose(0, 1, 3, 2))


OVERLAP_DTYPE = np.dtype([(f, np.int32) for f in _lib.OVERLAP_FIELDS])


def _matrix(m):
    m = np.ascontiguousarray(m, OVERLAP_DTYPE)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise Rgbd360Error("overlap matrix must be [n, n]")
    return m


def overlap_score(matrix, level_px: int) -> np.ndarray:
    """score[a, b] = min(m[a,b].n_consistent, m[b,a].n_consistent) / level_px, 0 unless both directions were evaluated (float32, the
    arithmetic of rgbd360_overlap_candidates)."""
    m = _matrix(matrix)
    both = (m["evaluated"] != 0) & (m["evaluated"].T != 0)
    c = np.minimum(m["n_consistent"], m["n_consistent"].T).astype(np.float32) / np.float32(level_px)
    return np.where(both, c, np.float32(0)).astype(np.float32)


def overlap_candidates(matrix, level_px: int, min_score: float, min_gap: int = 1, max_per_frame: int = 0, known=(), max_out=None):
    """rgbd360_overlap_candidates (host only): (a [k], b [k], score [k], number found); known: [(a, b), ...] edges to leave out."""
    L = _lib.load()
    m = _matrix(matrix)
    n = m.shape[0]
    kn = np.asarray(list(known), np.int32).reshape(-1, 2)
    ka, kb = np.ascontiguousarray(kn[:, 0]), np.ascontiguousarray(kn[:, 1])
    cap = n * (n - 1) // 2 if max_out is None else int(max_out)
    a, b, s = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)
    found = L.rgbd360_overlap_candidates(n, m.ctypes.data_as(C.c_void_p), int(level_px), float(min_score), int(min_gap), int(max_per_frame),
                                         kn.shape[0], ka.ctypes.data_as(C.c_void_p), kb.ctypes.data_as(C.c_void_p), cap,
                                         a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p))
    if found < 0:
        raise Rgbd360Error("rgbd360_overlap_candidates: bad arguments")
    k = min(found, cap)
    return a[:k], b[:k], s[:k], found


def overlap_representative(matrix, level_px: int, subset) -> int:
    """rgbd360_overlap_representative (host only): the member of `subset` with the largest score sum over the subset, ties to the first."""
    L = _lib.load()
    m = _matrix(matrix)
    sub = np.ascontiguousarray(np.asarray(subset), np.int32)
    r = L.rgbd360_overlap_representative(m.shape[0], m.ctypes.data_as(C.c_void_p), int(level_px), sub.ctypes.data_as(C.c_void_p), sub.size)
    if r < 0:
        raise Rgbd360Error("rgbd360_overlap_representative: bad arguments")
    return int(r)
