"""Resident voxel-grid global map: posed frames accumulated into a hash grid in HBM, read out as one point per voxel.

Mirror of rgbd360_map_* (include/rgbd360_hip.h, csrc/voxel_map.h): the map half of the reference's odometry loop
(OdometryRGBD360.cpp:242-268: filterEuclidean, transformPointCloud at currentPose, globalMap +=, filterVoxel):

    gmap = VoxelMap(reg, leaf=0.05, capacity=1 << 20)
    stats = gmap.insert_sphere(rgb, depth, currentPose, convention=0)
    pose, res = gmap.align_sphere(depth, guess, convention=0)      # point-to-point ICP of a frame against the map (csrc/map_align.h)
    pose, res = gmap.align_sphere_plane(depth, guess, convention=0)    # point-to-plane: planes fitted to the centroids (csrc/map_align_plane.h)
    poses, results = gmap.align_batch_cloud([xyz], [(0, g) for g in guesses], method="plane")      # many clouds or guesses in lock step, each
    best = gmap.best_job(results)                                  # job the single call's bytes (csrc/map_align_batch.h); the start of most matches
    pose, res = gmap.align_cloud_gicp(xyz, guess, normals=n)       # generalized ICP: per-match covariance weights (csrc/map_align_gicp.h)
    pose, res = gmap.align_map_gicp(other_map, guess)              # ... of another map's voxels and normals: submap against submap
    depth, rgb, count, key3, stats = gmap.render_sphere(rows, cols, pose)      # the map as a spherical RGB-D frame (csrc/map_render.h)
    depth, rgb, count, key3, stats = gmap.raycast_sphere(rows, cols, pose)     # ... as a per-pixel first hit (csrc/map_raycast.h)
    t, key3, count, rgb, status, stats = gmap.raycast(origins, dirs)           # the first voxel along each ray of a list
    xyz, normal, curvature, status, count, key3, stats = gmap.normals(viewpoint)   # one normal per voxel (csrc/map_normals.h) ...
    xyz, intensity, gradient, status, count, key3, stats = gmap.colours()          # one intensity and tangent gradient per voxel (csrc/map_colour.h)
    pose, res = gmap.align_sphere_colour(rgb, depth, guess)        # coloured ICP: point-to-plane plus photometric (csrc/map_align_colour.h)
    depth, normal, rgb, count, key3, n_on_plane, stats = gmap.raycast_surface_sphere(rows, cols, pose)     # ... and the surface a ray meets
    planes, root_key3, stats = gmap.planes()       # the map segmented into planar regions (csrc/map_planes.h): a PbMap of the map ...
    found = gmap.relocalize(frame_planes)          # ... against which a lost frame is placed without a guess: found["pose"] if status 0
    gmap.observe_sphere(depth, currentPose); gmap.carve()      # the voxels the frame looks straight through leave (csrc/map_carve.h)
    xyz, rgb, count, key = gmap.extract()          # sorted by (i_z, i_y, i_x)
    gmap.remove_sphere(rgb, depth, currentPose)    # exactly undoes that insert (csrc/map_edit.h); gmap.mismatch tells of a broken contract
    gmap.move_sphere(rgb, depth, currentPose, correctedPose)       # a pose-graph correction: removed at the old pose, inserted at the new
    c = gmap.census(); gmap.rehash() if c["n_tombstones"] > c["n_live"] else None      # compaction; rehash(capacity) grows or shrinks
    coarse = gmap.level(2)                         # the map at leaf * 4, merged out of the table (csrc/map_pyramid.h): a read-only VoxelMap
    pose, res = gmap.align_sphere_c2f(depth, guess, convention=0, top_shift=3)     # ICP on levels 3, 2, 1, 0: a basin of 8 leaves
    gmap.merge(submap, pose); gmap.unmerge(submap, pose)       # a submap's voxels added at a pose and taken off again, exactly (csrc/map_merge.h)
    gmap.merge(other)                              # pose None: the union of two maps of one leaf, word for word
    gmap.save(path); copy = VoxelMap.load(reg, path)           # records(): the table's slots as they are; add_records() puts them back

Every point has weight one and the sums are integers: the map does not depend on the order of the frames, and subtracting the same
integer terms takes a frame out again bit for bit.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib, pbmap
from .register import Rgbd360Error, _planes_to_dicts, _ptr, pose_from_cm, pose_to_cm

MAP_FULL = 3      # RGBD360_MAP_FULL
MAP_MISMATCH = 4  # RGBD360_MAP_MISMATCH
RAY_MISS_BOX, RAY_HIT, RAY_LEFT_BOX, RAY_T_MAX, RAY_MAX_STEPS, RAY_BAD = range(6)      # RGBD360_RAY_*
NORMAL_NONE, NORMAL_OK, NORMAL_UNSUPPORTED, NORMAL_NONPLANAR = range(4)                # RGBD360_NORMAL_*
COLOUR_NONE, COLOUR_OK, COLOUR_NO_NORMAL, COLOUR_NO_GRADIENT = range(4)                # RGBD360_COLOUR_*


def _as_dict(st, skip=()):
    """The fields of a ctypes struct by name."""
    return {name: getattr(st, name) for name, _ in st._fields_ if name not in skip}


def check_shift(shift, lowest: int = 1) -> int:
    """A level's shift, lowest .. RGBD360_MAP_MAX_SHIFT, or Rgbd360Error."""
    if isinstance(shift, bool) or int(shift) != shift or not lowest <= int(shift) <= _lib.MAP_MAX_SHIFT:
        raise Rgbd360Error(f"VoxelMap: a shift must be an integer in {lowest} .. {_lib.MAP_MAX_SHIFT}, not {shift!r}")
    return int(shift)


def check_c2f_params(p):
    """What rgbd360_map_align_c2f_* refuses of a MapC2fParams on its own fields, refused here with the field's name."""
    check_shift(p.top_shift, 0)
    if p.kind not in (0, 1):
        raise Rgbd360Error("VoxelMap: kind must be 0 / 'point' or 1 / 'plane'")
    if not 0.0 < p.max_dist_leaves <= 1.0:      # (NaN fails both)
        raise Rgbd360Error("VoxelMap: max_dist_leaves must lie in (0, 1]")
    return p


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
        self.leaf = float(np.float32(leaf))      # as the map holds it (float32)
        self._box = (True, np.array([-2.0, -4.0, -4.0], np.float32), np.array([1.0, 4.0, 4.0], np.float32))      # rgbd360_map_create's default
        self._parent = None      # a level of a pyramid (level()): the map it belongs to
        self._level_gen = 0      # raised when the levels are released: views made before are stale
        self.full = False        # the last insert dropped points of new voxels (RGBD360_MAP_FULL)
        self.mismatch = False    # the last removal was asked for points the map does not hold (RGBD360_MAP_MISMATCH): clear the map

    # ---- lifecycle
    def close(self):
        if self._parent is not None:      # a level goes with its parent
            self._h = None
            return
        self._level_gen += 1
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
        if self._parent is not None and (self._parent._h is None or self._parent._level_gen != self._gen):
            raise Rgbd360Error("VoxelMap: this level's parent was closed or its levels were released")
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
            self._box = (False,) + self._box[1:]
            return
        lo = np.ascontiguousarray(lo, np.float32).reshape(3)
        hi = np.ascontiguousarray(hi, np.float32).reshape(3)
        self._check(self._L.rgbd360_map_set_box(self._handle(), _ptr(lo), _ptr(hi)))
        self._box = (True, lo.copy(), hi.copy())

    @property
    def box(self):
        """(has_box, lo [3] float32, hi [3] float32) as set_box left them (a level: its parent's)."""
        has_box, lo, hi = (self if self._parent is None else self._parent)._box
        return has_box, lo.copy(), hi.copy()

    # ---- insertion
    def _stats(self, rc, st):
        self.last_status = self._check(rc)
        self.full = rc == MAP_FULL
        return _as_dict(st)

    @staticmethod
    def _sphere_args(what, rgb, depth, convention, colour=True):
        """The image arguments of the sphere entries in front of the pose(s) -- without the two of the colour image for the entries that
        take none (colour=False); the arrays they point into come back with them."""
        d = np.asarray(depth)
        if d.dtype not in (np.uint16, np.float32) or d.ndim != 2:
            raise Rgbd360Error(f"VoxelMap.{what}: depth must be HxW uint16 millimetres or float32 metres")
        if d.size and d.strides[1] != d.dtype.itemsize:
            d = np.ascontiguousarray(d)
        c = None
        if rgb is not None:
            c = np.asarray(rgb)
            if c.dtype != np.uint8 or c.shape != d.shape + (3,):
                raise Rgbd360Error(f"VoxelMap.{what}: rgb must be HxWx3 uint8 of the depth image's size")
            if c.size and c.strides[1:] != (3, 1):
                c = np.ascontiguousarray(c)
        args = (None if c is None else _ptr(c), 0 if c is None else c.strides[0], _ptr(d), d.strides[0], 0 if d.dtype == np.uint16 else 1, d.shape[0],
                d.shape[1], int(convention))
        return (args if colour else args[2:]), (d, c)

    @staticmethod
    def _cloud_args(what, xyz, rgb3):
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        c = None
        if rgb3 is not None:
            c = np.ascontiguousarray(rgb3, np.uint8).reshape(-1, 3)
            if c.shape != x.shape:
                raise Rgbd360Error(f"VoxelMap.{what}: one colour per point")
        return (_ptr(x), None if c is None else _ptr(c), x.shape[0]), (x, c)

    def insert_sphere(self, rgb, depth, pose, convention: int = 0):
        """rgb: HxWx3 uint8 or None; depth: HxW uint16 millimetres or float32 metres (rows may be strided); pose: 4x4 world <- frame.
        Returns the call's statistics; self.full tells whether points were dropped."""
        args, keep = self._sphere_args("insert_sphere", rgb, depth, convention)
        p = pose_to_cm(pose)
        st = _lib.MapStats()
        rc = self._L.rgbd360_map_insert_sphere(self._handle(), *args, _ptr(p), 0, C.byref(st))
        return self._stats(rc, st)

    def insert_cloud(self, xyz, rgb3, pose):
        """xyz: n x 3 float32 in the frame's coordinates; rgb3: n x 3 uint8 or None."""
        args, keep = self._cloud_args("insert_cloud", xyz, rgb3)
        p = pose_to_cm(pose)
        st = _lib.MapStats()
        rc = self._L.rgbd360_map_insert_cloud(self._handle(), *args, _ptr(p), 0, C.byref(st))
        return self._stats(rc, st)

    # ---- editing (rgbd360_map_remove_* / _move_* / _rehash / _census, csrc/map_edit.h): what was inserted leaves again, exactly
    def _edit_stats(self, rc, st):
        self.last_status = self._check(rc)
        self.mismatch = rc == MAP_MISMATCH
        return _as_dict(st)

    def remove_sphere(self, rgb, depth, pose, convention: int = 0):
        """Undoes insert_sphere of the same arguments (the same box, a map of the same leaf; that insert must not have been `full`), bit
        for bit and whatever was inserted in between.  Returns the statistics (n_removed, n_missing, n_underflow, n_voxels_emptied,
        ...); self.mismatch tells that points were asked to leave that the map does not hold: its content is then unspecified."""
        args, keep = self._sphere_args("remove_sphere", rgb, depth, convention)
        p = pose_to_cm(pose)
        st = _lib.MapEditStats()
        rc = self._L.rgbd360_map_remove_sphere(self._handle(), *args, _ptr(p), 0, C.byref(st))
        return self._edit_stats(rc, st)

    def remove_cloud(self, xyz, rgb3, pose):
        """Undoes insert_cloud of the same arguments."""
        args, keep = self._cloud_args("remove_cloud", xyz, rgb3)
        p = pose_to_cm(pose)
        st = _lib.MapEditStats()
        rc = self._L.rgbd360_map_remove_cloud(self._handle(), *args, _ptr(p), 0, C.byref(st))
        return self._edit_stats(rc, st)

    def _move_stats(self, rc, est, st):
        removed = self._edit_stats(rc, est)
        self.mismatch = est.n_missing != 0 or est.n_underflow != 0
        self.full = st.n_dropped_full != 0
        return removed, _as_dict(st)

    def move_sphere(self, rgb, depth, pose_old, pose_new, convention: int = 0):
        """The frame inserted at pose_old moves to pose_new: removed and inserted over one upload.  Returns (removal statistics, insert
        statistics); self.mismatch and self.full as after remove_sphere and insert_sphere (the insertion happens either way)."""
        args, keep = self._sphere_args("move_sphere", rgb, depth, convention)
        a, b = pose_to_cm(pose_old), pose_to_cm(pose_new)
        est, st = _lib.MapEditStats(), _lib.MapStats()
        rc = self._L.rgbd360_map_move_sphere(self._handle(), *args, _ptr(a), _ptr(b), 0, C.byref(est), C.byref(st))
        return self._move_stats(rc, est, st)

    def move_cloud(self, xyz, rgb3, pose_old, pose_new):
        args, keep = self._cloud_args("move_cloud", xyz, rgb3)
        a, b = pose_to_cm(pose_old), pose_to_cm(pose_new)
        est, st = _lib.MapEditStats(), _lib.MapStats()
        rc = self._L.rgbd360_map_move_cloud(self._handle(), *args, _ptr(a), _ptr(b), 0, C.byref(est), C.byref(st))
        return self._move_stats(rc, est, st)

    def rehash(self, capacity: int = 0):
        """The table rebuilt without tombstones into `capacity` voxels (a power of two above it; 0: the current size).  Returns the status:
        0, or MAP_FULL when a voxel found no slot in the new table (the map is unchanged); a capacity below len(self) raises."""
        return self._check(self._L.rgbd360_map_rehash(self._handle(), int(capacity)))

    def census(self):
        """{n_slots, n_live, n_tombstones, n_points, n_inconsistent} of a read-only scan of the table."""
        c = _lib.MapCensus()
        self._check(self._L.rgbd360_map_census(self._handle(), C.byref(c)))
        return _as_dict(c)

    # ---- alignment of a frame against the map (rgbd360_map_align_*; the reference's cloud ICP, OdometryRGBD360.cpp:98-114, 210-222)
    def _params(self, struct_type, default_fn, **fields):
        """The defaults of a parameter struct with the given fields replaced (None: the default stays)."""
        p = struct_type()
        default_fn(self._handle(), C.byref(p))
        for name, v in fields.items():
            if not hasattr(p, name):
                raise TypeError(f"{struct_type.__name__} has no field {name!r}")
            if v is not None:
                setattr(p, name, v)
        return p

    def align_params(self, max_dist=None, max_iters=None, eps=None, min_count=None, min_matches=None):
        """The defaults (max_dist = leaf, 10 iterations, eps 1e-6, min_count 1, min_matches 6) with the given fields replaced."""
        return self._params(_lib.MapAlignParams, self._L.rgbd360_map_default_align_params, max_dist=max_dist, max_iters=max_iters, eps=eps,
                            min_count=min_count, min_matches=min_matches)

    def _align(self, entry, result_type, params, input_args, guess):
        """One rgbd360_map_align_* call on a host input: (pose 4x4, the result struct as a dict)."""
        g = pose_to_cm(guess)
        out = np.zeros(16, np.float32)
        res = result_type()
        self._check(entry(self._handle(), *input_args, _ptr(g), 0, C.byref(params), _ptr(out), C.byref(res)))
        r = _as_dict(res, skip=("hessian", "gradient"))
        r["hessian"] = np.array(res.hessian, np.float32).reshape(6, 6).T.copy()
        r["gradient"] = np.array(res.gradient, np.float32)
        return pose_from_cm(out), r

    def align_sphere(self, depth, guess, convention: int = 0, **params):
        """Point-to-point ICP of the sphere frame `depth` (as in insert_sphere) against the map from `guess` (4x4 world <- frame); the
        nearest neighbour is the nearest voxel centroid within max_dist <= leaf.  Returns (pose 4x4, result dict with status,
        iterations, converged, the counters, n_matched, fitness, hessian, gradient).  The map is not changed."""
        args, keep = self._sphere_args("align_sphere", None, depth, convention, colour=False)
        return self._align(self._L.rgbd360_map_align_sphere, _lib.MapAlignResult, self.align_params(**params), args, guess)

    def align_cloud(self, xyz, guess, **params):
        """The same for a cloud xyz: n x 3 float32 in the frame's coordinates."""
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        return self._align(self._L.rgbd360_map_align_cloud, _lib.MapAlignResult, self.align_params(**params), (_ptr(x), x.shape[0]), guess)

    # ---- point-to-plane (rgbd360_map_align_plane_*: the same matches, the residual along the normal of a plane fitted to the centroids
    #      of the occupied cells around the point; the plane cost of the reference's GICP call sites)
    def align_plane_params(self, max_dist=None, max_iters=None, eps=None, min_count=None, min_matches=None, min_support=None, max_flatness=None):
        """align_params' defaults, min_support = 5 and max_flatness = 0.05, with the given fields replaced."""
        return self._params(_lib.MapAlignPlaneParams, self._L.rgbd360_map_default_align_plane_params, max_dist=max_dist, max_iters=max_iters, eps=eps,
                            min_count=min_count, min_matches=min_matches, min_support=min_support, max_flatness=max_flatness)

    def align_sphere_plane(self, depth, guess, convention: int = 0, **params):
        """Point-to-plane ICP of the sphere frame `depth` against the map from `guess`: align_sphere's matches, each with the plane fitted
        to the centroids of the occupied cells around the point.  Returns (pose 4x4, result dict: align_sphere's fields -- n_matched counts
        the contributing points, fitness is the mean squared plane distance -- plus n_unsupported, n_nonplanar and fitness_point, the
        point-to-point fitness of the same matches).  The map is not changed."""
        args, keep = self._sphere_args("align_sphere_plane", None, depth, convention, colour=False)
        return self._align(self._L.rgbd360_map_align_plane_sphere, _lib.MapAlignPlaneResult, self.align_plane_params(**params), args, guess)

    def align_cloud_plane(self, xyz, guess, **params):
        """The same for a cloud xyz: n x 3 float32 in the frame's coordinates."""
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        return self._align(self._L.rgbd360_map_align_plane_cloud, _lib.MapAlignPlaneResult, self.align_plane_params(**params), (_ptr(x), x.shape[0]), guess)

    # ---- generalized ICP (rgbd360_map_align_gicp_*: the same matches, each weighted by (C_B + C_A)^-1 with the target's covariance from the
    #      matched voxel's resident normal and the source's from a normal per point; the cost of the reference's GICP call sites)
    def align_gicp_params(self, max_dist=None, max_iters=None, eps=None, min_count=None, min_matches=None, epsilon=None, use_target_normals=None,
                          min_support=None, max_flatness=None):
        """align_params' defaults, epsilon = 1e-3, use_target_normals = 1, min_support = 5 and max_flatness = 0.05, with the given fields
        replaced."""
        use_target_normals = None if use_target_normals is None else int(use_target_normals)
        return self._params(_lib.MapAlignGicpParams, self._L.rgbd360_map_default_align_gicp_params, max_dist=max_dist, max_iters=max_iters, eps=eps,
                            min_count=min_count, min_matches=min_matches, epsilon=epsilon, use_target_normals=use_target_normals,
                            min_support=min_support, max_flatness=max_flatness)

    def align_cloud_gicp(self, xyz, guess, normals=None, **params):
        """Generalized ICP of the cloud xyz (n x 3 float32 in the frame's coordinates) against the map from `guess`: align_cloud's matches,
        each weighted by the inverse of the sum of the two sides' covariances -- the map's per-voxel normals (normals()) on the target side,
        `normals` (n x 3 float32 in the frame's coordinates; a zero or non-finite row: none for that point; None: none at all) on the source
        side.  Returns (pose 4x4, result dict: align_cloud's fields -- fitness is the mean weighted cost -- plus n_target_planes,
        n_source_planes, n_plane_pairs and fitness_point).  The map is not changed."""
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            if nrm.shape != x.shape:
                raise Rgbd360Error("VoxelMap.align_cloud_gicp: one normal per point")
        args = (_ptr(x), None if nrm is None else _ptr(nrm), x.shape[0])
        return self._align(self._L.rgbd360_map_align_gicp_cloud, _lib.MapAlignGicpResult, self.align_gicp_params(**params), args, guess)

    def align_sphere_gicp(self, depth, guess, convention: int = 0, **params):
        """The same for the sphere frame `depth`, which has no source normals: point-to-plane on the map's resident normals, weight
        1 / epsilon along a voxel's normal and 1 across it, point-to-point where the matched voxel has none."""
        args, keep = self._sphere_args("align_sphere_gicp", None, depth, convention, colour=False)
        return self._align(self._L.rgbd360_map_align_gicp_sphere, _lib.MapAlignGicpResult, self.align_gicp_params(**params), args, guess)

    def gicp_source(self, **normal_params):
        """This map as the source of another map's align_map_gicp: (xyz, normals), its voxels' centroids and normals (zero where a voxel has
        none) ordered by (i_z, i_y, i_x), so that the sums of an alignment are the same from run to run."""
        xyz, normal, _, _, _, key3, _ = self.normals(**normal_params)
        order = np.lexsort((key3[:, 0], key3[:, 1], key3[:, 2]))
        return np.ascontiguousarray(xyz[order]), np.ascontiguousarray(normal[order])

    def align_map_gicp(self, source_map, guess, **params):
        """Plane-to-plane ICP of another VoxelMap against this one from `guess` (4x4, this map's world <- the source map's world): the
        source's voxels (source_map.gicp_source(), its normals fitted under this call's min_count, min_support and max_flatness) through
        align_cloud_gicp.  "Voxel-filter both clouds, then GICP", and the alignment of two submaps of a loop closure.  As for any cloud, this
        map's box applies to the source's centroids in the source's own coordinates; set_box(None, None) where that is not wanted."""
        fit = {k: params[k] for k in ("min_count", "min_support", "max_flatness") if params.get(k) is not None}
        xyz, normal = source_map.gicp_source(**fit)
        return self.align_cloud_gicp(xyz, guess, normals=normal, **params)

    # ---- coloured ICP (rgbd360_map_align_colour_*: the same matches, point-to-plane on the map's resident normals joined with a photometric
    #      term on its resident intensity gradients, colours(); csrc/map_align_colour.h)
    def align_colour_params(self, max_dist=None, max_iters=None, eps=None, min_count=None, min_matches=None, lambda_geometric=None, min_support=None,
                            max_flatness=None, min_gradient_support=None, min_spread=None):
        """align_plane_params' defaults, lambda_geometric = 0.968, min_gradient_support = 4 and min_spread = 0.01, with the given fields
        replaced.  A lambda_geometric outside [0, 1] and supports outside their ranges raise here."""
        if lambda_geometric is not None and not 0.0 <= float(lambda_geometric) <= 1.0:
            raise Rgbd360Error("VoxelMap.align_colour_params: lambda_geometric must lie in [0, 1]")
        if min_support is not None and not 1 <= int(min_support) <= 27:
            raise Rgbd360Error("VoxelMap.align_colour_params: min_support must lie in 1 .. 27")
        if min_gradient_support is not None and not 1 <= int(min_gradient_support) <= 26:
            raise Rgbd360Error("VoxelMap.align_colour_params: min_gradient_support must lie in 1 .. 26")
        return self._params(_lib.MapAlignColourParams, self._L.rgbd360_map_default_align_colour_params, max_dist=max_dist, max_iters=max_iters, eps=eps,
                            min_count=min_count, min_matches=min_matches, lambda_geometric=lambda_geometric, min_support=min_support,
                            max_flatness=max_flatness, min_gradient_support=min_gradient_support, min_spread=min_spread)

    def align_cloud_colour(self, xyz, rgb3, guess, **params):
        """Coloured ICP of the cloud xyz (n x 3 float32 in the frame's coordinates) with its colours rgb3 (n x 3 uint8, required) against the
        map from `guess`: align_cloud's matches, the point-to-plane residual along the matched voxel's resident normal weighted
        lambda_geometric, and the difference between the map's intensity, carried along its tangent-plane gradient to the point, and the
        point's own, weighted 1 - lambda_geometric.  Returns (pose 4x4, result dict: align_cloud's fields -- fitness is the mean joint cost
        -- plus n_no_normal, n_no_gradient, rms_geometric and rms_colour).  The map, which must have been fed with colours, is not changed."""
        if rgb3 is None:
            raise Rgbd360Error("VoxelMap.align_cloud_colour: the cloud's colours are required")
        args, keep = self._cloud_args("align_cloud_colour", xyz, rgb3)
        p = self.align_colour_params(**params)
        return self._align(self._L.rgbd360_map_align_colour_cloud, _lib.MapAlignColourResult, p, args, guess)

    def align_sphere_colour(self, rgb, depth, guess, convention: int = 0, **params):
        """The same for the sphere frame (rgb, depth) as insert_sphere takes it; rgb is required."""
        if rgb is None:
            raise Rgbd360Error("VoxelMap.align_sphere_colour: the frame's colour image is required")
        args, keep = self._sphere_args("align_sphere_colour", rgb, depth, convention)
        p = self.align_colour_params(**params)
        return self._align(self._L.rgbd360_map_align_colour_sphere, _lib.MapAlignColourResult, p, args, guess)

    # ---- robust kernels of the alignments (rgbd360_map_set_align_robust; csrc/map_align_robust.h): a setting of the map per method
    METHODS = {"point": _lib.MAP_METHOD_POINT, "plane": _lib.MAP_METHOD_PLANE, "gicp": _lib.MAP_METHOD_GICP, "colour": _lib.MAP_METHOD_COLOUR}
    ROBUST_KINDS = {"none": _lib.MAP_ROBUST_NONE, "huber": _lib.MAP_ROBUST_HUBER, "cauchy": _lib.MAP_ROBUST_CAUCHY,
                    "geman_mcclure": _lib.MAP_ROBUST_GEMAN_MCCLURE}

    def set_align_robust(self, method, kind, delta: float = 0.0, scale_with_level: bool = False):
        """The robust kernel of `method` ("point", "plane", "gicp", "colour" or RGBD360_MAP_METHOD_*) from now on: kind "none", "huber",
        "cauchy" or "geman_mcclure" (or RGBD360_MAP_ROBUST_*), delta > 0 in the units of the square root of the method's cost term (metres
        for point and plane); scale_with_level: delta x 2^shift on level `shift` of the pyramid.  Every align_* call of the method,
        align_batch_* and align_*_c2f honour it; with "none" they are the quadratic calls.  The map's content is not touched."""
        r = _lib.MapRobust(int(self.ROBUST_KINDS.get(kind, kind)), 1 if scale_with_level else 0, float(delta))
        self._check(self._L.rgbd360_map_set_align_robust(self._handle(), int(self.METHODS.get(method, method)), C.byref(r)))

    def align_robust(self, method):
        """The setting of `method`: dict(kind, scale_with_level, delta)."""
        r = _lib.MapRobust()
        self._check(self._L.rgbd360_map_get_align_robust(self._handle(), int(self.METHODS.get(method, method)), C.byref(r)))
        return _as_dict(r)

    def robust_info(self, job=None):
        """What the last single alignment did with its robust kernel (job None), or job `job` of the last batch: dict(method, kind, delta_eff,
        sum_w, n, n_downweighted)."""
        info = _lib.MapRobustInfo()
        if job is None:
            self._check(self._L.rgbd360_map_align_robust_info(self._handle(), C.byref(info)))
        else:
            self._check(self._L.rgbd360_map_align_batch_robust_info(self._handle(), int(job), C.byref(info)))
        return _as_dict(info)

    def align_trace(self):
        """One record per step of the last align call of either kind: (n, sum_sq, update[6]) (rgbd360_map_align_eval, the diagnostics header)."""
        n = C.c_int()
        self._check(self._L.rgbd360_map_align_eval(self._handle(), None, 0, 0, 0, 0, 0, None, 0, None, 0, None, None, None, None, None, 0, C.byref(n), None))
        tr = (_lib.MapAlignTrace * max(n.value, 1))()
        self._check(self._L.rgbd360_map_align_eval(self._handle(), None, 0, 0, 0, 0, 0, None, 0, None, 0, None, None, None, None, None, n.value, None, tr))
        return [(int(t.n), float(t.sum_sq), np.array(t.update, np.float32)) for t in tr[:n.value]]

    # ---- many alignments in lock step (rgbd360_map_align_batch_* / rgbd360_map_align_plane_batch_*; csrc/map_align_batch.h): every job is the
    #      single call of its input from its guess, byte for byte; 2 max_iters + 3 launches and one synchronisation for the whole batch
    def _align_batch(self, form, method, inputs, geometry, jobs, params):
        if method not in ("point", "plane"):
            raise Rgbd360Error("VoxelMap.align_batch_*: method must be 'point' or 'plane'")
        plane = method == "plane"
        p = (self.align_plane_params if plane else self.align_params)(**params)
        jobs = list(jobs)
        if not 1 <= len(jobs) <= _lib.MAP_BATCH_MAX or not 1 <= len(inputs) <= _lib.MAP_BATCH_MAX:
            raise Rgbd360Error(f"VoxelMap.align_batch_{form}: 1 .. {_lib.MAP_BATCH_MAX} inputs and jobs")
        J = (_lib.MapBatchJob * len(jobs))()
        for k, (i, guess) in enumerate(jobs):
            J[k].input = int(i)
            J[k].guess[:] = pose_to_cm(guess).tolist()
        poses = np.zeros((len(jobs), 16), np.float32)
        res = ((_lib.MapAlignPlaneResult if plane else _lib.MapAlignResult) * len(jobs))()
        entry = getattr(self._L, ("rgbd360_map_align_plane_batch_" if plane else "rgbd360_map_align_batch_") + form)
        self._check(entry(self._handle(), inputs, len(inputs), *geometry, 0, J, len(jobs), C.byref(p), _ptr(poses), res))
        out = []
        for r in res:
            d = _as_dict(r, skip=("hessian", "gradient"))
            d["hessian"] = np.array(r.hessian, np.float32).reshape(6, 6).T.copy()
            d["gradient"] = np.array(r.gradient, np.float32)
            out.append(d)
        return np.stack([pose_from_cm(q) for q in poses]), out

    def align_batch_cloud(self, clouds, jobs, method: str = "point", **params):
        """Many alignments of clouds against the map in lock step.  clouds: a list of n x 3 float32 arrays in their frames' coordinates;
        jobs: a list of (index into clouds, guess 4x4); method: "point" (align_cloud) or "plane" (align_cloud_plane); params: the method's,
        one set for all jobs.  Returns (poses [n_jobs, 4, 4], a list of result dicts): per job exactly what the single call returns.  A job
        that ends early stops, the others go on; the map is not changed.  align_batch_trace(j) gives a job's trace, best_job a winner."""
        xs = [np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in clouds]
        I = (_lib.MapBatchCloud * max(len(xs), 1))()
        for k, x in enumerate(xs):
            I[k].xyz, I[k].n = x.ctypes.data, x.shape[0]
        return self._align_batch("cloud", method, I if xs else [], (), jobs, params)

    def align_batch_sphere(self, depths, jobs, convention: int = 0, method: str = "point", **params):
        """The same for sphere frames: depths, a list of HxW depth images of ONE size and type (uint16 millimetres or float32 metres; rows may
        be strided); jobs: (index into depths, guess 4x4)."""
        ds = []
        for depth in depths:
            d = np.asarray(depth)
            if d.dtype not in (np.uint16, np.float32) or d.ndim != 2:
                raise Rgbd360Error("VoxelMap.align_batch_sphere: depth must be HxW uint16 millimetres or float32 metres")
            if d.size and d.strides[1] != d.dtype.itemsize:
                d = np.ascontiguousarray(d)
            if ds and (d.shape != ds[0].shape or d.dtype != ds[0].dtype):
                raise Rgbd360Error("VoxelMap.align_batch_sphere: the frames of a batch share one size and depth type")
            ds.append(d)
        I = (_lib.MapBatchFrame * max(len(ds), 1))()
        for k, d in enumerate(ds):
            I[k].depth, I[k].depth_step = d.ctypes.data, d.strides[0]
        geometry = (0 if ds[0].dtype == np.uint16 else 1, ds[0].shape[0], ds[0].shape[1], int(convention)) if ds else (0, 0, 0, int(convention))
        return self._align_batch("sphere", method, I if ds else [], geometry, jobs, params)

    def align_batch_trace(self, job: int):
        """One record per step of job `job` of the last align_batch_* call: (n, sum_sq, update[6]), as align_trace after the single call."""
        n = C.c_int()
        self._check(self._L.rgbd360_map_align_batch_trace(self._handle(), int(job), 0, C.byref(n), None))
        tr = (_lib.MapAlignTrace * max(n.value, 1))()
        self._check(self._L.rgbd360_map_align_batch_trace(self._handle(), int(job), n.value, None, tr))
        return [(int(t.n), float(t.sum_sq), np.array(t.update, np.float32)) for t in tr[:n.value]]

    def best_job(self, results, min_matched: int = 0) -> int:
        """The winner among the result dicts of align_batch_* (rgbd360_map_align_best): status OK and n_matched >= min_matched; the largest
        n_matched, then the smaller fitness, then the smaller index; -1 when there is none.  A policy for the jobs of ONE input from several
        guesses (an inlier count), not part of the alignment."""
        results = list(results)
        plane = bool(results) and "fitness_point" in results[0]
        R = ((_lib.MapAlignPlaneResult if plane else _lib.MapAlignResult) * max(len(results), 1))()
        for k, r in enumerate(results):
            R[k].status, R[k].n_matched, R[k].fitness = int(r["status"]), int(r["n_matched"]), float(r["fitness"])
        return int((self._L.rgbd360_map_align_plane_best if plane else self._L.rgbd360_map_align_best)(R, len(results), int(min_matched)))

    # ---- the rig's extrinsics against the map (rgbd360_map_calibrate_rig_*; csrc/rig_calib.h): K frames x S sensors, one unknown per free
    #      sensor shared over all frames and, with refine_poses, one per frame; 4 max_iters + 5 launches and one synchronisation
    def rig_calib_params(self, refine_poses=None, fixed_sensor=None, lambda_=None, min_input_matches=None, **plane):
        """The defaults (the point-to-plane ones, refine_poses 0, fixed_sensor -1, lambda 0, min_input_matches 6) with the given fields replaced."""
        p = _lib.RigCalibParams()
        self._L.rgbd360_map_default_rig_calib_params(self._handle(), C.byref(p))
        p.plane = self.align_plane_params(**plane)
        for name, value in (("refine_poses", refine_poses), ("fixed_sensor", fixed_sensor), ("lambda_", lambda_), ("min_input_matches", min_input_matches)):
            if value is not None:
                setattr(p, name, value)
        return p

    def _calibrate_rig(self, entry, head, poses, extrinsics, params):
        T = np.stack([pose_to_cm(P) for P in poses]).astype(np.float32)
        E = np.stack([pose_to_cm(P) for P in extrinsics]).astype(np.float32)
        K, S = len(T), len(E)
        p = self.rig_calib_params(**params)
        res = _lib.RigCalibResult()
        sen = (_lib.RigCalibSensor * S)()
        self._check(entry(self._handle(), *head, K, S, 0, _ptr(T), _ptr(E), C.byref(p), C.byref(res), sen))
        sensors = []
        for r in sen:
            sensors.append({"n_matched": int(r.n_matched), "cost": float(r.cost), "hessian": np.array(r.hessian, np.float32).reshape(6, 6).T.copy(),
                            "gradient": np.array(r.gradient, np.float32)})
        return np.stack([pose_from_cm(q) for q in T]), np.stack([pose_from_cm(q) for q in E]), dict(_as_dict(res), sensors=sensors)

    def calibrate_rig_clouds(self, clouds, poses, extrinsics, **params):
        """The rig's extrinsics against the map.  clouds: K x S arrays (n x 3 float32, the cloud of sensor s in frame k in the sensor's
        coordinates; an empty array: no data), as a list of K lists of S or a flat frame-major list; poses: K world <- rig 4x4; extrinsics: S
        rig <- sensor 4x4; params: rig_calib_params' (refine_poses needs a fixed_sensor).  Returns (poses, extrinsics, result dict with the
        per-sensor records under "sensors").  The map is not changed."""
        flat = [x for row in clouds for x in row] if len(clouds) and isinstance(clouds[0], (list, tuple)) else list(clouds)
        if len(flat) != len(poses) * len(extrinsics):
            raise Rgbd360Error("VoxelMap.calibrate_rig_clouds: one cloud per frame and sensor")
        xs = [np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in flat]
        I = (_lib.MapBatchCloud * max(len(xs), 1))()
        for k, x in enumerate(xs):
            I[k].xyz, I[k].n = x.ctypes.data, x.shape[0]
        return self._calibrate_rig(self._L.rgbd360_map_calibrate_rig_clouds, (I,), poses, extrinsics, params)

    def calibrate_rig_depth(self, depths, K4, poses, extrinsics, models=None, **params):
        """The same from K x S pinhole depth images of ONE size and type (uint16 millimetres or float32 metres; rows may be strided), flat
        frame-major; K4 = (fx, fy, cx, cy).  models: a depth_train.DepthModels of the S sensors; every image is corrected by its sensor's
        model on the device before its cloud is formed (rgbd360_map_calibrate_rig_depth_models)."""
        ds = []
        for depth in depths:
            d = np.asarray(depth)
            if d.dtype not in (np.uint16, np.float32) or d.ndim != 2:
                raise Rgbd360Error("VoxelMap.calibrate_rig_depth: depth must be HxW uint16 millimetres or float32 metres")
            if d.size and d.strides[1] != d.dtype.itemsize:
                d = np.ascontiguousarray(d)
            if ds and (d.shape != ds[0].shape or d.dtype != ds[0].dtype):
                raise Rgbd360Error("VoxelMap.calibrate_rig_depth: the images of a call share one size and depth type")
            ds.append(d)
        if not ds or len(ds) != len(poses) * len(extrinsics):
            raise Rgbd360Error("VoxelMap.calibrate_rig_depth: one image per frame and sensor")
        I = (_lib.MapBatchFrame * len(ds))()
        for k, d in enumerate(ds):
            I[k].depth, I[k].depth_step = d.ctypes.data, d.strides[0]
        fx, fy, cx, cy = (float(v) for v in K4)
        head = (I, 0 if ds[0].dtype == np.uint16 else 1, ds[0].shape[0], ds[0].shape[1], fx, fy, cx, cy)
        if models is not None:
            return self._calibrate_rig(self._L.rgbd360_map_calibrate_rig_depth_models, (models._handle(),) + head, poses, extrinsics, params)
        return self._calibrate_rig(self._L.rgbd360_map_calibrate_rig_depth, head, poses, extrinsics, params)

    def rig_calib_trace(self):
        """One record per step of the last calibrate_rig_* call: (n, cost, largest v.v, largest w.w over the blocks' updates)."""
        n = C.c_int()
        self._check(self._L.rgbd360_rig_calib_trace(self._handle(), 0, C.byref(n), None))
        tr = (_lib.RigCalibStep * max(n.value, 1))()
        self._check(self._L.rgbd360_rig_calib_trace(self._handle(), n.value, None, tr))
        return [(int(t.n), float(t.cost), float(t.max_vv), float(t.max_ww)) for t in tr[:n.value]]

    # ---- the map pyramid and coarse-to-fine ICP (rgbd360_map_level, rgbd360_map_align_c2f_*; csrc/map_pyramid.h): level s is the map of
    #      leaf * 2^s merged out of this table by index >> s, exact; the chain aligns on levels top_shift .. 0, each from the pose before
    def level(self, shift: int) -> "VoxelMap":
        """Level `shift` (1 .. 6) of this map as a non-owning, read-only VoxelMap: levels 1 .. shift are built or refreshed now and keep
        that content until the next level() / align_*_c2f call.  Readers work on it (len, extract, census, align_*, render_sphere,
        raycast*, normals); writers raise.  It is valid until the parent is closed or release_levels() is called.  A build that drops a
        voxel (RGBD360_MAP_FULL: no free slot within the probe bound of the level's table) raises; the parent is unchanged."""
        shift = check_shift(shift)
        if self._parent is not None:
            raise Rgbd360Error("VoxelMap.level: a level has no levels of its own")
        h = C.c_void_p()
        rc = self._L.rgbd360_map_level(self._handle(), shift, C.byref(h))
        if rc != 0:      # a failed build took the levels from the failing one up with it: views made before are stale
            self._level_gen += 1
        self.last_status = self._check(rc)
        if rc == MAP_FULL:
            raise Rgbd360Error(f"rgbd360_map_level failed ({rc}, MAP_FULL): {self._L.rgbd360_map_last_error(self._h).decode()}")
        view = VoxelMap.__new__(VoxelMap)
        view._L, view._reg, view._h, view._ctx_value = self._L, self._reg, h, self._ctx_value
        view._parent, view._gen, view._level_gen = self, self._level_gen, 0
        view.full = view.mismatch = False
        view.shift = shift
        view.leaf = float(np.float32(self.leaf) * np.float32(2.0 ** shift))
        return view

    @property
    def pyramid_bytes(self) -> int:
        """Device memory of the levels' tables (`bytes` stays the table of this map alone)."""
        return int(self._L.rgbd360_map_pyramid_bytes(self._handle()))

    def release_levels(self):
        """Frees every level; views handed out by level() become unusable."""
        self._check(self._L.rgbd360_map_release_levels(self._handle()))
        self._level_gen += 1

    def c2f_params(self, top_shift=None, kind=None, max_iters=None, eps=None, min_count=None, min_matches=None, max_dist_leaves=None,
                   min_support=None, max_flatness=None):
        """The defaults (top_shift 3, kind 0 = point-to-point, max_dist_leaves 1, the single-level defaults for the rest) with the given
        fields replaced.  kind: 0 / 1 or "point" / "plane"."""
        kind = {"point": 0, "plane": 1}.get(kind, kind)
        p = self._params(_lib.MapC2fParams, self._L.rgbd360_map_default_c2f_params, top_shift=top_shift, kind=kind, max_iters=max_iters, eps=eps,
                         min_count=min_count, min_matches=min_matches, max_dist_leaves=max_dist_leaves, min_support=min_support,
                         max_flatness=max_flatness)
        return check_c2f_params(p)

    def _align_c2f(self, entry, params, input_args, guess):
        g = pose_to_cm(guess)
        out = np.zeros(16, np.float32)
        res = _lib.MapC2fResult()
        rc = self._check(entry(self._handle(), *input_args, _ptr(g), 0, C.byref(params), _ptr(out), C.byref(res)))
        if rc == MAP_FULL:       # a level could not be built (level()): nothing was aligned, and views of the levels are stale
            self._level_gen += 1
            raise Rgbd360Error(f"rgbd360_map_align_c2f failed ({rc}, MAP_FULL): {self._L.rgbd360_map_last_error(self._h).decode()}")
        levels = []
        for lv in res.levels[:res.n_levels]:
            d = _as_dict(lv, skip=("pose",))
            d["pose"] = pose_from_cm(np.array(lv.pose, np.float32))
            levels.append(d)
        r = dict(levels[-1], levels=levels, n_levels=int(res.n_levels)) if levels else dict(levels=levels, n_levels=0)
        r["hessian"] = np.array(res.hessian, np.float32).reshape(6, 6).T.copy()
        r["gradient"] = np.array(res.gradient, np.float32)
        return pose_from_cm(out), r

    def align_sphere_c2f(self, depth, guess, convention: int = 0, **params):
        """Coarse-to-fine ICP of the sphere frame `depth` from `guess`: align_sphere (kind 0) or align_sphere_plane (kind 1) on levels
        top_shift .. 0, each with max_dist = max_dist_leaves x its leaf and from the pose the level before ended on (a level that does not
        end OK hands on the pose it was given).  Returns (pose 4x4, result dict: level 0's status, iterations, converged, counters,
        n_matched, fitness, hessian, gradient, and `levels`, one dict per level from the coarsest down with shift, those fields and the
        pose it ended on).  Neither the map nor its levels' tables are written."""
        args, keep = self._sphere_args("align_sphere_c2f", None, depth, convention, colour=False)
        return self._align_c2f(self._L.rgbd360_map_align_c2f_sphere, self.c2f_params(**params), args, guess)

    def align_cloud_c2f(self, xyz, guess, **params):
        """The same for a cloud xyz: n x 3 float32 in the frame's coordinates."""
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        return self._align_c2f(self._L.rgbd360_map_align_c2f_cloud, self.c2f_params(**params), (_ptr(x), x.shape[0]), guess)

    # ---- composing maps (rgbd360_map_merge / _unmerge / _records / _add_records; csrc/map_merge.h): voxel records moved between tables --
    #      a submap merged into a global map at a pose and taken out again exactly, a map copied, saved and loaded with its bits intact
    def merge_params(self, min_count=None):
        """The default (min_count 1) with the given field replaced."""
        return self._params(_lib.MapMergeParams, self._L.rgbd360_map_default_merge_params, min_count=min_count)

    def _merge(self, entry, source, pose, params):
        if not isinstance(source, VoxelMap):
            raise Rgbd360Error("VoxelMap.merge / unmerge: the source must be a VoxelMap")
        p = self.merge_params(**params)
        g = None if pose is None else pose_to_cm(pose)
        st = _lib.MapMergeStats()
        rc = entry(self._handle(), source._handle(), None if g is None else _ptr(g), C.byref(p), C.byref(st))
        self.last_status = self._check(rc)
        return rc, _as_dict(st)

    def merge(self, source, pose=None, **params):
        """The live voxels of `source` (another VoxelMap, or a level of one) added to this map.  pose None: sum mode -- equal leaves, the
        keys kept, the seven words added: this map becomes the map that received both maps' insertions, bit for bit.  pose 4x4 (this
        map's world <- the source's world): each source voxel enters as its count of coincident points at its posed centroid, its colour
        sums kept; the leaves may differ.  Returns the statistics; self.full tells whether new voxels were dropped."""
        rc, st = self._merge(self._L.rgbd360_map_merge, source, pose, params)
        self.full = rc == MAP_FULL
        return st

    def unmerge(self, source, pose=None, **params):
        """Undoes merge(source, pose, **params) of the same, unchanged source (that merge must not have been `full`), bit for bit and
        whatever was inserted in between; emptied voxels stay as tombstones (rehash()).  Returns the statistics (n_voxels_new: voxels
        emptied); self.mismatch tells that voxels were asked to leave that the map does not hold: its content is then unspecified."""
        rc, st = self._merge(self._L.rgbd360_map_unmerge, source, pose, params)
        self.mismatch = rc == MAP_MISMATCH
        return st

    def records(self, max_out=None):
        """The live slots as they are: uint64 [k, 8] = (key, count, Sx, Sy, Sz, Sr, Sg, Sb) per voxel (the sums in two's complement), ascending
        key = ascending (i_z, i_y, i_x), k = min(len, max_out)."""
        n = len(self)
        k = n if max_out is None else min(n, int(max_out))
        rec = np.zeros((k, 8), np.uint64)
        got = self._L.rgbd360_map_records(self._handle(), k, _ptr(rec))
        if got != n:
            raise Rgbd360Error(f"rgbd360_map_records failed ({got}): {self._L.rgbd360_map_last_error(self._h).decode()}")
        return rec

    def add_records(self, records):
        """Adds a list of records (uint64 [n, 8], as records() returns them) in sum mode; equal keys add up.  Every record is checked on the
        device first; one bad record raises and leaves the map unchanged.  Returns the statistics; self.full as after merge."""
        rec = np.ascontiguousarray(records, np.uint64).reshape(-1, 8)
        st = _lib.MapMergeStats()
        rc = self._L.rgbd360_map_add_records(self._handle(), _ptr(rec), rec.shape[0], 0, C.byref(st))
        self.last_status = self._check(rc)
        self.full = rc == MAP_FULL
        return _as_dict(st)

    def save(self, path):
        """numpy.savez of the records, the leaf and the box (has_box, lo, hi): load() gives the same map back."""
        has_box, lo, hi = self.box
        with open(path, "wb") as f:
            np.savez(f, records=self.records(), leaf=np.array([self.leaf], np.float32), has_box=np.array([has_box], np.uint8), lo=lo, hi=hi)

    @classmethod
    def load(cls, reg, path, capacity=None, leaf=None):
        """A new map on reg's context with the content, leaf and box of a save() file; capacity None: twice the file's voxels, at least 1024.
        leaf given: a file whose leaf bits differ is refused."""
        with np.load(path) as f:
            rec, file_leaf = np.ascontiguousarray(f["records"], np.uint64).reshape(-1, 8), np.float32(f["leaf"][0])
            has_box, lo, hi = bool(f["has_box"][0]), np.array(f["lo"], np.float32), np.array(f["hi"], np.float32)
        if leaf is not None and np.float32(leaf).tobytes() != file_leaf.tobytes():
            raise Rgbd360Error(f"VoxelMap.load: the file's leaf {file_leaf!r} is not the leaf asked for, {np.float32(leaf)!r}")
        m = cls(reg, float(file_leaf), max(2 * len(rec), 1024) if capacity is None else int(capacity))
        try:
            if has_box:
                m.set_box(lo, hi)
            else:
                m.set_box(None, None)
            m.add_records(rec)
            if m.full:
                raise Rgbd360Error("VoxelMap.load: the capacity is too small for the file's voxels")
        except Exception:
            m.close()
            raise
        return m

    # ---- the map as a spherical frame (rgbd360_map_render_sphere: the reference's viewer.globalMap, OdometryRGBD360.cpp:242-268, as a
    #      panorama; the keyframe target of OdometryKeyFrame360.cpp with the whole map as the model)
    def render_params(self, min_count=None, near=None, splat=None, max_half=None):
        """The defaults (min_count 1, near = leaf, splat 1.0, max_half 8) with the given fields replaced."""
        return self._params(_lib.MapRenderParams, self._L.rgbd360_map_default_render_params, min_count=min_count, near=near, splat=splat, max_half=max_half)

    def render_sphere(self, rows: int, cols: int, pose, **params):
        """The map splatted into the full-sphere panorama of rows x cols at `pose` (4x4 world <- frame), the nearest voxel winning a
        pixel.  Returns (depth HxW float32 metres, 0 in holes; rgb HxWx3 uint8; count HxW int32, 0 in holes; key3 HxWx3 int32; the
        statistics as a dict).  depth and rgb are what RegisterPhotoICP.setTargetFrame takes.  The map is not changed."""
        rows, cols = int(rows), int(cols)
        p = self.render_params(**params)
        g = pose_to_cm(pose)
        shape = (max(rows, 0), max(cols, 0))
        depth = np.zeros(shape, np.float32)
        rgb = np.zeros(shape + (3,), np.uint8)
        count = np.zeros(shape, np.int32)
        key3 = np.zeros(shape + (3,), np.int32)
        st = _lib.MapRenderStats()
        self._check(self._L.rgbd360_map_render_sphere(self._handle(), rows, cols, _ptr(g), C.byref(p), _ptr(depth), _ptr(rgb), _ptr(count), _ptr(key3),
                                                      C.byref(st)))
        return depth, rgb, count, key3, _as_dict(st)

    # ---- ray casting through the map (rgbd360_map_raycast*: the first occupied voxel along a ray; csrc/map_raycast.h)
    def raycast_params(self, min_count=None, t_min=None, t_max=None, max_offset=None, max_steps=None):
        """The defaults (min_count 1, t_min = leaf, t_max +inf, max_offset +inf = off, max_steps 8192) with the given fields replaced."""
        return self._params(_lib.MapRaycastParams, self._L.rgbd360_map_default_raycast_params, min_count=min_count, t_min=t_min, t_max=t_max,
                            max_offset=max_offset, max_steps=max_steps)

    def raycast(self, origins, dirs, **params):
        """The first voxel along each of n rays (origins, dirs: n x 3 float32, world coordinates; a point of the ray is o + t d).  Returns
        (t [n] float32, 0 on a miss; key3 [n, 3] int32; count [n] int32; rgb [n, 3] uint8; status [n] int32 = RAY_*; the statistics as a
        dict).  The map is not changed."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise Rgbd360Error("VoxelMap.raycast: origins and dirs must have the same shape")
        n = o.shape[0]
        p = self.raycast_params(**params)
        t = np.zeros(n, np.float32)
        key3 = np.zeros((n, 3), np.int32)
        count = np.zeros(n, np.int32)
        rgb = np.zeros((n, 3), np.uint8)
        status = np.zeros(n, np.int32)
        st = _lib.MapRaycastStats()
        self._check(self._L.rgbd360_map_raycast(self._handle(), n, _ptr(o), _ptr(d), 0, C.byref(p), _ptr(t), _ptr(key3), _ptr(count), _ptr(rgb),
                                                _ptr(status), C.byref(st)))
        return t, key3, count, rgb, status, _as_dict(st)

    def raycast_sphere(self, rows: int, cols: int, pose, **params):
        """The full-sphere panorama of rows x cols at `pose` (4x4 world <- frame) by ray casting: per pixel the first voxel along the
        pixel's ray.  Returns what render_sphere returns, (depth, rgb, count, key3, the statistics as a dict); depth and rgb are what
        RegisterPhotoICP.setTargetFrame takes.  The map is not changed."""
        rows, cols = int(rows), int(cols)
        p = self.raycast_params(**params)
        g = pose_to_cm(pose)
        shape = (max(rows, 0), max(cols, 0))
        depth = np.zeros(shape, np.float32)
        rgb = np.zeros(shape + (3,), np.uint8)
        count = np.zeros(shape, np.int32)
        key3 = np.zeros(shape + (3,), np.int32)
        st = _lib.MapRaycastStats()
        self._check(self._L.rgbd360_map_raycast_sphere(self._handle(), rows, cols, _ptr(g), C.byref(p), _ptr(depth), _ptr(rgb), _ptr(count), _ptr(key3),
                                                       C.byref(st)))
        return depth, rgb, count, key3, _as_dict(st)

    # ---- surface normals (rgbd360_map_normals, rgbd360_map_raycast_surface*: one normal per voxel fitted to the centroids of the 27 cells
    #      around it, resident next to the table; csrc/map_normals.h)
    def normal_params(self, min_count=None, min_support=None, max_flatness=None, max_shift=None):
        """The defaults (min_count 1, min_support 5, max_flatness 0.05, max_shift 2.0 leaves) with the given fields replaced."""
        return self._params(_lib.MapNormalParams, self._L.rgbd360_map_default_normal_params, min_count=min_count, min_support=min_support,
                            max_flatness=max_flatness, max_shift=max_shift)

    def normals(self, viewpoint=None, max_out=None, **params):
        """One record per voxel, in no specified order: (xyz [k, 3] float32, normal [k, 3] float32, curvature [k] float32, status [k] int32 =
        NORMAL_*, count [k] int32, key3 [k, 3] int32, the statistics as a dict), k = min(len, max_out).  viewpoint (3 floats, world): the
        normals face it; None: the canonical sign (the largest component positive).  The normal is zero unless the status is NORMAL_OK."""
        p = self.normal_params(**params)
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float32).reshape(3)
        n = len(self)
        k = n if max_out is None else min(n, int(max_out))
        xyz, normal, key3 = np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32), np.zeros((k, 3), np.int32)
        curvature, status, count = np.zeros(k, np.float32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        st = _lib.MapNormalStats()
        got = self._L.rgbd360_map_normals(self._handle(), C.byref(p), None if v is None else _ptr(v), k, _ptr(xyz), _ptr(normal), _ptr(curvature),
                                          _ptr(status), _ptr(count), _ptr(key3), C.byref(st))
        if got != n:
            raise Rgbd360Error(f"rgbd360_map_normals failed ({got}): {self._L.rgbd360_map_last_error(self._h).decode()}")
        return xyz, normal, curvature, status, count, key3, _as_dict(st)

    # ---- colour (rgbd360_map_colours: one intensity per voxel and its gradient on the voxel's tangent plane, resident next to the table;
    #      csrc/map_colour.h)
    def colour_params(self, min_count=None, min_support=None, max_flatness=None, min_gradient_support=None, min_spread=None):
        """The defaults (min_count 1, min_support 5, max_flatness 0.05, min_gradient_support 4, min_spread 0.01) with the given fields
        replaced."""
        return self._params(_lib.MapColourParams, self._L.rgbd360_map_default_colour_params, min_count=min_count, min_support=min_support,
                            max_flatness=max_flatness, min_gradient_support=min_gradient_support, min_spread=min_spread)

    def colours(self, max_out=None, **params):
        """One record per voxel, ordered by (i_z, i_y, i_x) as extract(): (xyz [k, 3] float32, intensity [k] float32 in [0, 1], gradient
        [k, 3] float32 per metre, world coordinates, tangent to the voxel's plane, status [k] int32 = COLOUR_*, count [k] int32, key3 [k, 3]
        int32, the statistics as a dict), k = min(len, max_out).  The gradient is zero unless the status is COLOUR_OK.  A map fed without
        colours has zero intensities and gradients."""
        p = self.colour_params(**params)
        n = len(self)
        k = n if max_out is None else min(n, int(max_out))
        xyz, gradient, key3 = np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32), np.zeros((k, 3), np.int32)
        intensity, status, count = np.zeros(k, np.float32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        st = _lib.MapColourStats()
        got = self._L.rgbd360_map_colours(self._handle(), C.byref(p), k, _ptr(xyz), _ptr(intensity), _ptr(gradient), _ptr(status), _ptr(count), _ptr(key3),
                                          C.byref(st))
        if got != n:
            raise Rgbd360Error(f"rgbd360_map_colours failed ({got}): {self._L.rgbd360_map_last_error(self._h).decode()}")
        return xyz, intensity, gradient, status, count, key3, _as_dict(st)

    @property
    def colour_bytes(self) -> int:
        """Device memory of the colour layer (16 bytes per slot once a call needed it; 0 after release_colours)."""
        return int(self._L.rgbd360_map_colour_bytes(self._handle()))

    def release_colours(self):
        self._check(self._L.rgbd360_map_release_colours(self._handle()))

    def _surface_params(self, params):
        names = ("min_support", "max_flatness", "max_shift", "normal_min_count")
        nm = {k: params.pop(k) for k in names if k in params}
        nm["min_count"] = nm.pop("normal_min_count", None)
        return self.raycast_params(**params), self.normal_params(**nm)

    def raycast_surface(self, origins, dirs, **params):
        """raycast with the surface: (t, normal [n, 3] float32, key3, count, rgb, status, n_on_plane, the statistics).  A hit whose voxel has
        a normal gets it, facing the ray's origin, and the depth on the plane through the voxel's centroid (n_on_plane counts those); all
        else is raycast's, bit for bit.  params: raycast_params' fields, and min_support, max_flatness, max_shift, normal_min_count."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise Rgbd360Error("VoxelMap.raycast_surface: origins and dirs must have the same shape")
        n = o.shape[0]
        p, q = self._surface_params(params)
        t = np.zeros(n, np.float32)
        normal = np.zeros((n, 3), np.float32)
        key3 = np.zeros((n, 3), np.int32)
        count = np.zeros(n, np.int32)
        rgb = np.zeros((n, 3), np.uint8)
        status = np.zeros(n, np.int32)
        on_plane = C.c_longlong()
        st = _lib.MapRaycastStats()
        self._check(self._L.rgbd360_map_raycast_surface(self._handle(), n, _ptr(o), _ptr(d), 0, C.byref(p), C.byref(q), _ptr(t), _ptr(normal), _ptr(key3),
                                                        _ptr(count), _ptr(rgb), _ptr(status), C.byref(on_plane), C.byref(st)))
        return t, normal, key3, count, rgb, status, int(on_plane.value), _as_dict(st)

    def raycast_surface_sphere(self, rows: int, cols: int, pose, **params):
        """raycast_sphere with the surface: (depth, normal HxWx3 float32 in world coordinates, rgb, count, key3, n_on_plane, the
        statistics); depth and rgb are what RegisterPhotoICP.setTargetFrame takes."""
        rows, cols = int(rows), int(cols)
        p, q = self._surface_params(params)
        g = pose_to_cm(pose)
        shape = (max(rows, 0), max(cols, 0))
        depth = np.zeros(shape, np.float32)
        normal = np.zeros(shape + (3,), np.float32)
        rgb = np.zeros(shape + (3,), np.uint8)
        count = np.zeros(shape, np.int32)
        key3 = np.zeros(shape + (3,), np.int32)
        on_plane = C.c_longlong()
        st = _lib.MapRaycastStats()
        self._check(self._L.rgbd360_map_raycast_surface_sphere(self._handle(), rows, cols, _ptr(g), C.byref(p), C.byref(q), _ptr(depth), _ptr(normal),
                                                               _ptr(rgb), _ptr(count), _ptr(key3), C.byref(on_plane), C.byref(st)))
        return depth, normal, rgb, count, key3, int(on_plane.value), _as_dict(st)

    def raycast_set_plain(self, plain: bool):
        """Diagnostics: the one-level traversal instead of the coarse layer for the later ray casts; the outputs are the same bits."""
        self._check(self._L.rgbd360_map_raycast_set_plain(self._handle(), int(bool(plain))))

    # ---- free-space observation and carving (rgbd360_map_observe_* / _votes / _carve: the voxels a posed frame looks straight through,
    #      counted per voxel and erased on request; csrc/map_carve.h)
    def observe_params(self, min_count=None, near=None, margin_leaves=None, margin_rel=None, max_offset=None, max_steps=None, accumulate=None):
        """The defaults (min_count 1, near = leaf, margin_leaves 2.0, margin_rel 0, max_offset 0.5 leaves, max_steps 8192, accumulate 0) with
        the given fields replaced."""
        accumulate = None if accumulate is None else int(accumulate)
        return self._params(_lib.MapObserveParams, self._L.rgbd360_map_default_observe_params, min_count=min_count, near=near,
                            margin_leaves=margin_leaves, margin_rel=margin_rel, max_offset=max_offset, max_steps=max_steps, accumulate=accumulate)

    def observe_sphere(self, depth, pose, convention: int = 0, **params):
        """Every pixel of the sphere frame `depth` (as in insert_sphere) at `pose` is a line of sight: the map voxels it passes through
        well in front of the measured point get a through-vote, the voxel the point would feed an end-vote.  accumulate=True adds to the
        votes of earlier observations.  Returns the statistics as a dict.  The map's table is not changed."""
        args, keep = self._sphere_args("observe_sphere", None, depth, convention, colour=False)
        p = self.observe_params(**params)
        g = pose_to_cm(pose)
        st = _lib.MapObserveStats()
        self._check(self._L.rgbd360_map_observe_sphere(self._handle(), *args, _ptr(g), 0, C.byref(p), C.byref(st)))
        return _as_dict(st)

    def observe_rays(self, origins, endpoints, **params):
        """The same for n segments (origins, endpoints: n x 3 float32, world coordinates; the measurement is the endpoint)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        w = np.ascontiguousarray(endpoints, np.float32).reshape(-1, 3)
        if o.shape != w.shape:
            raise Rgbd360Error("VoxelMap.observe_rays: origins and endpoints must have the same shape")
        p = self.observe_params(**params)
        st = _lib.MapObserveStats()
        self._check(self._L.rgbd360_map_observe_rays(self._handle(), o.shape[0], _ptr(o), _ptr(w), 0, C.byref(p), C.byref(st)))
        return _as_dict(st)

    def votes(self, max_out=None):
        """(key3 [k, 3] int32, through [k] int32, end [k] int32, count [k] int32) of the voxels with a vote, ascending by (i_z, i_y, i_x);
        count is the voxel's count now, 0 once a carve erased it.  Raises when the map holds no votes or was written since they were taken."""
        n = self._L.rgbd360_map_votes(self._handle(), 0, None, None, None, None)
        if n < 0:
            raise Rgbd360Error(f"rgbd360_map_votes failed ({n}): {self._L.rgbd360_map_last_error(self._h).decode()}")
        k = n if max_out is None else min(n, int(max_out))
        key3 = np.zeros((k, 3), np.int32)
        through, end, count = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        got = self._L.rgbd360_map_votes(self._handle(), k, _ptr(key3), _ptr(through), _ptr(end), _ptr(count))
        if got != n:
            raise Rgbd360Error(f"rgbd360_map_votes failed ({got}): {self._L.rgbd360_map_last_error(self._h).decode()}")
        return key3, through, end, count

    def carve(self, min_through: int = 1, max_end: int = 0, max_count: int = 0):
        """Erases the live voxels with through >= min_through, end <= max_end and (max_count == 0 or count <= max_count); the votes are
        spent afterwards.  A lossy edit: a later remove of a frame that fed a carved voxel reports a mismatch.  Returns the statistics."""
        st = _lib.MapCarveStats()
        self._check(self._L.rgbd360_map_carve(self._handle(), int(min_through), int(max_end), int(max_count), C.byref(st)))
        return _as_dict(st)

    def vote_bytes(self) -> int:
        """Device memory of the vote array (8 bytes per slot once an observation was made; 0 after release_votes or rehash)."""
        return int(self._L.rgbd360_map_vote_bytes(self._handle()))

    def release_votes(self):
        self._check(self._L.rgbd360_map_release_votes(self._handle()))

    # ---- planar regions and relocalisation (rgbd360_map_planes, rgbd360_map_plane_labels; csrc/map_planes.h): the map segmented into
    #      planes, a PbMap of the global map, and a frame placed in it without an initial guess (the reference's Relocalizer360)
    def plane_seg_params(self, **kw):
        """The defaults (min_count 1, min_support 5, max_flatness 0.05, max_voxel_curvature inf, cos_angle cos 5 deg, max_offset 0.5
        leaves, min_voxels 50, max_curvature 0.0013) with the given fields replaced."""
        return self._params(_lib.MapPlaneSegParams, self._L.rgbd360_map_default_plane_seg_params, **kw)

    def planes(self, viewpoint=None, max_planes: int = 256, **params):
        """(planes, root_key3 [k, 3] int32, the statistics): the map's planar regions as the plane dicts of the frame plane calls, by root
        key ascending, with the key of each region's root voxel.  viewpoint: three floats the normals face (None: the origin).  More than
        max_planes passing the filters: the max_planes of most voxels; the statistics' n_planes_available counts them all."""
        p = self.plane_seg_params(**params)
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float32).reshape(3)
        k = max(int(max_planes), 0)
        arr = (_lib.Plane * max(k, 1))()
        key3 = np.zeros((k, 3), np.int32)
        n, st = C.c_int(0), _lib.MapPlaneSegStats()
        self._check(self._L.rgbd360_map_planes(self._handle(), C.byref(p), None if v is None else _ptr(v), int(max_planes), C.cast(arr, C.c_void_p),
                                               _ptr(key3), C.byref(n), C.byref(st)))
        return _planes_to_dicts(arr, n.value), key3[:n.value].copy(), _as_dict(st)

    def plane_labels(self, **params):
        """One record per voxel, in no specified order: (key3 [k, 3] int32, label_key3 [k, 3] int32 = the root key of the voxel's region,
        its own key where it is not eligible, plane_index [k] int32 = the region's place among the planes that pass the filters, -1:
        none)."""
        p = self.plane_seg_params(**params)
        k = len(self)
        key3, label, index = np.zeros((k, 3), np.int32), np.zeros((k, 3), np.int32), np.full(k, -1, np.int32)
        got = self._L.rgbd360_map_plane_labels(self._handle(), C.byref(p), k, _ptr(key3), _ptr(label), _ptr(index))
        if got != k:
            raise Rgbd360Error(f"rgbd360_map_plane_labels failed ({got}): {self._L.rgbd360_map_last_error(self._h).decode()}")
        return key3, label, index

    def relocalize(self, frame_planes, max_match_planes: int = 0, regist_mode: int = pbmap.DEFAULT_6DoF, params=None, **seg_params):
        """The frame whose planes are `frame_planes` (plane dicts in the frame's coordinates) placed in the map without an initial guess:
        pbmap.register_planes(ref = the map's planes, trg = frame_planes).  Returns that dict -- status 0 accepted, pose 4x4 world <- frame,
        info, match {map plane: frame plane}, area_matched -- with map_planes, root_key3 and stats, the map planes it was matched against.
        seg_params: viewpoint, max_planes and plane_seg_params' fields."""
        map_planes, root_key3, stats = self.planes(**seg_params)
        out = pbmap.register_planes(map_planes, frame_planes, max_match_planes=max_match_planes, regist_mode=regist_mode, params=params)
        out.update(map_planes=map_planes, root_key3=root_key3, stats=stats)
        return out

    def plane_bytes(self) -> int:
        """Device memory of the label layer and the region lists (0 after release_planes)."""
        return int(self._L.rgbd360_map_plane_bytes(self._handle()))

    def release_planes(self):
        self._check(self._L.rgbd360_map_release_planes(self._handle()))

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
