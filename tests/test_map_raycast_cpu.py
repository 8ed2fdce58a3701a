"""CPU tests of ray casting through the voxel map: the numpy restatement (tests/map_raycast_reference.py) against answers derived by hand
-- a single voxel along each axis, the diagonal through a cell corner that pins the tie rule, a ray that starts inside a voxel, negative
coordinates, the box, t_max, max_steps, max_offset, bad rays -- the condition of the sphere scene, proven on the restatement, and the
agreement of the header, the ctypes binding and the C++ adapter.

The hand cases use cells of 0.25 m (inv_leaf = 4) and dyadic coordinates, so every number below is exact."""
import ctypes as C
import os
import re

import numpy as np

import map_raycast_reference as M
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
F = np.float32
LEAF = 0.25
Q = 0.125       # half a cell


def centres(cells):
    """A map of one point per cell, at the cell's centre; colours 10 k + (1, 2, 3)."""
    xyz = np.array([[(c + 0.5) * LEAF for c in cell] for cell in cells], F)
    rgb = np.array([[10 * k + 1, 10 * k + 2, 10 * k + 3] for k in range(len(cells))], np.uint8)
    ref = R.Map([(xyz, rgb, EYE)], LEAF, None)
    assert sorted(map(tuple, ref.key.tolist())) == sorted(map(tuple, cells))
    return ref


def one(ref, o, d, **params):
    out = M.cast(ref, LEAF, np.array([o], F), np.array([d], F), **params)
    return int(out["status"][0]), float(out["t"][0]), tuple(out["key3"][0].tolist()), out["stats"]


def test_a_single_voxel_along_each_axis():
    for axis in range(3):
        cell = [0, 0, 0]
        cell[axis] = 4
        ref = centres([tuple(cell)])
        o, d = [Q, Q, Q], [0.0, 0.0, 0.0]
        o[axis], d[axis] = 0.0, 1.0
        # the box is the one cell: entered at t = 1, left at 1.25, the centre projects to 1.125
        st, t, key, stats = one(ref, o, d)
        assert (st, t, key) == (M.HIT, 1.125, tuple(cell)) and stats["n_steps"] == 1 and stats["n_hits"] == 1 and stats["n_lookups"] == 1
        # t is in units of |d|
        d[axis] = 2.0
        assert one(ref, o, d)[:3] == (M.HIT, 0.5625, tuple(cell))
        # from the other side: the box entered at (5 - 8) (-1 / 4) = 0.75, the centre at 0.875
        o[axis], d[axis] = 2.0, -1.0
        assert one(ref, o, d)[:3] == (M.HIT, 0.875, tuple(cell))
        # the voxel behind the origin: the slab test ends before it begins
        d[axis] = 1.0
        st, t, key, stats = one(ref, o, d)
        assert (st, t, key) == (M.MISS_BOX, 0.0, (0, 0, 0)) and stats["n_steps"] == 0 and stats["n_miss_box"] == 1
        # the centroid is projected, then clamped into the cell's span: a point in the cell's far corner seen along the axis
        pt = np.array([[(c + 0.5) * LEAF for c in cell]], F)
        pt[0, axis] += F(0.09375)
        ref2 = R.Map([(pt, None, EYE)], LEAF, None)
        o[axis], d[axis] = 0.0, 1.0
        assert one(ref2, o, d)[:3] == (M.HIT, 1.21875, tuple(cell))


def test_the_diagonal_through_a_cell_corner_pins_the_tie_rule():
    """From the centre of cell (0, 0, 0) along (1, 1, 1) all three boundary times are equal at every corner: x steps first, then y, then z.
    The ray visits (0,0,0), (1,0,0), (1,1,0), (1,1,1) and never (0,1,0) or (0,0,1), which touch the same corner."""
    o, d = [Q, Q, Q], [1.0, 1.0, 1.0]
    ref = centres([(0, 1, 0), (0, 0, 1), (1, 1, 1)])
    st, t, key, stats = one(ref, o, d, t_min=0.0)
    assert (st, t, key) == (M.HIT, 0.25, (1, 1, 1)) and stats["n_steps"] == 4
    # with (1, 0, 0) occupied the ray stops there: entered and left at t = 0.125 (y steps next at the same time), the centre projects to
    # (0.25 + 0 + 0) / 3 and is clamped to the cell's span
    ref = centres([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
    st, t, key, stats = one(ref, o, d, t_min=0.0)
    assert (st, t, key) == (M.HIT, 0.125, (1, 0, 0)) and stats["n_steps"] == 2
    # in the plane: (1, 1, 0) takes x before y as well
    ref = centres([(0, 1, 0), (1, 1, 0), (1, 0, 1)])          # (the third only widens the box to the cells 0 .. 1 of every axis)
    st, t, key, stats = one(ref, o, [1.0, 1.0, 0.0], t_min=0.0)
    assert (st, t, key) == (M.HIT, 0.25, (1, 1, 0)) and stats["n_steps"] == 3
    # and with negative steps: (-1, -1, -1) from the same centre visits (-1,0,0), (-1,-1,0), (-1,-1,-1)
    ref = centres([(0, -1, 0), (0, 0, -1), (-1, -1, -1)])
    st, t, key, stats = one(ref, o, [-1.0, -1.0, -1.0], t_min=0.0)
    assert (st, t, key) == (M.HIT, 0.25, (-1, -1, -1)) and stats["n_steps"] == 4


def test_a_ray_that_starts_inside_an_occupied_voxel():
    ref = centres([(0, 0, 0), (3, 0, 0)])
    o, d = [0.0625, Q, Q], [1.0, 0.0, 0.0]
    # t_min = leaf: the own voxel's hit at 0.0625 is passed through, cells 1 and 2 are air, cell 3 is entered at (3 - 0.25) / 4
    st, t, key, stats = one(ref, o, d)
    assert (st, t, key) == (M.HIT, 0.8125, (3, 0, 0)) and stats["n_steps"] == 4
    assert stats["n_lookups"] == 2 and one(ref, o, d, layer=False)[3]["n_lookups"] == 4
    st, t, key, stats = one(ref, o, d, t_min=0.0)
    assert (st, t, key) == (M.HIT, 0.0625, (0, 0, 0)) and stats["n_steps"] == 1
    # t_max: cell 3 is entered at 0.6875 > 0.5, after three cells
    st, t, key, stats = one(ref, o, d, t_max=0.5)
    assert (st, t, key) == (M.T_MAX, 0.0, (0, 0, 0)) and stats["n_steps"] == 3 and stats["n_t_max"] == 1
    assert one(ref, o, d, t_max=0.6875)[0] == M.HIT          # the entry AT t_max still counts
    # max_steps: two cells visited, none a hit
    st, t, key, stats = one(ref, o, d, max_steps=2)
    assert st == M.MAX_STEPS and stats["n_steps"] == 2 and stats["n_max_steps"] == 1
    assert one(ref, o, d, max_steps=4)[0] == M.HIT
    # min_count: single points do not stop a ray that asks for two
    st, _, _, stats = one(ref, o, d, min_count=2)
    assert st == M.LEFT_BOX and stats["n_steps"] == 4 and stats["n_left_box"] == 1


def test_negative_coordinates():
    ref = centres([(-1, -1, -1), (-9, -1, -1)])
    st, t, key, stats = one(ref, [0.625, -Q, -Q], [-1.0, 0.0, 0.0])
    assert (st, t, key) == (M.HIT, 0.75, (-1, -1, -1)) and stats["n_steps"] == 1          # the box begins at x = 0: cell -1 is the first
    # through -1 | 0 the other way round: from inside cell -9 to cell -1, eight cells, across the brick boundary -9 | -8
    st, t, key, stats = one(ref, [-2.1875, -Q, -Q], [1.0, 0.0, 0.0])
    assert (st, t, key) == (M.HIT, 2.0625, (-1, -1, -1)) and stats["n_steps"] == 9
    # -0.01 lies in cell -1 (floor, not truncation)
    ref = R.Map([(np.array([[-0.01, -0.01, -0.01]], F), None, EYE)], LEAF, None)
    assert ref.key.tolist() == [[-1, -1, -1]]
    st, t, key, _ = one(ref, [-Q, -Q, 1.0], [0.0, 0.0, -1.0])
    assert (st, key) == (M.HIT, (-1, -1, -1)) and t == F(1.0 - np.float64(ref.xyz[0, 2])) and 1.0 < t < 1.02


def test_the_box_and_the_offset():
    ref = centres([(3, 0, 0)])
    assert one(ref, [0.0, 5.0, Q], [1.0, 0.0, 0.0])[0] == M.MISS_BOX            # parallel to the box, outside its slab
    assert one(ref, [0.0, 0.25, Q], [1.0, 0.0, 0.0])[0] == M.MISS_BOX           # g_y = 1 = hi + 1: cells are [i, i + 1)
    assert one(ref, [0.0, 0.0, Q], [1.0, 0.0, 0.0])[0] == M.HIT                 # g_y = 0 = lo: along the cell's face, inside
    assert one(ref, [0.0, 1.0, Q], [1.0, -0.5, 0.0])[0] == M.MISS_BOX           # crosses y in 0 .. 0.25 before x reaches 0.75
    # a centroid 0.0625 m = 0.25 leaves off the ray
    pt = np.array([[0.875, 0.1875, Q]], F)
    ref = R.Map([(pt, None, EYE)], LEAF, None)
    o, d = [0.0, Q, Q], [1.0, 0.0, 0.0]
    assert one(ref, o, d)[:3] == (M.HIT, 0.875, (3, 0, 0))
    assert one(ref, o, d, max_offset=0.25)[0] == M.HIT                           # rejected only when farther
    st, t, key, stats = one(ref, o, d, max_offset=0.2)
    assert (st, t, key) == (M.LEFT_BOX, 0.0, (0, 0, 0)) and stats["n_steps"] == 1


def test_bad_rays_and_empty_inputs():
    ref = centres([(3, 0, 0)])
    o = np.array([[0, Q, Q]] * 6, F)
    d = np.array([[1, 0, 0], [0, 0, 0], [np.nan, 0, 0], [1, np.inf, 0], [1, 0, 0], [-0.0, 0.0, -0.0]], F)
    o[4, 2] = -np.inf
    out = M.cast(ref, LEAF, o, d)
    assert out["status"].tolist() == [M.HIT, M.BAD, M.BAD, M.BAD, M.BAD, M.BAD]
    assert out["stats"] == dict(n_rays=6, n_hits=1, n_miss_box=0, n_left_box=0, n_t_max=0, n_max_steps=0, n_bad_rays=5, n_steps=1, n_lookups=1)
    assert not out["t"][1:].any() and not out["count"][1:].any() and out["rgb"][0].tolist() == [1, 2, 3]
    empty = R.Map([], LEAF, None)
    out = M.cast(empty, LEAF, o, d)
    assert out["stats"] == dict.fromkeys(M.STAT_NAMES, 0) and not out["status"].any()
    out = M.cast_sphere(empty, LEAF, 32, 64, EYE)
    assert out["depth"].shape == (32, 64) and out["stats"] == dict.fromkeys(M.STAT_NAMES, 0)


def test_sphere_rays_are_unit_vectors_through_the_pixel_centres():
    o, d = M.sphere_rays(32, 64, R.general_pose())
    assert np.array_equal(o, np.broadcast_to(R.general_pose()[:3, 3], o.shape))
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    o, d = M.sphere_rays(32, 64, EYE)
    d = d.reshape(32, 64, 3)
    assert d[0, 0, 0] > 0.99 and d[31, 0, 0] < -0.99          # the first row looks up (+x), the last down
    assert abs(d[16, 0, 1]) < 1e-6 and d[16, 0, 2] < 0 and d[16, 16, 1] < -0.99 and d[16, 32, 2] > 0.99      # theta = 0 looks along -z


def sphere_cloud(radius, n):
    """n points on the sphere of `radius` around the origin, a Fibonacci lattice."""
    k = np.arange(n) + 0.5
    z = 1 - 2 * k / n
    rho = np.sqrt(1 - z * z)
    th = np.pi * (1 + 5 ** 0.5) * k
    return (radius * np.stack([rho * np.cos(th), rho * np.sin(th), z], axis=1)).astype(F)


SPHERE_POINTS = 400000      # 0.0084 m between neighbours, a sixth of a cell: dense enough that the restatement leaves no miss (checked below)


def sphere_scene_checks(out, radius, leaf):
    """Every pixel hits, within the cell diagonal of the sphere."""
    d = out["depth"]
    assert (out["count"] > 0).all(), int((out["count"] == 0).sum())
    assert (np.abs(d.astype(np.float64) - radius) <= np.sqrt(3.0) * leaf).all(), (d.min(), d.max())


def test_every_pixel_of_a_sphere_scene_hits_on_the_restatement():
    leaf = 0.05
    ref = R.Map([(sphere_cloud(1.5, SPHERE_POINTS), None, EYE)], leaf, None)
    out = M.cast_sphere(ref, leaf, 32, 64, EYE)
    print("voxels", len(ref), out["stats"], out["depth"].min(), out["depth"].max())
    assert out["stats"]["n_hits"] == 32 * 64 and (out["status"] == M.HIT).all()
    sphere_scene_checks(out, 1.5, leaf)


def test_header_binding_and_adapter_agree():
    from rgbd360_amd import _lib, build, voxel_map
    L = C.CDLL(build.build())
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    for name in ("rgbd360_map_default_raycast_params", "rgbd360_map_raycast", "rgbd360_map_raycast_sphere", "rgbd360_map_raycast_sphere_dev"):
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS
    for name in ("rgbd360_map_time_raycast", "rgbd360_map_raycast_set_plain"):
        assert re.search(r"\b%s\s*\(" % name, diag) and name not in main and hasattr(L, name) and name in _lib.SYMBOLS

    def fields(text, struct):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, text).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
        return names

    for struct, cls, size in (("rgbd360_map_raycast_params", _lib.MapRaycastParams, 20), ("rgbd360_map_raycast_stats", _lib.MapRaycastStats, 72),
                              ("rgbd360_map_render_params", _lib.MapRenderParams, 16)):
        assert fields(main, struct) == [n for n, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    assert [n for n, _ in _lib.MapRaycastStats._fields_] == list(M.STAT_NAMES)
    status = dict(re.findall(r"RGBD360_RAY_([A-Z_]+) = (\d)", main))
    assert {k: int(v) for k, v in status.items()} == dict(MISS_BOX=M.MISS_BOX, HIT=M.HIT, LEFT_BOX=M.LEFT_BOX, T_MAX=M.T_MAX, MAX_STEPS=M.MAX_STEPS, BAD=M.BAD)
    assert (voxel_map.RAY_MISS_BOX, voxel_map.RAY_HIT, voxel_map.RAY_LEFT_BOX, voxel_map.RAY_T_MAX, voxel_map.RAY_MAX_STEPS, voxel_map.RAY_BAD) == tuple(range(6))
    L.rgbd360_map_default_raycast_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapRaycastParams)]
    L.rgbd360_map_default_raycast_params.restype = None
    p = _lib.MapRaycastParams()
    L.rgbd360_map_default_raycast_params(None, C.byref(p))
    assert (p.min_count, p.max_steps) == (1, 8192) and p.t_min == F(0.05) and p.t_max == np.inf and p.max_offset == np.inf
    assert (M.DEFAULTS["min_count"], M.DEFAULTS["t_max"], M.DEFAULTS["max_offset"], M.DEFAULTS["max_steps"]) == (p.min_count, p.t_max, p.max_offset, p.max_steps)
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("raycastSphere", "raycastParams", "raycastStats", "void raycast(", "rgbd360_map_raycast_sphere", "rgbd360_map_default_raycast_params"):
        assert name in hpp, name
    py = open(os.path.join(ROOT, "rgbd360_amd", "voxel_map.py")).read()
    assert "def raycast_sphere" in py and "def raycast_params" in py and "def raycast(" in py
    assert "--raycast-map" in open(os.path.join(ROOT, "examples", "odometry_replay.cpp")).read()
    assert "rgbd360_map_raycast" in open(os.path.join(ROOT, "README.md")).read()
    # the sentence that declared ray casting out of scope is gone
    for doc in ("include/rgbd360_hip.h", "DESIGN.md"):
        assert "ray casting through the grid, pinhole views" not in open(os.path.join(ROOT, doc)).read(), doc
