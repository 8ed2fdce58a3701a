"""CPU tests of the voxel map's surface normals and of the surface cast: the numpy restatement (tests/map_normals_reference.py) against
answers derived by hand -- a flat patch, supports, tombstones, the viewpoint, the canonical sign, the plane depth of a ray --, the host
plane function against the restatement's on the supports of a scene, the agreement of the header, the ctypes binding, the adapter and
the example, the conditions of the GPU scenes proven on the restatement, and the feature's number: the depth error of the sphere
panorama with and without the surface.

The hand cases use cells of 0.25 m (inv_leaf = 4) and dyadic coordinates, so every number in them is exact."""
import ctypes as C
import os
import re

import numpy as np

import map_align_plane_reference as P
import map_normals_reference as N
import map_raycast_reference as M
import voxel_map_reference as R
from test_map_raycast_cpu import LEAF, SPHERE_POINTS, centres, sphere_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
F = np.float32
OFF_CENTRE = (0.5, -0.3, 0.2)


def patch(axis=2, at=0):
    """The 3 x 3 cells 0 .. 2 x 0 .. 2 in the plane `axis` = `at`."""
    cells = []
    for a in range(3):
        for b in range(3):
            c = [a, b]
            c.insert(axis, at)
            cells.append(tuple(c))
    return cells


def by_key(ref, out, cell):
    row = np.nonzero((out["key3"] == np.array(cell, np.int32)).all(axis=1))[0]
    assert len(row) == 1, cell
    return int(row[0])


def test_a_flat_patch():
    ref = centres(patch())
    out = N.normals(ref)
    centre, corner, edge = by_key(ref, out, (1, 1, 0)), by_key(ref, out, (0, 0, 0)), by_key(ref, out, (1, 0, 0))
    assert out["support"][centre] == 9 and out["support"][edge] == 6 and out["support"][corner] == 4
    assert out["status"][centre] == N.OK and out["normal"][centre].tolist() == [0.0, 0.0, 1.0] and out["curvature"][centre] == 0.0
    assert out["status"][edge] == N.OK and out["normal"][edge].tolist() == [0.0, 0.0, 1.0]
    assert out["status"][corner] == N.UNSUPPORTED and not out["normal"][corner].any()
    assert out["stats"] == dict(n_voxels=9, n_below_min_count=0, n_unsupported=4, n_nonplanar=0, n_normals=5)
    out = N.normals(ref, min_support=3)
    assert out["status"][corner] == N.OK and out["normal"][corner].tolist() == [0.0, 0.0, 1.0] and out["stats"]["n_normals"] == 9
    # the read-out's other planes are the map's
    assert out["xyz"].tobytes() == ref.xyz.tobytes() and np.array_equal(out["count"], ref.count) and np.array_equal(out["key3"], ref.key)


def test_a_lone_voxel_is_unsupported_and_the_corner_of_a_room_is_nonplanar():
    out = N.normals(centres([(3, -2, 5)]))
    assert out["status"].tolist() == [N.UNSUPPORTED] and out["support"].tolist() == [1] and not out["normal"].any() and not out["curvature"].any()
    assert N.normals(centres([(3, -2, 5)]), min_support=1)["status"].tolist() == [N.NONPLANAR]       # a point has no plane either
    ref = R.Map([(P.corner_scene(1, size=1.0, step=0.05), None, EYE)], LEAF, None)
    out = N.normals(ref)
    corner = by_key(ref, out, (0, 0, 0))
    assert out["status"][corner] == N.NONPLANAR and not out["normal"][corner].any() and out["curvature"][corner] > 0.05
    # ... while the middle of each wall, two cells from the others, is a plane along its axis
    for axis in range(3):
        cell = [2, 2, 2]
        cell[axis] = 0
        row = by_key(ref, out, tuple(cell))
        want = [0.0, 0.0, 0.0]
        want[axis] = 1.0
        assert out["status"][row] == N.OK and out["support"][row] == 9 and np.abs(out["normal"][row] - want).max() < 1e-6


def test_min_count_drops_single_points_out_of_a_support():
    cells = patch()
    xyz = np.array([[(c + 0.5) * LEAF for c in cell] for cell in cells], F)
    twice = xyz[[k for k, c in enumerate(cells) if c[1] == 1]]        # the middle row holds two points per cell
    ref = R.Map([(xyz, None, EYE), (twice, None, EYE)], LEAF, None)
    out = N.normals(ref, min_count=2)
    centre, corner = by_key(ref, out, (1, 1, 0)), by_key(ref, out, (0, 0, 0))
    assert out["support"][centre] == 3 and out["status"][centre] == N.UNSUPPORTED
    assert out["status"][corner] == N.NONE and out["support"][corner] == 0
    assert out["stats"] == dict(n_voxels=9, n_below_min_count=6, n_unsupported=3, n_nonplanar=0, n_normals=0)
    assert N.normals(ref, min_count=2, min_support=3)["status"][centre] == N.NONPLANAR       # three centroids in a line
    assert N.normals(ref)["support"][centre] == 9


def test_a_tombstoned_neighbour_is_absent():
    ref = centres(patch())
    gone = int(np.nonzero((ref.key == (0, 0, 0)).all(axis=1))[0][0])
    ref.count[gone] = 0
    out = N.normals(ref)
    assert out["stats"]["n_voxels"] == 8 and len(out["status"]) == 8 and not (out["key3"] == (0, 0, 0)).all(axis=1).any()
    assert out["support"][by_key(ref, out, (1, 1, 0))] == 8 and out["support"][by_key(ref, out, (1, 0, 0))] == 5
    assert out["support"][by_key(ref, out, (0, 1, 0))] == 5


def test_the_viewpoint_and_the_canonical_sign():
    ref = centres(patch())
    below = N.normals(ref, viewpoint=(0.375, 0.375, -1.0))
    above = N.normals(ref, viewpoint=(0.375, 0.375, 1.0))
    centre = by_key(ref, below, (1, 1, 0))
    assert below["normal"][centre].tolist() == [0.0, 0.0, -1.0] and above["normal"][centre].tolist() == [0.0, 0.0, 1.0]
    assert not below["normal"][by_key(ref, below, (0, 0, 0))].any()          # only OK normals turn
    # a patch in y = const: the plane function's cross product points along -y, the stored normal along +y
    ref = centres(patch(axis=1, at=-3))
    L = N.layer(ref)
    centre = int(np.nonzero((ref.key == (1, -3, 1)).all(axis=1))[0][0])
    raw = P.plane_fit(L["cov"][centre], 0.05)[0][0]
    assert raw.tolist() == [0.0, -1.0, 0.0] and L["normal"][centre].tolist() == [0.0, 1.0, 0.0]
    # ... and in x = const
    ref = centres(patch(axis=0, at=2))
    assert N.layer(ref)["normal"][int(np.nonzero((ref.key == (2, 1, 1)).all(axis=1))[0][0])].tolist() == [1.0, 0.0, 0.0]


def test_a_ray_onto_the_patch_gets_the_plane_depth():
    ref = centres(patch(at=4))
    # straight down the z axis: the normal faces the ray, the depth is the centroid's either way
    out = N.cast_surface(ref, LEAF, [[0.3125, 0.4375, 0.0]], [[0.0, 0.0, 1.0]])
    assert out["status"].tolist() == [M.HIT] and out["key3"][0].tolist() == [1, 1, 4] and out["normal"][0].tolist() == [0.0, 0.0, -1.0]
    assert out["t"].tolist() == [1.125] and out["n_on_plane"] == 1
    # obliquely: the box (z cell 4) is entered at t = 1 in x cell 2; the plane z = 1.125 is met at t = 1.125 exactly, 0.03125 m = an
    # eighth of a leaf from the centroid, where the plain cast gives the centroid's projection on the ray
    o, d = [[0.3125, 0.375, 0.0]], [[0.25, 0.0, 1.0]]
    plain = M.cast(ref, LEAF, o, d)
    out = N.cast_surface(ref, LEAF, o, d)
    assert out["key3"][0].tolist() == [2, 1, 4] and out["t"].tolist() == [1.125] and out["normal"][0].tolist() == [0.0, 0.0, -1.0]
    assert plain["t"][0] == F((0.3125 * 0.25 + 1.125) / 1.0625) != out["t"][0]
    for k in ("status", "key3", "count", "rgb"):
        assert np.array_equal(out[k], plain[k])
    assert out["stats"] == plain["stats"]
    # max_shift: 0.125 leaves is taken, less is not -- the normal is reported all the same
    assert N.cast_surface(ref, LEAF, o, d, max_shift=0.125)["n_on_plane"] == 1
    out = N.cast_surface(ref, LEAF, o, d, max_shift=0.0)
    assert out["n_on_plane"] == 0 and out["t"].tobytes() == plain["t"].tobytes() and out["normal"][0].tolist() == [0.0, 0.0, -1.0]
    # from above the normal keeps its sign; a ray in the plane (q = 0) keeps the plain depth
    out = N.cast_surface(ref, LEAF, [[0.3125, 0.375, 2.0]], [[0.0, 0.0, -1.0]])
    assert out["normal"][0].tolist() == [0.0, 0.0, 1.0] and out["t"].tolist() == [0.875]
    o, d = [[-1.0, 0.375, 1.125]], [[1.0, 0.0, 0.0]]
    out = N.cast_surface(ref, LEAF, o, d)
    assert out["status"].tolist() == [M.HIT] and out["n_on_plane"] == 0 and out["t"].tobytes() == M.cast(ref, LEAF, o, d)["t"].tobytes()
    assert out["normal"][0].tolist() == [0.0, 0.0, 1.0]
    # an unsupported voxel: no normal, the plain depth
    out = N.cast_surface(ref, LEAF, [[0.0625, 0.0625, 0.0]], [[0.0, 0.0, 1.0]])
    assert out["key3"][0].tolist() == [0, 0, 4] and not out["normal"].any() and out["n_on_plane"] == 0 and out["t"].tolist() == [1.125]


def test_the_host_plane_function_is_the_restatements_on_the_supports_of_a_scene():
    """rgbd360_map_plane_fit (what k_vmap_normals calls on the device) against map_align_plane_reference.plane_fit on every support of the
    room corner: the layer uses that function and no second one."""
    from rgbd360_amd import build
    L = C.CDLL(build.build())
    L.rgbd360_map_plane_fit.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    ref = R.Map([(P.corner_scene(3, size=1.0), None, R.general_pose())], 0.05, None)
    lay = N.layer(ref)
    fit = np.nonzero(lay["support"] >= 5)[0]
    assert len(fit) > 1000 and {N.OK, N.NONPLANAR} <= set(lay["status"][fit].tolist())
    want_n, want_planar, want_l0, want_l1 = P.plane_fit(lay["cov"][fit], 0.05)
    n, eig = np.zeros(3), np.zeros(2)
    for j, row in enumerate(fit):
        cov = np.ascontiguousarray(lay["cov"][row])
        planar = L.rgbd360_map_plane_fit(cov.ctypes.data_as(C.c_void_p), float(F(0.05)), n.ctypes.data_as(C.c_void_p), eig.ctypes.data_as(C.c_void_p))
        assert planar == int(want_planar[j]) == int(lay["status"][row] == N.OK)
        assert n.tobytes() == want_n[j].tobytes() and eig.tobytes() == np.array([want_l0[j], want_l1[j]]).tobytes()
        if planar:
            n32 = n.astype(F)
            assert lay["normal"][row].tobytes() in (n32.tobytes(), (-n32).tobytes())


def test_header_binding_adapter_and_example_agree():
    from rgbd360_amd import _lib, build, voxel_map
    L = C.CDLL(build.build())
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    for name in ("rgbd360_map_default_normal_params", "rgbd360_map_normals", "rgbd360_map_normals_dev", "rgbd360_map_raycast_surface",
                 "rgbd360_map_raycast_surface_sphere", "rgbd360_map_raycast_surface_sphere_dev"):
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS, name
    assert re.search(r"\brgbd360_map_time_normals\s*\(", diag) and "rgbd360_map_time_normals" not in main
    assert hasattr(L, "rgbd360_map_time_normals") and "rgbd360_map_time_normals" in _lib.SYMBOLS

    def fields(text, struct):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, text).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
        return names

    for struct, cls, size in (("rgbd360_map_normal_params", _lib.MapNormalParams, 16), ("rgbd360_map_normal_stats", _lib.MapNormalStats, 40)):
        assert fields(main, struct) == [n for n, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    assert [n for n, _ in _lib.MapNormalStats._fields_] == list(N.STAT_NAMES)
    status = {k: int(v) for k, v in re.findall(r"RGBD360_NORMAL_([A-Z_]+) = (\d)", main)}
    assert status == dict(NONE=P.NONE, OK=P.KEPT, UNSUPPORTED=P.UNSUPPORTED, NONPLANAR=P.NONPLANAR)
    assert (voxel_map.NORMAL_NONE, voxel_map.NORMAL_OK, voxel_map.NORMAL_UNSUPPORTED, voxel_map.NORMAL_NONPLANAR) == (N.NONE, N.OK, N.UNSUPPORTED, N.NONPLANAR)
    L.rgbd360_map_default_normal_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapNormalParams)]
    L.rgbd360_map_default_normal_params.restype = None
    p = _lib.MapNormalParams()
    L.rgbd360_map_default_normal_params(None, C.byref(p))
    assert (p.min_count, p.min_support) == (1, 5) and p.max_flatness == F(0.05) and p.max_shift == 2.0
    assert N.DEFAULTS == dict(min_count=p.min_count, min_support=p.min_support, max_flatness=0.05, max_shift=p.max_shift)
    # ... which are the point-to-plane alignment's
    L.rgbd360_map_default_align_plane_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapAlignPlaneParams)]
    L.rgbd360_map_default_align_plane_params.restype = None
    q = _lib.MapAlignPlaneParams()
    L.rgbd360_map_default_align_plane_params(None, C.byref(q))
    assert (q.min_count, q.min_support, q.max_flatness) == (p.min_count, p.min_support, p.max_flatness)
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("normalParams", "long long normals(", "void raycastSurface(", "void raycastSurfaceSphere(", "rgbd360_map_normals", "rgbd360_map_raycast_surface_sphere",
                 "rgbd360_map_default_normal_params"):
        assert name in hpp, name
    py = open(os.path.join(ROOT, "rgbd360_amd", "voxel_map.py")).read()
    for name in ("def normals(", "def raycast_surface(", "def raycast_surface_sphere(", "def normal_params("):
        assert name in py, name
    example = open(os.path.join(ROOT, "examples", "odometry_replay.cpp")).read()
    assert "--map-normals" in example and "--raycast-surface" in example
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "rgbd360_map_normals" in readme and "rgbd360_map_raycast_surface" in readme
    from rgbd360_amd import build as B
    assert any(d.endswith("map_normals.h") for d in B.deps()) and any(d.endswith("map_normals.h") for d in B.unit_deps("rgbd360_frame360.hip"))
    # the sentences that declared normals absent or out of scope are gone
    text = open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read()
    for gone in ("The map stores no normals", "the map holds no surface normals", "with no normals and no interpolation", "normals or shaded output"):
        assert gone not in text, gone


def sphere_scene():
    if not hasattr(sphere_scene, "ref"):
        sphere_scene.ref = R.Map([(sphere_cloud(1.5, SPHERE_POINTS), None, EYE)], 0.05, None)
    return sphere_scene.ref


def pose_at(t):
    T = EYE.copy()
    T[:3, 3] = t
    return T


def sphere_depth(origin, dirs, radius):
    """The depth at which rays from `origin` (inside) along unit `dirs` leave the sphere of `radius` around 0, in double."""
    o = np.asarray(origin, np.float64)
    d = dirs.astype(np.float64)
    b = d @ o
    return -b + np.sqrt(b * b - (o @ o - radius * radius))


def test_the_conditions_of_the_gpu_scenes_and_the_depth_error_of_the_sphere_panorama():
    """On the restatement alone.  The sphere scene at the identity and at the off-centre pose: every pixel hits, every hit voxel is OK and
    every plane depth is taken (the GPU tests compare against these panoramas, so they cannot be vacuous).  The feature's number: the RMS
    depth error of the 32 x 64 panorama, plain against surface -- against r = 1.5 at the identity, against the analytic intersection at
    the off-centre pose.  The surface cast's is at most a tenth of the plain cast's (a probe in float64 saw a fiftieth; the factor of ten
    leaves five for operation order and float32 rounding).  The four figures are printed; DESIGN.md 3.20 records them."""
    ref = sphere_scene()
    lay = N.layer(ref)
    keys = M.packed_keys(ref.key)
    for name, t in (("identity", (0.0, 0.0, 0.0)), ("off-centre", OFF_CENTRE)):
        pose = pose_at(t)
        plain = M.cast_sphere(ref, 0.05, 32, 64, pose)
        surf = N.cast_surface_sphere(ref, 0.05, 32, 64, pose)
        assert (plain["status"] == M.HIT).all() and (surf["status"] == M.HIT).all()
        rows = np.searchsorted(keys, M.packed_keys(surf["key3"].reshape(-1, 3)))
        assert (lay["status"][rows] == N.OK).all()
        assert surf["n_on_plane"] == 32 * 64 and surf["on_plane"].all()
        for k in ("key3", "count", "rgb", "status"):
            assert np.array_equal(plain[k], surf[k])
        _, dirs = M.sphere_rays(32, 64, pose)
        truth = sphere_depth(t, dirs, 1.5)
        rms = [float(np.sqrt(np.mean((out["depth"].ravel().astype(np.float64) - truth) ** 2))) for out in (plain, surf)]
        print("sphere scene, %s pose: RMS depth error plain %.3f mm, surface %.3f mm, ratio %.1f" % (name, 1e3 * rms[0], 1e3 * rms[1], rms[0] / rms[1]))
        assert rms[1] <= 0.1 * rms[0], rms
        # the normals are the sphere's, facing the camera inside it
        hit = (truth[:, None] * dirs.astype(np.float64) + np.asarray(t)) / 1.5
        cosine = -(surf["normal"].reshape(-1, 3).astype(np.float64) * hit).sum(axis=1)
        assert cosine.min() > 0.99, cosine.min()


def oblique_wall(seed=2, size=1.5, dist=1.5, step=0.01, noise=0.002):
    """A size x size wall whose centre lies `dist` m along -z, turned 35 degrees about y and 20 about x, sampled every `step` m with
    `noise` m (1 sigma) along its normal: (points float32, centre, unit normal)."""
    rng = np.random.default_rng(seed)
    g = np.arange(-size / 2, size / 2, step) + step / 2
    u, v = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    ay, ax = np.radians(35.0), np.radians(20.0)
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Rm = Ry @ Rx
    centre = np.array([0.0, 0.0, -dist])
    p = np.stack([u, v, rng.normal(0.0, noise, len(u))], axis=1) @ Rm.T + centre
    return p.astype(F), centre, Rm[:, 2]


def test_the_interior_of_a_noisy_oblique_wall_is_planar():
    pts, centre, normal = oblique_wall()
    ref = R.Map([(pts, None, EYE)], 0.05, None)
    out = N.normals(ref)
    inner = np.linalg.norm(out["xyz"].astype(np.float64) - centre, axis=1) < 0.55
    assert inner.sum() > 500 and (out["status"][inner] == N.OK).all(), np.bincount(out["status"][inner])
    cosine = np.abs(out["normal"][inner].astype(np.float64) @ normal)
    print("oblique wall: %d interior voxels, all OK; worst angle to the true normal %.2f degrees, largest curvature %.4f"
          % (inner.sum(), np.degrees(np.arccos(cosine.min())), out["curvature"][inner].max()))
    assert cosine.min() > np.cos(np.radians(10.0))
