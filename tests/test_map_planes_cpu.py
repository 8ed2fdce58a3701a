"""Planar regions of the voxel map without a device: the numpy restatement (tests/map_planes_reference.py) on hand cases around every
decision of the definition, the library's host-side plane fit (rgbd360_map_plane_from_sums, rgbd360_map_plane_from_members) against numpy's
eigh on the same integer sums, the range rule at its bound, the agreement of header, ctypes binding, adapter and example, the matcher on the
relocalisation scene, and the conditions that tests/test_map_planes_gpu.py relies on (no link of a scene within 1e-9 of a threshold, the
hull areas inside their bound)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_align_reference as A
import map_normals_reference as N
import map_planes_reference as Q
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = np.float64
EYE = np.eye(4, dtype=np.float32)
LEAF = 0.25
SMALL = dict(min_voxels=20)        # the scenes' patches are 5 x 5 and 8 x 8 cells: below the default of 50


def make_map(points, leaf=LEAF):
    return R.Map([(np.asarray(points, F), None, EYE)], leaf, box=None)


class HandMap:
    """A map given as rows, one point per voxel; the rows are put in key order."""

    def __init__(self, keys, xyz):
        key = np.asarray(keys, np.int32).reshape(-1, 3)
        order = np.argsort(A.packed_keys(key), kind="stable")
        self.key, self.xyz, self.count = key[order], np.asarray(xyz, F).reshape(-1, 3)[order], np.ones(len(key), np.int64)

    def __len__(self):
        return len(self.count)


def flat_layer(ref, normals=None):
    """A hand-made normal layer: every voxel OK with the given normal (z where none is given) and curvature 0."""
    k = len(ref)
    n = np.tile(F([0, 0, 1]), (k, 1)) if normals is None else np.asarray(normals, F).reshape(k, 3)
    return dict(status=np.full(k, N.OK, np.int32), normal=n, curvature=np.zeros(k, F))


def scenes():
    """The GPU suite's scenes: name -> (points, leaf, parameters)."""
    bridge = np.concatenate([Q.patch((0, 0, 0), (1, 0, 0), (0, 1, 0), 4, 5), Q.patch((1.0, 0.5, 0), (1, 0, 0), (0, 1, 0), 1, 1),
                             Q.patch((1.25, 0, 0), (1, 0, 0), (0, 1, 0), 4, 5)]) + F([0, 0, 0.125])
    return {"patch": (Q.patch((0, 0, 0.125), (1, 0, 0), (0, 1, 0), 5, 5), LEAF, SMALL),
            "bridge": (bridge, LEAF, dict(min_voxels=5)),
            "corner": (Q.corner_scene(), LEAF, SMALL),
            "spiral": (Q.spiral_scene()[0], LEAF, {}),
            "patches": (Q.patches_scene(), LEAF, dict(SMALL, max_planes=64))}


@pytest.fixture(scope="module")
def room():
    """The relocalisation scene as two restated maps: A of the world points, B of the same points in the frame at Q.frame_pose()."""
    pts, T = Q.room_scene(), Q.frame_pose()
    a, b = make_map(pts, 0.1), make_map(Q.in_frame(pts, T), 0.1)
    return dict(points=pts, T=T, A=a, B=b, planes_a=Q.planes(a, 0.1), planes_b=Q.planes(b, 0.1))


# ---- the restatement on hand cases
def test_a_patch_is_one_region_rooted_at_its_smallest_key():
    ref = make_map(Q.patch((0.5, -0.75, 0.125), (1, 0, 0), (0, 1, 0), 5, 5))
    S = Q.segment(ref, LEAF, min_support=4)            # the corners have four cells around them
    assert S["eligible"].all() and len(S["regions"]) == 1
    g = S["regions"][0]
    assert g["row"] == 0 and g["n_voxels"] == 25 and (S["root"] == 0).all() and tuple(ref.key[0]) == (2, -3, 0)
    assert S["n_links"] == 2 * 5 * 4 + 2 * 4 * 4       # 40 along the axes, 32 diagonal
    assert g["extent"] == 4 and g["sums"][0] == 25 * 2 * 16384 and g["sums"][2] == 0
    S5 = Q.segment(ref, LEAF)                          # min_support 5: the four corners have no normal and carry their own key
    assert S5["eligible"].sum() == 21 and len(S5["regions"]) == 1 and S5["regions"][0]["row"] == 1
    out = Q.planes(ref, LEAF, **SMALL)
    assert (out["plane_index"][S5["eligible"]] == 0).all() and (out["plane_index"][~S5["eligible"]] == -1).all()
    assert np.array_equal(out["label_key3"][~S5["eligible"]], ref.key[~S5["eligible"]]) and np.array_equal(out["root_key3"], ref.key[1:2])


def test_a_bridge_of_one_voxel_joins_two_patches_and_its_absence_parts_them():
    pts, leaf, P = scenes()["bridge"]
    ref = make_map(pts)
    S = Q.segment(ref, leaf, **P)
    assert len(ref) == 41 and len(S["regions"]) == 1
    row = int(np.nonzero((ref.key == (4, 2, 0)).all(axis=1))[0][0])
    assert S["eligible"][row]
    ref.count[row] = 0                                 # a tombstone: absent everywhere
    S = Q.segment(ref, leaf, **P)
    assert len(S["regions"]) == 2 and not S["eligible"][row]
    assert [g["n_voxels"] for g in S["regions"]] == [16, 16] and S["eligible"].sum() == 32      # 4 x 5 cells less their corners, twice


def test_a_step_of_one_leaf_links_at_equality_and_not_below():
    # two rows of cells, the second one leaf higher, every normal z by hand: |n . e| is exactly one leaf
    keys = [(x, 0, 0) for x in range(4)] + [(x, 1, 1) for x in range(4)]
    xyz = [((x + 0.5) * LEAF, 0.125, 0.0) for x in range(4)] + [((x + 0.5) * LEAF, 0.375, 0.25) for x in range(4)]
    ref = HandMap(keys, xyz)
    at = Q.segment(ref, LEAF, flat_layer(ref), max_offset=1.0)
    below = Q.segment(ref, LEAF, flat_layer(ref), max_offset=float(np.nextafter(F(1.0), F(0))))
    assert len(at["regions"]) == 1 and at["margin"] == 0.0
    assert len(below["regions"]) == 2 and [g["n_voxels"] for g in below["regions"]] == [4, 4]
    assert at["n_links"] == below["n_links"] + 4 + 3 + 3


def test_an_angle_links_on_either_side_of_cos_angle():
    # two rows of cells with the normals (0, 0, 1) and (0.6, 0, 0.8) by hand: the cosine is the float32 0.8 exactly (0.8f x 1.0)
    keys = [(x, 0, 0) for x in range(4)] + [(x, 1, 0) for x in range(4)]
    xyz = [((x + 0.5) * LEAF, 0.125, 0.125) for x in range(4)] + [((x + 0.5) * LEAF, 0.375, 0.125) for x in range(4)]
    ref = HandMap(keys, xyz)
    normals = [(0, 0, 1)] * 4 + [(0.6, 0, 0.8)] * 4
    c = float(F(0.8))
    at = Q.segment(ref, LEAF, flat_layer(ref, normals), cos_angle=c, max_offset=4.0)
    above = Q.segment(ref, LEAF, flat_layer(ref, normals), cos_angle=float(np.nextafter(F(0.8), F(1))), max_offset=4.0)
    assert len(at["regions"]) == 1 and len(above["regions"]) == 2
    # the absolute value: a flipped normal links all the same
    flipped = Q.segment(ref, LEAF, flat_layer(ref, [(0, 0, 1)] * 4 + [(-0.6, 0, -0.8)] * 4), cos_angle=c, max_offset=4.0)
    assert len(flipped["regions"]) == 1


def test_a_room_corner_is_three_regions_and_its_edges_carry_no_label():
    pts, leaf, P = scenes()["corner"]
    ref = make_map(pts)
    out = Q.planes(ref, leaf, **P)
    S = out["segmentation"]
    assert len(S["regions"]) == 3 and out["stats"]["n_planes_available"] == 3 and [p["n_voxels"] for p in out["planes"]] == [35, 35, 35]
    on_edge = (ref.key == 0).sum(axis=1) >= 2          # on two of the three planes
    assert on_edge.sum() == 22 and not S["eligible"][on_edge].any() and (out["plane_index"][on_edge] == -1).all()
    normals = np.array([p["normal"] for p in out["planes"]])
    assert np.allclose(np.abs(normals).sum(axis=0), 1, atol=1e-6) and np.allclose(np.abs(normals).max(axis=1), 1, atol=1e-6)
    assert all(np.dot(p["normal"], p["centroid"]) < 0 for p in out["planes"])      # towards the origin


def test_a_neighbour_index_outside_the_key_range_does_not_exist():
    # the +x neighbour of the last cell has no 21-bit index; packed carelessly it is the key of the first cell of the next row
    top, low = (1 << 20) - 1, -(1 << 20)
    ref = HandMap([(top, 0, 0), (low, 1, 0)], [(4000.0, 0.1, 0.1), (-4000.0, 0.3, 0.1)])
    assert A.packed_keys(ref.key)[0] + 1 == A.packed_keys(ref.key)[1]
    S = Q.segment(ref, LEAF, flat_layer(ref), max_offset=1e9)
    assert S["n_links"] == 0 and len(S["regions"]) == 2


def test_min_voxels_and_max_planes_cut_with_their_tie_rules():
    # four patches by ascending root key with 21, 26, 21 and 26 eligible voxels (5 x 5, 5 x 6, 5 x 5, 5 x 6)
    sizes = [(5, 5), (5, 6), (5, 5), (5, 6)]
    pts = np.concatenate([Q.patch((0, k * 2.0, 0.125), (1, 0, 0), (0, 1, 0), a, b) for k, (a, b) in enumerate(sizes)])
    ref = make_map(pts)
    every = Q.planes(ref, LEAF, min_voxels=21)
    assert [p["n_voxels"] for p in every["planes"]] == [21, 26, 21, 26] and every["stats"]["n_planes_available"] == 4
    assert [p["n_voxels"] for p in Q.planes(ref, LEAF, min_voxels=22)["planes"]] == [26, 26]
    three = Q.planes(ref, LEAF, min_voxels=21, max_planes=3)        # the two of 26, and of the two of 21 the smaller root key
    assert np.array_equal(three["root_key3"], every["root_key3"][[0, 1, 3]]) and [p["root"] for p in three["planes"]] == [0, 1, 2]
    one = Q.planes(ref, LEAF, min_voxels=21, max_planes=1)
    assert np.array_equal(one["root_key3"], every["root_key3"][[1]]) and one["stats"] == every["stats"]
    assert np.array_equal(three["plane_index"], every["plane_index"]) and Q.planes(ref, LEAF, min_voxels=21, max_planes=0)["planes"] == []


# ---- the library's host side
def lib():
    from rgbd360_amd import _lib
    return _lib, _lib.load()


def library_plane(L, _lib, g, ref, viewpoint=None, members=True):
    pl = _lib.Plane()
    r = np.ascontiguousarray(ref.xyz[g["row"]], F)
    s = np.ascontiguousarray(g["sums"], np.int64)
    v = None if viewpoint is None else np.ascontiguousarray(viewpoint, F)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    if members:
        xyz, key3 = np.ascontiguousarray(ref.xyz[g["members"]], F), np.ascontiguousarray(ref.key[g["members"]], np.int32)
        assert L.rgbd360_map_plane_from_members(g["n_voxels"], g["n_points"], vp(r), vp(s), vp(xyz), vp(key3), vp(v), C.byref(pl)) == 0
    else:
        assert L.rgbd360_map_plane_from_sums(g["n_voxels"], g["n_points"], vp(r), vp(s), vp(v), C.byref(pl)) == 0
    return pl


def assert_plane_close(pl, fit, what):
    """centroid and d within 4 float32 ulps of their magnitude; the normal within 2 float32 ulps per component (a component below 2^-20:
    2 ulps of 2^-20 -- the two float64 eigenvectors agree to about 1e-15, many ulps of a component that is itself 1e-17)."""
    c, n = np.array(list(pl.centroid), F), np.array(list(pl.normal), F)
    assert np.abs(c.astype(D) - fit["centroid"]).max() <= 4 * np.spacing(F(np.linalg.norm(fit["centroid"]))), what
    assert abs(D(pl.d) - fit["d"]) <= 4 * np.spacing(F(abs(fit["d"]))), what
    tol = 2 * np.spacing(np.maximum(np.abs(fit["normal"]), 2.0 ** -20).astype(F)).astype(D)
    assert (np.abs(n.astype(D) - fit["normal"]) <= tol).all(), (what, n, fit["normal"])
    assert 1 - abs(float(n.astype(D) @ fit["normal"])) <= 1e-7 and pl.count == fit["count"]


def test_plane_from_sums_agrees_with_eigh_on_the_same_sums(room):
    _lib, L = lib()
    cases = [(name, make_map(pts, leaf), leaf, P) for name, (pts, leaf, P) in scenes().items()] + [("room A", room["A"], 0.1, {}), ("room B", room["B"], 0.1, {})]
    n = 0
    for name, ref, leaf, P in cases:
        out = Q.planes(ref, leaf, **P) if not name.startswith("room") else room["planes_" + name[-1].lower()]
        for view in (None, (0.3, -0.2, 5.0)):
            for pl_ref in out["planes"]:
                g = next(g for g in out["segmentation"]["regions"] if g["row"] == pl_ref["root_row"])
                fit = Q.plane_from_sums(g["n_voxels"], g["n_points"], ref.xyz[g["row"]], g["sums"], view)
                for members in (False, True):
                    pl = library_plane(L, _lib, g, ref, view, members)
                    assert_plane_close(pl, fit, (name, g["row"], members))
                    assert abs(pl.curvature - fit["curvature"]) <= 1e-9 and pl.color_count == 0 and pl.color_mode_count == 0
                    assert abs(pl.area_moment - fit["area_moment"]) <= 1e-5 * fit["area_moment"]
                    assert (pl.hull_n == 0 and pl.area == pl.area_moment) if not members else pl.hull_n >= 3
                n += 1
    assert n >= 2 * (1 + 1 + 3 + 1 + 64 + 9 + 9)
    assert L.rgbd360_map_plane_from_sums(0, 0, None, None, None, None) == -1


def test_the_range_rule_at_and_beyond_its_bound():
    _lib, L = lib()
    # leaf 0.25: b = (E + 2) 2^14, so N (E + 2)^2 < 2^34 -- with E + 2 = 2^10 the last N in range is 2^14 - 1
    for n, e, want in ((16383, 1022, 1), (16384, 1022, 0), (16384, 1021, 1), (1, (1 << 17) - 3, 1), (1, (1 << 17) - 2, 0), (1 << 30, 2, 0), (1 << 30, 1, 1)):
        assert L.rgbd360_map_plane_sums_in_range(n, e, 0.25) == want == int(Q.sums_in_range(n, e, 0.25)), (n, e)
    assert Q.sums_in_range(100000, 1000, 0.1) and not Q.sums_in_range(1000000, 1000, 0.1)
    # the sums of a region in range can not leave int64: |q| <= (E + 1) leaf 2^16 + 1 < b
    assert 16383 * ((1022 + 2) * 0.25 * 65536) ** 2 < 2 ** 62


# ---- header, binding, adapters
def test_header_binding_adapter_and_example_agree():
    _lib, L = lib()
    hdr = open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read()
    assert C.sizeof(_lib.MapPlaneSegParams) == 32 and C.sizeof(_lib.MapPlaneSegStats) == 48
    fields = re.search(r"typedef struct \{([^}]*)\} rgbd360_map_plane_seg_params;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    assert re.findall(r"(\w+);", fields) == [n for n, _ in _lib.MapPlaneSegParams._fields_] == list(Q.DEFAULTS)
    assert [n for n, _ in _lib.MapPlaneSegStats._fields_] == list(Q.STAT_NAMES)
    p = _lib.MapPlaneSegParams()
    L.rgbd360_map_default_plane_seg_params(None, C.byref(p))
    assert {n: getattr(p, n) for n in Q.DEFAULTS} == {n: (v if isinstance(v, int) else float(F(v))) for n, v in Q.DEFAULTS.items()}
    table = re.search(r"RGBD360_MAP_PLANE_DIRS\[64\]\[2\] = \{(.*?)\};", hdr, flags=re.S).group(1)
    dirs = np.array(re.findall(r"-?\d+", table), np.int64).reshape(64, 2)
    assert np.array_equal(dirs, Q.DIRS) and np.array_equal(dirs, np.array(_lib.MAP_PLANE_DIRS))
    k = np.arange(64) * (2 * np.pi / 64)
    assert np.abs(dirs - 1024 * np.stack([np.cos(k), np.sin(k)], axis=1)).max() <= 0.5
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("planeSegParams", "planes", "planeLabels", "planeSegStats", "relocalize", "planeBytes", "releasePlanes", "Relocalizer360"):
        assert name in hpp, name
    assert "--map-planes" in open(os.path.join(ROOT, "examples", "odometry_replay.cpp")).read()
    from rgbd360_amd.voxel_map import VoxelMap
    for name in ("plane_seg_params", "planes", "plane_labels", "relocalize", "release_planes", "plane_bytes"):
        assert callable(getattr(VoxelMap, name))


# ---- what the GPU scenes rely on
def test_no_link_of_a_gpu_scene_lies_near_a_threshold(room):
    """The bit equality of tests/test_map_planes_gpu.py is honest only where no pair of voxels sits on a threshold of the link predicate,
    and no region on max_curvature or min_voxels by less than the two fits differ."""
    for name, (pts, leaf, P) in scenes().items():
        out = Q.planes(make_map(pts, leaf), leaf, **P)
        assert out["segmentation"]["margin"] > 1e-9, name
        assert all(p["curvature"] < 1e-9 for p in out["planes"]), name
    coarse = Q.planes(make_map(scenes()["corner"][0], 2 * LEAF), 2 * LEAF, min_voxels=3)      # the corner as level 1 of its pyramid
    assert coarse["segmentation"]["margin"] > 1e-9 and coarse["stats"]["n_planes_available"] == 3
    for name in ("planes_a", "planes_b"):
        S = room[name]["segmentation"]
        assert S["margin"] > 1e-9, name
        curv = [Q.plane_from_sums(g["n_voxels"], g["n_points"], (0, 0, 0), g["sums"])["curvature"] for g in S["regions"] if g["n_voxels"] >= 50]
        assert all(abs(c - float(F(0.0013))) > 1e-9 for c in curv), name
    assert Q.spiral_scene()[1] >= 200 and 600 < len(make_map(Q.spiral_scene()[0])) < 0.7 * 1024
    assert len(make_map(Q.patches_scene())) == 65 * 25 and len(make_map(scenes()["patch"][0])) == 25


def hull_area_of_all_members(ref, pl):
    """The area of the convex hull of every member centroid projected on the restated plane."""
    fit = pl["fit"]
    d = ref.xyz[pl["members"]].astype(D) - fit["centroid"][None, :]
    poly = Q.convex_hull(np.stack([d @ fit["e1"], d @ fit["e2"]], axis=1))
    return Q.polygon_area_centre(poly)[0]


def test_the_hull_areas_of_the_scenes_stay_inside_their_bound(room):
    """0.99 A_ref <= area <= A_ref (1 + 1e-5) for the inscribed polygon of 64 directions, on the restatement and on the library's host
    hull of the same members."""
    _lib, L = lib()
    cases = [(make_map(pts, leaf), Q.planes(make_map(pts, leaf), leaf, **P)) for name, (pts, leaf, P) in scenes().items() if name != "patches"]
    cases += [(room["A"], room["planes_a"]), (room["B"], room["planes_b"])]
    for ref, out in cases:
        for pl in out["planes"]:
            a_ref = hull_area_of_all_members(ref, pl)
            g = next(g for g in out["segmentation"]["regions"] if g["row"] == pl["root_row"])
            got = library_plane(L, _lib, g, ref)
            for area in (pl["area"], got.area):
                assert 0.99 * a_ref <= area <= a_ref * (1 + 1e-5), (pl["n_voxels"], area, a_ref)
            # the vertices are projections of member centroids, counter-clockwise seen from the normal's side
            hull = np.array([list(got.hull[k]) for k in range(got.hull_n)], D)
            n = np.array(list(got.normal), D)
            assert np.abs((hull - np.array(list(got.centroid), D)) @ n).max() < 1e-5
            turn = np.cross(np.roll(hull, -1, axis=0) - hull, np.roll(hull, -2, axis=0) - np.roll(hull, -1, axis=0)) @ n
            assert (turn > 0).all()


def test_the_matcher_accepts_the_relocalisation_scene(room):
    """The room segments into its nine faces in both maps; register_planes (host code) accepts the pair, and its pose moves no point of the
    cloud by more than half the capture range of coarse-to-fine ICP (2^top_shift leaves)."""
    from rgbd360_amd import pbmap
    _lib, L = lib()
    for name in ("planes_a", "planes_b"):
        assert room[name]["stats"]["n_planes_available"] == 9 and len(room[name]["planes"]) == 9, name
    assert room["planes_a"]["stats"]["n_regions"] == 9 and 3000 < len(room["A"]) < 10000
    got = relocalize_restated(room)
    assert got["status"] == 0 and len(got["match"]) == 9
    c2f = _lib.MapC2fParams()
    L.rgbd360_map_default_c2f_params(None, C.byref(c2f))
    moved = np.linalg.norm(room["points"].astype(D) @ (got["pose"][:3, :3].astype(D) - room["T"][:3, :3]).T + (got["pose"][:3, 3] - room["T"][:3, 3]), axis=1)
    print("relocalisation: matches", got["match"], "largest displacement", moved.max(), "m")
    assert moved.max() <= 0.5 * (1 << c2f.top_shift) * 0.1


def library_planes(ref, out, viewpoint=None):
    """The records the library builds on the host for the restated regions of `out`, as plane dicts: byte for byte what rgbd360_map_planes
    returns on the device for the same map."""
    from rgbd360_amd.register import _planes_to_dicts
    _lib, L = lib()
    arr = (_lib.Plane * max(len(out["planes"]), 1))()
    for o, pl in enumerate(out["planes"]):
        g = next(g for g in out["segmentation"]["regions"] if g["row"] == pl["root_row"])
        arr[o] = library_plane(L, _lib, g, ref, viewpoint)
        arr[o].root = o
    return arr, _planes_to_dicts(arr, len(out["planes"]))


def relocalize_restated(room):
    from rgbd360_amd import pbmap
    return pbmap.register_planes(library_planes(room["A"], room["planes_a"])[1], library_planes(room["B"], room["planes_b"])[1])
