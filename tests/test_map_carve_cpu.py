"""CPU tests of free-space observation and carving of the voxel map: the numpy restatement (tests/map_carve_reference.py) against answers
derived by hand -- a voxel midway, the endpoint's voxel, the margin, the voxel behind the endpoint, the near rule, the offset rule, the
corner-diagonal tie rule, negative coordinates, margin_rel, invalid measurements, d = 0 -- the vote layer (accumulation, the two forms of
the walk, the carve's thresholds, the carved map), the functional scene (a phantom box in the synthetic room), and the agreement of the
header, the ctypes binding and the C++ adapter.

The hand cases use cells of 0.05 m (inv_leaf = 20 exactly) and one point per voxel at the cell's centre; the rays run through cell
centres, and every case keeps clear of the thresholds by a fifth of a leaf or more, so that no rounding decides it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_carve_reference as V
import map_raycast_reference as M
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
F = np.float32
LEAF = 0.05
H = 0.025       # half a cell


def centre(cell):
    return [(c + 0.5) * LEAF for c in cell]


def centres(cells, extra=()):
    """A map of one point per cell at the cell's centre, and the points of `extra` as they are."""
    xyz = np.array([centre(cell) for cell in cells] + [list(p) for p in extra], F)
    return R.Map([(xyz, None, EYE)], LEAF, None)


def voted(ref, ob):
    """{cell: (through, end)} of the voxels with a vote."""
    key3, through, end, _ = V.votes(ref, ob)
    return {tuple(k): (int(t), int(e)) for k, t, e in zip(key3.tolist(), through.tolist(), end.tolist())}


def one(ref, o, w, **params):
    ob = V.observe_rays(ref, LEAF, np.array([o], F), np.array([w], F), **params)
    return voted(ref, ob), ob["stats"]


def test_midway_endpoint_margin_behind_and_near():
    """From the centre of cell 0 to the centre of cell 20 along x, |d| = 1 m: cell k's centre lies at t = k / 20."""
    cells = [(k, 0, 0) for k in (0, 2, 10, 17, 19, 20, 22)]
    ref = centres(cells)
    got, stats = one(ref, centre((0, 0, 0)), centre((20, 0, 0)))
    # 0: the origin's own voxel, th = 0 < near.  2, 10, 17: 0.1, 0.5 and 0.85 m along, at least 0.15 m in front of the measurement.
    # 19: 0.05 m in front of it, inside the margin of 0.1 m.  20: the measured voxel, th = 1, q = 0: the end-vote alone.
    # 22: behind the measurement; the walk ends at cell 21, whose entry lies at t = 1.025 > 1.
    assert got == {(2, 0, 0): (1, 0), (10, 0, 0): (1, 0), (17, 0, 0): (1, 0), (20, 0, 0): (0, 1)}
    assert stats == dict(n_rays=1, n_valid=1, n_skipped=0, n_miss_box=0, n_max_steps=0, n_steps=21, n_lookups=6, n_through=3, n_end=1, n_voxels_voted=4)
    assert one(ref, centre((0, 0, 0)), centre((20, 0, 0)), layer=False)[1]["n_lookups"] == 21
    # near = 0.12 m drops cell 2 as well; near = 0 takes the origin's voxel in
    assert (2, 0, 0) not in one(ref, centre((0, 0, 0)), centre((20, 0, 0)), near=0.12)[0]
    assert one(ref, centre((0, 0, 0)), centre((20, 0, 0)), near=0.0)[0][(0, 0, 0)] == (1, 0)
    # a margin of 0.5 leaves lets cell 19 in; one of 4 leaves (0.2 m) drops cell 17
    assert one(ref, centre((0, 0, 0)), centre((20, 0, 0)), margin_leaves=0.5)[0][(19, 0, 0)] == (1, 0)
    assert (17, 0, 0) not in one(ref, centre((0, 0, 0)), centre((20, 0, 0)), margin_leaves=4.0)[0]
    # min_count: single points are not voted on by a call that asks for two; the end-vote only needs a live voxel
    assert one(ref, centre((0, 0, 0)), centre((20, 0, 0)), min_count=2)[0] == {(20, 0, 0): (0, 1)}
    # max_steps: the walk ends after three cells, before cell 10; the end-vote is given all the same
    got, stats = one(ref, centre((0, 0, 0)), centre((20, 0, 0)), max_steps=3)
    assert got == {(2, 0, 0): (1, 0), (20, 0, 0): (0, 1)} and stats["n_max_steps"] == 1 and stats["n_steps"] == 3
    # a measurement that no voxel holds gives no end-vote
    got, stats = one(ref, centre((0, 0, 0)), centre((15, 0, 0)))
    assert got == {(2, 0, 0): (1, 0), (10, 0, 0): (1, 0)} and stats["n_end"] == 0


def test_the_offset_rule():
    """The ray runs 0.1 leaf above the cells' lower face: a centroid 0.6 leaves off it is not voted, one at 0.4 leaves is."""
    pts = [(10.5 * LEAF, 0.005 + 0.6 * LEAF, H), (12.5 * LEAF, 0.005 + 0.4 * LEAF, H)]
    ref = centres([(20, 0, 0)], pts)
    assert sorted(map(tuple, ref.key.tolist())) == [(10, 0, 0), (12, 0, 0), (20, 0, 0)]
    o, w = [H, 0.005, H], [20.5 * LEAF, 0.005, H]
    assert one(ref, o, w)[0] == {(12, 0, 0): (1, 0), (20, 0, 0): (0, 1)}
    assert one(ref, o, w, max_offset=0.7)[0] == {(10, 0, 0): (1, 0), (12, 0, 0): (1, 0), (20, 0, 0): (0, 1)}
    assert one(ref, o, w, max_offset=0.3)[0] == {(20, 0, 0): (0, 1)}


def test_the_corner_diagonal_pins_the_tie_rule():
    """From the centre of cell (0, 0, 0) to the centre of (20, 20, 20) all three boundary times are equal at every corner: x steps first,
    then y, then z.  Between (9, 9, 9) and (10, 10, 10) the segment visits (10, 9, 9) and (10, 10, 9) and none of the other four cells that
    touch the corner.  (The offset rule is off: those centres lie 0.8 leaves from the diagonal.)"""
    around = [(10, 9, 9), (10, 10, 9), (9, 10, 9), (9, 9, 10), (9, 10, 10), (10, 9, 10)]
    ref = centres(around + [(0, 0, 0), (20, 20, 20)])
    got, stats = one(ref, centre((0, 0, 0)), centre((20, 20, 20)), max_offset=np.inf)
    assert got == {(10, 9, 9): (1, 0), (10, 10, 9): (1, 0), (20, 20, 20): (0, 1)}
    assert stats["n_steps"] == 61          # cells (0,0,0) .. (20,20,20): three per corner
    assert one(ref, centre((0, 0, 0)), centre((20, 20, 20)))[0] == {(20, 20, 20): (0, 1)}
    # and with negative steps: y before z
    ref = centres([(0, -10, -9), (0, -9, -10), (0, 0, 0), (0, -20, -20)])
    got, _ = one(ref, centre((0, 0, 0)), centre((0, -20, -20)), max_offset=np.inf)
    assert got == {(0, -10, -9): (1, 0), (0, -20, -20): (0, 1)}


def test_negative_coordinates_and_margin_rel():
    ref = centres([(-1, -1, -1), (-11, -1, -1), (-16, -1, -1), (-18, -1, -1), (-21, -1, -1)])
    o, w = centre((-1, -1, -1)), centre((-21, -1, -1))
    assert one(ref, o, w)[0] == {(-11, -1, -1): (1, 0), (-16, -1, -1): (1, 0), (-18, -1, -1): (1, 0), (-21, -1, -1): (0, 1)}
    # -0.01 lies in cell -1 (floor, not truncation): the end-vote goes there
    ref2 = centres([(-1, -1, -1)])
    assert one(ref2, [0.5, -H, -H], [-0.01, -H, -H])[0] == {(-1, -1, -1): (0, 1)}
    # margin_rel = 0.2 of the range 1 m, no fixed margin: -16 (0.25 in front) stays, -18 (0.15 in front) goes
    assert one(ref, o, w, margin_leaves=0.0, margin_rel=0.2)[0] == {(-11, -1, -1): (1, 0), (-16, -1, -1): (1, 0), (-21, -1, -1): (0, 1)}
    # both margins add: 0.1 + 0.2 = 0.3 m drops -16 as well
    assert one(ref, o, w, margin_rel=0.2)[0] == {(-11, -1, -1): (1, 0), (-21, -1, -1): (0, 1)}


def test_invalid_measurements_and_empty_inputs():
    ref = centres([(0, 0, 0), (10, 0, 0), (20, 0, 0)])
    o = np.array([centre((0, 0, 0))] * 8, F)
    w = np.array([centre((20, 0, 0))] * 8, F)
    w[1, 1] = np.nan
    w[2, 0] = 4096.0
    o[3, 2] = np.inf
    w[4] = o[4]                 # d = 0
    w[5, 0] = -np.inf
    o[6, 0] = np.nan
    w[7] = (np.nextafter(F(4096.0), F(0)), H, H)       # the last float in range: valid, leaves the box
    ob = V.observe_rays(ref, LEAF, o, w)
    assert ob["stats"] == dict(n_rays=8, n_valid=2, n_skipped=6, n_miss_box=0, n_max_steps=0, n_steps=21 + 21, n_lookups=3 + 3, n_through=3, n_end=1,
                               n_voxels_voted=2)
    # (the long ray passes cell 20 far in front of its own measurement: a through-vote next to the first ray's end-vote)
    assert voted(ref, ob) == {(10, 0, 0): (2, 0), (20, 0, 0): (1, 1)}
    empty = R.Map([], LEAF, None)
    ob = V.observe_rays(empty, LEAF, o, w)
    assert ob["stats"] == dict.fromkeys(V.STAT_NAMES, 0) and len(ob["through"]) == 0
    ob = V.observe_rays(ref, LEAF, np.zeros((0, 3), F), np.zeros((0, 3), F))
    assert ob["stats"] == dict.fromkeys(V.STAT_NAMES, 0) and not ob["through"].any()
    # a sphere frame: a pixel whose point is not finite is skipped; the box of the map plays no part
    xyz = np.array([[1.0, 0, 0], [np.nan, 0, 0], [0, 0, 5000.0]], F)
    T = EYE.copy()
    T[:3, 3] = centre((0, 0, 0))
    ob = V.observe_cloud(ref, LEAF, xyz, T)
    assert (ob["stats"]["n_rays"], ob["stats"]["n_valid"], ob["stats"]["n_skipped"]) == (3, 1, 2) and voted(ref, ob) == {(10, 0, 0): (1, 0), (20, 0, 0): (0, 1)}


def blob(n_points=10000, seed=3):
    """~5000 voxels in a 2 m cube around the origin, one to a dozen points each: (points, the map)."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1.0, 1.0, size=(n_points // 4, 3))
    pts = (base[:, None, :] + rng.normal(scale=0.01, size=(len(base), 4, 3))).reshape(-1, 3).astype(F)
    return pts, R.Map([(pts, None, EYE)], LEAF, None)


def segments(n, pts, seed=11):
    """n segments through the blob from a point outside or inside the cube; every other one ends on a point of the blob (its voxel gets the
    end-vote), the rest end anywhere in the cube."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.6, 1.6, size=(n, 3)).astype(F)
    w = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(F)
    w[::2] = pts[rng.integers(0, len(pts), size=len(w[::2]))]
    return o, w


@pytest.fixture(scope="module")
def blob_votes():
    pts, ref = blob()
    o, w = segments(600, pts)
    return dict(pts=pts, ref=ref, o=o, w=w, ob=V.observe_rays(ref, LEAF, o, w))


def test_accumulation_and_the_two_forms_of_the_walk(blob_votes):
    ref, o, w, whole = (blob_votes[k] for k in ("ref", "o", "w", "ob"))
    assert 4000 < len(ref) < 6000 and ref.key.min() < -15 and ref.key.max() > 15
    assert whole["stats"]["n_through"] > 500 and whole["stats"]["n_end"] > 100 and whole["through"].max() > 1
    a, b = V.observe_rays(ref, LEAF, o[:250], w[:250]), V.observe_rays(ref, LEAF, o[250:], w[250:])
    both = V.add(a, b)
    assert np.array_equal(both["through"], whole["through"]) and np.array_equal(both["end"], whole["end"])
    assert a["stats"]["n_voxels_voted"] + both["stats"]["n_voxels_voted"] == whole["stats"]["n_voxels_voted"]
    plain = V.observe_rays(ref, LEAF, o, w, layer=False)
    assert np.array_equal(plain["through"], whole["through"]) and np.array_equal(plain["end"], whole["end"])
    assert plain["stats"]["n_lookups"] == plain["stats"]["n_steps"] > whole["stats"]["n_lookups"]
    assert {k: v for k, v in plain["stats"].items() if k != "n_lookups"} == {k: v for k, v in whole["stats"].items() if k != "n_lookups"}


def test_carve_thresholds_and_the_carved_map(blob_votes):
    pts, ref, ob = blob_votes["pts"], blob_votes["ref"], blob_votes["ob"]
    t, e = ob["through"], ob["end"]
    erased, stats = V.carve(ref, ob)
    assert np.array_equal(erased, (t >= 1) & (e == 0))
    assert stats == dict(n_voted=int(((t + e) > 0).sum()), n_voxels_carved=int(erased.sum()), n_points_carved=int(ref.count[erased].sum()),
                         n_protected_end=int(((t >= 1) & (e > 0)).sum()), n_protected_count=0, n_voxels=len(ref) - int(erased.sum()))
    assert stats["n_voxels_carved"] > 500 and stats["n_protected_end"] > 10
    two, stats2 = V.carve(ref, ob, min_through=2)
    assert np.array_equal(two, (t >= 2) & (e == 0)) and 0 < stats2["n_voxels_carved"] < stats["n_voxels_carved"]
    lax, stats3 = V.carve(ref, ob, max_end=1)
    assert np.array_equal(lax, (t >= 1) & (e <= 1)) and stats3["n_voxels_carved"] > stats["n_voxels_carved"]
    small, stats4 = V.carve(ref, ob, max_count=4)
    assert np.array_equal(small, erased & (ref.count <= 4)) and stats4["n_protected_count"] == int((erased & (ref.count > 4)).sum()) > 0
    # the carved map is the map of the points outside the carved voxels
    i = R.voxel_index(pts, LEAF)
    pk = ((i[:, 2] + R.BIAS) << 42) | ((i[:, 1] + R.BIAS) << 21) | (i[:, 0] + R.BIAS)
    keep = ~np.isin(pk, M.packed_keys(ref.key[erased]))
    want = R.Map([(pts[keep], None, EYE)], LEAF, None)
    got = V.without(ref, erased)
    assert len(got) == len(want) == stats["n_voxels"] and (~keep).sum() == stats["n_points_carved"] == V.points_in(ref, erased, pts, EYE, LEAF, None)
    R.assert_map_equals((got.xyz, got.rgb, got.count, got.key), want)
    # the read-out after the carve: the carved voxels read count 0
    key3, through, end, count = V.votes(ref, ob, erased)
    assert len(key3) == stats["n_voted"] and int((count == 0).sum()) == stats["n_voxels_carved"]


def phantom_scene(sphere_cloud, width=64, height=32, observer=1, n_frames=3):
    """The synthetic room seen from `n_frames` poses of its trajectory (their convention-2 clouds at the true poses, no box), and a phantom
    box of points that no frame contains: a 0.3 m cube of points 0.9 m from the observer's pose, in the room's free space.
    Returns (ref of room + phantom, is_phantom mask over ref, the observer's cloud and pose)."""
    from rgbd360_amd import synth
    frames = []
    for k in range(n_frames):
        T = synth.trajectory_pose(k)
        rgb, depth = synth.render(T, width, height)
        frames.append((sphere_cloud(depth), rgb.reshape(-1, 3), T.astype(F)))
    room = R.Map(frames, LEAF, None)
    rng = np.random.default_rng(5)
    mid = synth.trajectory_pose(observer)[:3, 3] + np.array([0.2, 0.5, 0.7])
    box = (mid[None, :] + rng.uniform(-0.15, 0.15, size=(4000, 3))).astype(F)
    ref = R.Map(frames + [(box, None, EYE)], LEAF, None)
    is_phantom = ~np.isin(M.packed_keys(ref.key), M.packed_keys(room.key))
    return ref, is_phantom, frames[observer][0], frames[observer][2]


# What the restatement gives on this scene (printed by the test): 84 of the phantom's 313 voxels erased, a share of 0.268,
# and none of the room's 5384.  64 x 32 rays are 0.1 rad apart -- 0.09 m at the phantom's distance against cells of 0.05 m and an offset
# rule of half a leaf -- so one coarse frame sees through about a quarter of the phantom; the room's own voxels are all measured from
# another pose at most a few centimetres away and are protected by the margin and the end-votes.  The bounds: the phantom's share less a
# quarter of itself; for the room, where the figure is 0, one voxel in 200 (27 voxels) of slack.
PHANTOM_SHARE_MIN = 0.20
ROOM_SHARE_MAX = 0.005


def test_a_frame_carves_a_phantom_box_out_of_the_room(oracle_mod):
    ref, is_phantom, cloud, pose = phantom_scene(lambda d: oracle_mod.sphere_cloud(d, 2))
    assert 200 < is_phantom.sum() < 400 and (~is_phantom).sum() > 3000
    ob = V.observe_cloud(ref, LEAF, cloud, pose)
    erased, stats = V.carve(ref, ob)
    phantom_share = erased[is_phantom].mean()
    room_share = erased[~is_phantom].mean()
    print("phantom voxels %d erased %.3f; room voxels %d erased %.4f; %s %s" % (is_phantom.sum(), phantom_share, (~is_phantom).sum(), room_share,
                                                                                  ob["stats"], stats))
    assert phantom_share >= PHANTOM_SHARE_MIN and room_share <= ROOM_SHARE_MAX


def test_header_binding_and_adapter_agree():
    from rgbd360_amd import _lib, build, voxel_map
    L = C.CDLL(build.build())
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    for name in ("rgbd360_map_default_observe_params", "rgbd360_map_observe_sphere", "rgbd360_map_observe_rays", "rgbd360_map_votes", "rgbd360_map_carve",
                 "rgbd360_map_vote_bytes", "rgbd360_map_release_votes"):
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS, name
    assert re.search(r"\brgbd360_map_time_observe\s*\(", diag) and "rgbd360_map_time_observe" not in main and hasattr(L, "rgbd360_map_time_observe")

    def fields(text, struct):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, text).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
        return names

    for struct, cls, size in (("rgbd360_map_observe_params", _lib.MapObserveParams, 28), ("rgbd360_map_observe_stats", _lib.MapObserveStats, 80),
                              ("rgbd360_map_carve_stats", _lib.MapCarveStats, 48)):
        assert fields(main, struct) == [n for n, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    assert [n for n, _ in _lib.MapObserveStats._fields_] == list(V.STAT_NAMES)
    assert [n for n, _ in _lib.MapCarveStats._fields_] == list(V.CARVE_STAT_NAMES)
    L.rgbd360_map_default_observe_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapObserveParams)]
    L.rgbd360_map_default_observe_params.restype = None
    p = _lib.MapObserveParams()
    L.rgbd360_map_default_observe_params(None, C.byref(p))
    assert (p.min_count, p.max_steps, p.accumulate) == (1, 8192, 0) and p.near == F(0.05)
    assert (p.margin_leaves, p.margin_rel, p.max_offset) == (2.0, 0.0, 0.5)
    assert {k: v for k, v in V.DEFAULTS.items() if k != "near"} == dict(min_count=p.min_count, margin_leaves=p.margin_leaves, margin_rel=p.margin_rel,
                                                                        max_offset=p.max_offset, max_steps=p.max_steps)
    # refusals that need no device: a null map
    assert L.rgbd360_map_carve(None, 1, 0, 0, None) == -1 and L.rgbd360_map_release_votes(None) == -1
    L.rgbd360_map_vote_bytes.restype = C.c_size_t
    assert L.rgbd360_map_vote_bytes(None) == 0
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("observeParams", "observeStats", "void observe(", "votes(", "carve(", "carveStats", "rgbd360_map_observe_sphere", "rgbd360_map_observe_rays",
                 "rgbd360_map_carve"):
        assert name in hpp, name
    py = open(os.path.join(ROOT, "rgbd360_amd", "voxel_map.py")).read()
    for name in ("def observe_params", "def observe_sphere", "def observe_rays", "def votes", "def carve", "def vote_bytes", "def release_votes"):
        assert name in py, name
    assert "--carve" in open(os.path.join(ROOT, "examples", "odometry_replay.cpp")).read()
    assert "rgbd360_map_carve" in open(os.path.join(ROOT, "README.md")).read()
    # the sentences that declared carving out of scope are gone
    for doc in ("include/rgbd360_hip.h", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "Out of scope: carving" not in text and "neither is built here" not in text, doc
    assert "removal by region or age without the source data" not in open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read()
