"""Planar regions of the voxel map and relocalisation against them (rgbd360_map_planes, rgbd360_map_plane_labels, VoxelMap.relocalize;
csrc/map_planes.h) on the device against the numpy restatement (tests/map_planes_reference.py): labels, plane ordinals, statistics, root
keys and the integer sums bit for bit; the plane records byte for byte against the library's host fit of the restated regions; invariance
under insertion order, capacity and rehash; the cache across writes, parameter changes and release; the hull areas; a frame placed in
the map without a guess; and the contract (empty maps, max_out, NULL outputs, a pyramid level, refusals, a table nobody writes).

Shapes: cells of 0.25 m with exactly representable coordinates; one 5 x 5 patch in 64 slots (a single wave), two patches and a bridge in
128, a room corner of three 8 x 8 patches in 512 and 4096, a spiral strip 3 cells wide and 230 long in 1024 (several workgroups), 65
patches in 4096 (more regions than a wave has lanes); the relocalisation room (7000 voxels at leaf 0.1) in 2^14.  The conditions these
scenes rely on are proved on the restatement in tests/test_map_planes_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import map_align_reference as A
import map_planes_reference as Q
import voxel_map_reference as R
from map_input_forms import vp
from test_map_planes_cpu import EYE, LEAF, hull_area_of_all_members, library_planes, make_map, relocalize_restated, scenes

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
POSE_TOL = 5e-6       # tests/test_map_pyramid_gpu.py
CAPACITY = {"patch": (64,), "bridge": (128,), "corner": (512, 4096), "spiral": (1024,), "patches": (4096,)}


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def wants():
    """The restatement of every scene, computed once: name -> (points, leaf, parameters, the restated map, Q.planes of it)."""
    out = {}
    for name, (pts, leaf, P) in scenes().items():
        ref = make_map(pts, leaf)
        out[name] = (pts, leaf, P, ref, Q.planes(ref, leaf, **P))
    return out


@pytest.fixture(scope="module")
def room():
    pts, T = Q.room_scene(), Q.frame_pose()
    a, b = make_map(pts, 0.1), make_map(Q.in_frame(pts, T), 0.1)
    return dict(points=pts, T=T, A=a, B=b, planes_a=Q.planes(a, 0.1), planes_b=Q.planes(b, 0.1))


def new_map(reg, capacity, leaf=LEAF, points=None):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, leaf, capacity)
    m.set_box(None, None)
    if points is not None:
        m.insert_cloud(points, None, EYE)
        assert not m.full
    return m


def snapshot(m, **params):
    """Every output of the two calls as bytes: the plane records, the root keys, the statistics, the label records in key order."""
    from rgbd360_amd import _lib
    p = m.plane_seg_params(**{k: v for k, v in params.items() if k != "max_planes"})
    k = params.get("max_planes", 256)
    arr, key3, n, st = (_lib.Plane * max(k, 1))(), np.zeros((k, 3), np.int32), C.c_int(-1), _lib.MapPlaneSegStats()
    assert m._L.rgbd360_map_planes(m._handle(), C.byref(p), None, k, C.cast(arr, C.c_void_p), vp(key3), C.byref(n), C.byref(st)) == 0
    vk, lk, pi = m.plane_labels(**{k_: v for k_, v in params.items() if k_ != "max_planes"})
    order = np.argsort(A.packed_keys(vk), kind="stable")
    return dict(planes=bytes(arr)[:n.value * C.sizeof(_lib.Plane)], root_key3=key3[:n.value].tobytes(), stats=bytes(st), n=n.value,
                key3=vk[order].tobytes(), label=lk[order].tobytes(), index=pi[order].tobytes(), arr=arr, st=st)


def assert_equals_restatement(m, ref, want, params, what):
    from rgbd360_amd import _lib
    got = snapshot(m, **params)
    assert {k: getattr(got["st"], k) for k in Q.STAT_NAMES} == want["stats"], what
    assert got["n"] == len(want["planes"]) and got["root_key3"] == want["root_key3"].tobytes(), what
    live = ref.count > 0
    assert got["key3"] == ref.key[live].tobytes() and got["label"] == want["label_key3"][live].astype(np.int32).tobytes(), what
    assert got["index"] == want["plane_index"][live].tobytes(), what
    # the integer sums, N and P through the records: byte for byte the library's host fit of the restated regions (their sums, their members)
    arr, _ = library_planes(ref, want)
    assert got["planes"] == bytes(arr)[:got["n"] * C.sizeof(_lib.Plane)], what
    for o, pl in enumerate(want["planes"]):
        assert got["arr"][o].count == pl["count"] and got["arr"][o].root == o, what
    return got


@pytest.mark.parametrize("name,capacity", [(n, c) for n, cs in CAPACITY.items() for c in cs])
def test_labels_statistics_and_records_equal_the_restatement(reg, wants, name, capacity):
    pts, leaf, P, ref, want = wants[name]
    with new_map(reg, capacity, leaf, pts) as m:
        assert m.bytes == capacity * 64 and len(m) == len(ref)
        got = assert_equals_restatement(m, ref, want, P, (name, capacity))
        assert m.plane_bytes() >= 32 * capacity
        if name == "patches":
            assert got["st"].n_planes_available == 65 and got["n"] == 64 and got["st"].n_regions == 65
        if name == "spiral":
            assert got["n"] == 1 and got["st"].n_voxels_in_planes == got["st"].n_eligible > 600 and capacity // 256 >= 4
        # the plane records against the restatement's own fit of the same sums, and the hull against the hull of all members
        for o, pl in enumerate(want["planes"]):
            rec = got["arr"][o]
            c, n = np.array(list(rec.centroid), F), np.array(list(rec.normal), F)
            fit = pl["fit"]
            assert np.abs(c.astype(D) - fit["centroid"]).max() <= 4 * np.spacing(F(np.linalg.norm(fit["centroid"])))
            assert abs(D(rec.d) - fit["d"]) <= 4 * np.spacing(F(abs(fit["d"])))
            tol = 2 * np.spacing(np.maximum(np.abs(fit["normal"]), 2.0 ** -20).astype(F)).astype(D)
            assert (np.abs(n.astype(D) - fit["normal"]) <= tol).all()
            if name != "patches" or o < 3:
                a_ref = hull_area_of_all_members(ref, pl)
                assert 0.99 * a_ref <= rec.area <= a_ref * (1 + 1e-5), (name, o, rec.area, a_ref)
                hull = np.array([list(rec.hull[k]) for k in range(rec.hull_n)], D)
                members = ref.xyz[pl["members"]].astype(D)
                proj = members - ((members - c.astype(D)) @ n.astype(D))[:, None] * n.astype(D)[None, :]
                assert rec.hull_n >= 3 and all(np.abs(proj - v).max(axis=1).min() < 1e-5 for v in hull)      # each a projected member centroid


def test_insertion_order_capacity_rehash_and_repetition_leave_every_byte(reg, wants):
    pts, leaf, P, ref, want = wants["corner"]
    keys = ("planes", "root_key3", "stats", "key3", "label", "index")
    with new_map(reg, 512, leaf, pts) as m:
        first = snapshot(m, **P)
        again = snapshot(m, **P)
        assert all(first[k] == again[k] for k in keys)
        # a parameter change rebuilds, and changing it back reproduces the first bytes
        other = snapshot(m, **dict(P, min_support=7, min_voxels=3))
        w2 = Q.planes(ref, leaf, **dict(P, min_support=7, min_voxels=3))
        assert other["stats"] != first["stats"] and {k: getattr(other["st"], k) for k in Q.STAT_NAMES} == w2["stats"]
        back = snapshot(m, **P)
        assert all(first[k] == back[k] for k in keys)
        assert m.rehash(2048) == 0 and m.bytes == 2048 * 64
        assert all(first[k] == snapshot(m, **P)[k] for k in keys)
    rng = np.random.default_rng(5)
    shuffled = pts[rng.permutation(len(pts))]
    with new_map(reg, 4096, leaf) as m:
        for part in (shuffled[100:], shuffled[:100]):
            m.insert_cloud(part, None, EYE)
        assert all(first[k] == snapshot(m, **P)[k] for k in keys)


def test_the_cache_follows_removal_insertion_and_release(reg, wants):
    pts, leaf, P, ref, want = wants["bridge"]
    bridge = pts[20:21]
    assert tuple(R.voxel_index(bridge, leaf)[0]) == (4, 2, 0)
    with new_map(reg, 128, leaf, pts) as m:
        joined = assert_equals_restatement(m, ref, want, P, "joined")
        assert joined["st"].n_regions == 1
        m.remove_cloud(bridge, None, EYE)            # a tombstone: the region splits
        parted = make_map(pts, leaf)
        parted.count[np.nonzero((parted.key == (4, 2, 0)).all(axis=1))[0][0]] = 0
        got = assert_equals_restatement(m, parted, Q.planes(parted, leaf, **P), P, "parted")
        assert got["st"].n_regions == 2 and got["st"].n_voxels == 40
        m.insert_cloud(bridge, None, EYE)            # ... and joins again
        assert snapshot(m, **P)["planes"] == joined["planes"] and snapshot(m, **P)["label"] == joined["label"]
        assert m.plane_bytes() > 0
        m.release_planes()
        assert m.plane_bytes() == 0
        assert snapshot(m, **P)["planes"] == joined["planes"] and m.plane_bytes() > 0


def test_a_lost_frame_is_placed_in_the_map_without_a_guess(reg, room):
    """Map A holds the room, map B the same points seen from the frame at T.  A.relocalize(B's planes) is accepted, equals the matcher's
    result on the restated planes bit for bit, and lands inside half the capture range of coarse-to-fine ICP, which then ends where it
    ends from the true pose."""
    cloud = Q.in_frame(room["points"], room["T"])
    with new_map(reg, 1 << 14, 0.1, room["points"]) as a, new_map(reg, 1 << 14, 0.1, cloud) as b:
        R.assert_map_equals(a.extract(), room["A"])
        R.assert_map_equals(b.extract(), room["B"])
        assert_equals_restatement(a, room["A"], room["planes_a"], {}, "map A")
        assert_equals_restatement(b, room["B"], room["planes_b"], {}, "map B")
        frame_planes, _, stats_b = b.planes()
        got = a.relocalize(frame_planes)
        assert got["status"] == 0 and len(got["map_planes"]) == 9 and stats_b["n_planes_available"] == 9
        want = relocalize_restated(room)
        assert got["pose"].tobytes() == want["pose"].tobytes() and got["match"] == want["match"] and got["info"].tobytes() == want["info"].tobytes()
        T = room["T"]
        moved = np.linalg.norm(room["points"].astype(D) @ (got["pose"][:3, :3].astype(D) - T[:3, :3]).T + (got["pose"][:3, 3] - T[:3, 3]), axis=1)
        top_shift = a.c2f_params().top_shift
        print("relocalisation: largest displacement of a point", moved.max(), "m; capture range", (1 << top_shift) * 0.1, "m")
        assert moved.max() <= 0.5 * (1 << top_shift) * 0.1
        from_guess, res_g = a.align_cloud_c2f(cloud, got["pose"])
        from_truth, res_t = a.align_cloud_c2f(cloud, T.astype(F))
        dr, dt = A.pose_error(from_guess, from_truth)
        print("coarse-to-fine from the guess against from the truth:", dr, "rad", dt, "m; statuses", res_g["status"], res_t["status"])
        assert res_g["status"] == res_t["status"] == 0 and dr <= POSE_TOL and dt <= POSE_TOL


def test_the_contract_at_the_boundaries(reg, hip_lib, wants):
    from rgbd360_amd import _lib
    from rgbd360_amd.register import Rgbd360Error
    pts, leaf, P, ref, want = wants["corner"]
    sentinel = lambda: [(_lib.Plane * 8)(), np.full((8, 3), 77, np.int32), C.c_int(77), _lib.MapPlaneSegStats(n_voxels=77)]
    untouched = lambda s: bytes(s[0]) == bytes((_lib.Plane * 8)()) and (s[1] == 77).all() and s[2].value == 77 and s[3].n_voxels == 77
    call = lambda H, p, view, k, s: hip_lib.rgbd360_map_planes(H, p, view, k, C.cast(s[0], C.c_void_p), vp(s[1]), C.byref(s[2]), C.byref(s[3]))
    with new_map(reg, 512, leaf) as m:                   # an empty map: 0, zero statistics, nothing launched
        H, s = m._handle(), sentinel()
        assert call(H, None, None, 8, s) == 0 and s[2].value == 0 and bytes(s[3]) == bytes(_lib.MapPlaneSegStats()) and (s[1] == 77).all()
        assert hip_lib.rgbd360_map_plane_labels(H, None, 10, None, None, None) == 0 and m.plane_bytes() == 0
        none, keys, stats = m.planes()
        assert none == [] and keys.shape == (0, 3) and stats == dict.fromkeys(Q.STAT_NAMES, 0) and len(m.plane_labels()[0]) == 0
    with new_map(reg, 512, leaf, pts) as m:
        H, n = m._handle(), len(ref)
        before = (m.census(), m.extract())
        small = m.plane_seg_params(**P)
        # max_out smaller than the map: the count comes back, the rest of the arrays stays
        bufs = [np.full((n, 3), 77, np.int32), np.full((n, 3), 77, np.int32), np.full(n, 77, np.int32)]
        assert hip_lib.rgbd360_map_plane_labels(H, C.byref(small), 10, *map(vp, bufs)) == n
        assert all((b[10:] == 77).all() and (b[:10] != 77).all() for b in bufs)
        rows = np.searchsorted(A.packed_keys(ref.key), A.packed_keys(bufs[0][:10]))
        assert len(set(rows.tolist())) == 10 and np.array_equal(bufs[1][:10], want["label_key3"][rows]) and np.array_equal(bufs[2][:10], want["plane_index"][rows])
        assert hip_lib.rgbd360_map_plane_labels(H, C.byref(small), 0, *map(vp, bufs)) == n
        # NULL in every output position, and all of them
        for skip in range(3):
            bufs = [np.full((n, 3), 77, np.int32), np.full((n, 3), 77, np.int32), np.full(n, 77, np.int32)]
            assert hip_lib.rgbd360_map_plane_labels(H, C.byref(small), n, *[None if k == skip else vp(b) for k, b in enumerate(bufs)]) == n
            assert (bufs[skip] == 77).all() and all((b != 77).any() for k, b in enumerate(bufs) if k != skip)
        assert hip_lib.rgbd360_map_plane_labels(H, C.byref(small), n, None, None, None) == n
        assert hip_lib.rgbd360_map_planes(H, C.byref(small), None, 8, None, None, None, None) == 0
        s = sentinel()
        assert hip_lib.rgbd360_map_planes(H, C.byref(small), None, 8, C.cast(s[0], C.c_void_p), None, None, None) == 0 and s[0][2].count == 35
        s = sentinel()
        assert call(H, C.byref(small), None, 2, s) == 0 and s[2].value == 2 and s[3].n_planes_available == 3 and (s[1][2:] == 77).all()
        assert bytes(s[0][2]) == bytes(_lib.Plane())
        # the viewpoint: the normals face it
        view = np.array([5.0, 5.0, 5.0], F)
        s = sentinel()
        assert call(H, C.byref(small), vp(view), 8, s) == 0
        for o in range(3):
            nrm, c = np.array(list(s[0][o].normal)), np.array(list(s[0][o].centroid))
            assert nrm @ (view - c) > 0 and abs(s[0][o].d + nrm @ c) < 1e-6
        # every refusal: -1, an error text, no output byte touched
        nan = float("nan")
        bad = [dict(min_count=0), dict(min_support=0), dict(min_support=28), dict(max_flatness=-1.0), dict(max_flatness=nan),
               dict(max_voxel_curvature=-1.0), dict(max_voxel_curvature=nan), dict(cos_angle=-0.1), dict(cos_angle=1.5), dict(cos_angle=nan),
               dict(max_offset=-1.0), dict(max_offset=nan), dict(min_voxels=0), dict(max_curvature=-1.0), dict(max_curvature=nan)]
        for b in bad:
            p, s = m.plane_seg_params(**b), sentinel()
            assert call(H, C.byref(p), None, 8, s) == -1 and untouched(s) and hip_lib.rgbd360_map_last_error(H), b
            bufs = [np.full((n, 3), 77, np.int32), np.full((n, 3), 77, np.int32), np.full(n, 77, np.int32)]
            assert hip_lib.rgbd360_map_plane_labels(H, C.byref(p), n, *map(vp, bufs)) == -1 and all((x == 77).all() for x in bufs), b
        s = sentinel()
        assert call(H, None, None, -1, s) == -1 and untouched(s) and b"max_planes" in hip_lib.rgbd360_map_last_error(H)
        for v in ((nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
            s = sentinel()
            assert call(H, None, vp(np.array(v, F)), 8, s) == -1 and untouched(s) and b"viewpoint" in hip_lib.rgbd360_map_last_error(H)
        assert hip_lib.rgbd360_map_plane_labels(H, None, -1, None, None, None) == -1 and b"max_out" in hip_lib.rgbd360_map_last_error(H)
        with pytest.raises(Rgbd360Error, match=r"\(-1\): .*min_voxels"):
            m.planes(min_voxels=0)
        # a level of the pyramid as the map: the restatement of the merged map at twice the leaf
        lv = m.level(1)
        coarse = make_map(pts, 2 * leaf)
        R.assert_map_equals(lv.extract(), coarse)
        assert_equals_restatement(lv, coarse, Q.planes(coarse, 2 * leaf, min_voxels=3), dict(min_voxels=3), "level 1")
        # nothing has written the table
        after = (m.census(), m.extract())
        assert before[0] == after[0] and all(x.tobytes() == y.tobytes() for x, y in zip(before[1], after[1]))
        R.assert_map_equals(after[1], ref)


def test_odometry_replay_writes_the_planes_of_the_map(reg, tmp_path):
    """examples/odometry_replay.cpp --map F --map-planes OUT on the three-frame replay of the map tests: one well-formed line per plane
    (root key, N, P, centroid, normal, d, area, curvature), N over the lines = n_voxels_in_planes, the pose lines unchanged."""
    import os
    import subprocess
    import sys
    from tests.test_cpp_adapter import ROOT, build_example
    exe = build_example(tmp_path)
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "3", "256", "128"])
    out = tmp_path / "planes.txt"
    base = [exe, str(seq), "3", "256", "128", "--map", str(tmp_path / "map.txt")]
    plain = subprocess.run(base, text=True, capture_output=True, check=True)
    run = subprocess.run(base + ["--map-planes", str(out)], text=True, capture_output=True, check=True)
    words = [l for l in run.stdout.splitlines() if l.startswith("planes ")][0].split()
    st = dict(zip(words[1::2], map(int, words[2::2])))
    assert [l for l in run.stdout.splitlines() if not l.startswith("planes ")] == plain.stdout.splitlines()
    rec = np.loadtxt(out, ndmin=2)
    assert rec.shape == (st["planes"], 14) and st["planes"] == st["available"] >= 1 and st["voxels"] == len((tmp_path / "map.txt").read_text().splitlines())
    assert rec[:, 3].sum() == st["in_planes"] and (rec[:, 3] >= 50).all() and (rec[:, 4] >= rec[:, 3]).all()
    assert np.abs(np.linalg.norm(rec[:, 8:11], axis=1) - 1).max() < 1e-5 and np.abs((rec[:, 8:11] * rec[:, 5:8]).sum(axis=1) + rec[:, 11]).max() < 1e-4
    assert (rec[:, 12] > 0).all() and (rec[:, 13] >= 0).all() and (rec[:, 13] <= 0.0013 * (1 + 1e-6)).all()
    keys = A.packed_keys(rec[:, 0:3].astype(np.int64))
    assert (np.diff(keys) > 0).all()
    needs = subprocess.run([exe, str(seq), "3", "256", "128", "--map-planes", str(out)], text=True, capture_output=True)
    assert needs.returncode == 2 and "need --map" in needs.stderr
