"""Surface normals of the voxel map and the surface cast (rgbd360_map_normals*, rgbd360_map_raycast_surface*, csrc/map_normals.h) on the
device against the numpy restatement (tests/map_normals_reference.py), bit for bit: the read-out with its statistics, its independence
of insertion order, capacity and rehash, the layer's cache across writes and parameter changes, the surface cast of ray lists next to
the plain cast, the panorama through its three entries, and the contract (empty maps, max_out, refusals, NULL outputs, a table nobody
writes).

Shapes: leaf 0.05; a room corner of 1 m sides plus one 256 x 128 frame of the synthetic room (about 9000 voxels, tables of 2^14 .. 2^16
slots); lists of 1, 63, 65 and 257 rays (partly filled waves and workgroups); 32 x 64 panoramas of the sphere scene whose conditions
tests/test_map_normals_cpu.py proves on the restatement."""
import ctypes as C

import numpy as np
import pytest

import map_align_plane_reference as P
import map_normals_reference as N
import map_raycast_reference as M
import voxel_map_reference as R
from map_input_forms import cm, hip_runtime, vp
from test_map_normals_cpu import OFF_CENTRE, pose_at
from test_map_raycast_cpu import SPHERE_POINTS, sphere_cloud
from test_map_raycast_gpu import SMALL_BOX, ray_list

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)
F = np.float32
LEAF = 0.05
OTHER = dict(min_count=2, min_support=7, max_flatness=0.01)
OUT_NAMES = ("xyz", "normal", "curvature", "status", "count", "key3")


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip():
    return hip_runtime()


def new_map(reg, capacity=1 << 14, box=SMALL_BOX):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, LEAF, capacity)
    m.set_box(*box) if box is not None else m.set_box(None, None)
    return m


@pytest.fixture(scope="module")
def scene(reg):
    """The room corner at the general pose (a cloud) and frame 0 of the synthetic room (a sphere image with colours, around the origin:
    negative coordinates), with the restatement's map of both under SMALL_BOX; computed once, never changed."""
    from rgbd360_amd import synth
    corner = P.corner_scene(1, size=1.0)
    rgb, depth = synth.render(synth.trajectory_pose(0), 256, 128)
    pose = synth.trajectory_pose(0).astype(F)
    cloud = reg.sphere_cloud(depth, 2)
    ref = R.Map([(corner, None, R.general_pose()), (cloud, rgb.reshape(-1, 3), pose)], LEAF, SMALL_BOX)
    assert 3000 < len(ref) < 0.7 * (1 << 14) and ref.key.min() < -10 and ref.count.max() > 2
    return dict(corner=corner, rgb=rgb, depth=depth, pose=pose, ref=ref, wants={})


def fill(m, scene, reverse=False):
    steps = [lambda: m.insert_cloud(scene["corner"], None, R.general_pose()),
             lambda: m.insert_sphere(scene["rgb"], scene["depth"], scene["pose"], convention=2)]
    for step in (steps[::-1] if reverse else steps):
        step()
        assert not m.full


def sorted_records(got):
    """The six planes of a read-out in ascending key order, and the statistics."""
    order = np.argsort(M.packed_keys(got[5]), kind="stable")
    return [np.ascontiguousarray(a[order]) for a in got[:6]], got[6]


def assert_normals_equal(got, want, what=""):
    planes, stats = sorted_records(got)
    assert stats == want["stats"], (what, stats, want["stats"])
    for name, a in zip(OUT_NAMES, planes):
        assert a.tobytes() == want[name].astype(a.dtype).tobytes(), (what, name)


def want_normals(scene, viewpoint=None, **params):
    key = (None if viewpoint is None else tuple(viewpoint), tuple(sorted(params.items())))
    if key not in scene["wants"]:
        scene["wants"][key] = N.normals(scene["ref"], viewpoint=viewpoint, **params)
    return scene["wants"][key]


def test_read_out_equals_the_restatement(reg, scene):
    with new_map(reg) as m:
        fill(m, scene)
        extract = m.extract()
        for params in ({}, OTHER):
            want = want_normals(scene, **params)
            got = m.normals(**params)
            print(params, got[6])
            assert_normals_equal(got, want, str(params))
            planes, _ = sorted_records(got)
            assert planes[0].tobytes() == extract[0].tobytes() and planes[4].tobytes() == extract[2].tobytes() and np.array_equal(planes[5], extract[3])
        # not vacuous: every status occurs, at the defaults and at the stricter parameters
        st = want_normals(scene)["stats"]
        assert st["n_normals"] > 1000 and st["n_unsupported"] > 10 and st["n_nonplanar"] > 10 and st["n_below_min_count"] == 0
        so = want_normals(scene, **OTHER)["stats"]
        assert so["n_below_min_count"] > 100 and so["n_normals"] > 100 and so != st
        # a viewpoint turns the normals towards it
        view = (0.3, -0.2, 0.1)
        want = want_normals(scene, viewpoint=view)
        assert_normals_equal(m.normals(viewpoint=view), want, "viewpoint")
        assert (want["normal"] != want_normals(scene)["normal"]).any(axis=1).sum() > 100


def test_insertion_order_capacity_and_rehash_change_no_bit(reg, scene):
    want = want_normals(scene)
    with new_map(reg, 1 << 14) as a, new_map(reg, 1 << 16) as b:
        fill(a, scene)
        fill(b, scene, reverse=True)
        first, _ = sorted_records(a.normals())
        second, stats = sorted_records(b.normals())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, second)) and stats == want["stats"]
        assert b.rehash(1 << 14) == 0
        third, stats = sorted_records(b.normals())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, third)) and stats == want["stats"]
        assert_normals_equal(a.normals(), want)


def test_the_layer_follows_the_map_and_the_parameters(reg, scene):
    extra = P.corner_scene(2, size=0.6)
    pose = R.general_pose()
    pose[:3, 3] += (0.1, 0.15, -0.1)          # a second corner through the first
    base = R.Map([(scene["corner"], None, R.general_pose())], LEAF, SMALL_BOX)
    both = R.Map([(scene["corner"], None, R.general_pose()), (extra, None, pose)], LEAF, SMALL_BOX)
    with new_map(reg) as m:
        m.insert_cloud(scene["corner"], None, R.general_pose())
        first = m.normals()
        assert_normals_equal(first, N.normals(base), "first")
        again = m.normals()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(sorted_records(first)[0], sorted_records(again)[0])) and first[6] == again[6]
        m.insert_cloud(extra, None, pose)
        second = m.normals()
        want = N.normals(both)
        assert_normals_equal(second, want, "after the insert")
        # (the new frame changes normals of voxels that were there before)
        old = np.isin(M.packed_keys(want["key3"]), M.packed_keys(base.key))
        assert (want["normal"][old] != N.normals(base)["normal"]).any() or (want["status"][old] != N.normals(base)["status"]).any()
        m.remove_cloud(extra, None, pose)
        assert not m.mismatch and m.census()["n_tombstones"] > 0
        third = m.normals()
        assert_normals_equal(third, N.normals(base), "after the removal")
        assert all(x.tobytes() == y.tobytes() for x, y in zip(sorted_records(first)[0], sorted_records(third)[0])) and first[6] == third[6]
        # a parameter change without a write rebuilds the layer, and changing back does again
        loose = m.normals(min_support=3)
        assert_normals_equal(loose, N.normals(base, min_support=3), "min_support 3")
        assert loose[6] != first[6]
        flat = m.normals(max_flatness=0.001)
        assert_normals_equal(flat, N.normals(base, max_flatness=0.001), "max_flatness 0.001")
        assert flat[6]["n_nonplanar"] > first[6]["n_nonplanar"]
        assert_normals_equal(m.normals(), N.normals(base), "the defaults again")
        # the surface cast shares the layer: after the read-out at other parameters it still sees its own
        o, d = ray_list(65)
        got = m.raycast_surface(o, d)
        want = N.cast_surface(base, LEAF, o, d)
        assert got[0].tobytes() == want["t"].tobytes() and got[1].tobytes() == want["normal"].tobytes() and got[6] == want["n_on_plane"]


@pytest.fixture(scope="module")
def cast_map(reg, scene):
    m = new_map(reg)
    fill(m, scene)
    yield m
    m.close()


def assert_surface_equals(got, plain, want, what=""):
    """got: raycast_surface's tuple; plain: raycast's on the same rays; want: the restatement."""
    t, normal, key3, count, rgb, status, on_plane, stats = got
    for a, b in zip((key3, count, rgb, status), plain[1:5]):
        assert a.tobytes() == b.tobytes(), what
    assert stats == plain[5], what
    assert np.array_equal(status, want["status"]) and np.array_equal(key3, want["key3"]), what
    assert t.tobytes() == want["t"].tobytes(), (what, np.nonzero(t != want["t"])[0][:10])
    assert normal.tobytes() == want["normal"].tobytes(), (what, np.nonzero((normal != want["normal"]).any(axis=1))[0][:10])
    assert on_plane == want["n_on_plane"], what


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_surface_cast_of_ray_lists(hip_lib, hip, scene, cast_map, n):
    from rgbd360_amd import _lib
    m, ref = cast_map, scene["ref"]
    o, d = ray_list(n)
    for params in ({}, dict(t_min=0.0, max_steps=40), dict(max_shift=0.0), dict(min_support=7, max_flatness=0.01, normal_min_count=2)):
        ray = {k: v for k, v in params.items() if k in ("t_min", "max_steps")}
        plain = m.raycast(o, d, **ray)
        want = N.cast_surface(ref, LEAF, o, d, **params)
        got = m.raycast_surface(o, d, **params)
        print(n, params, got[6], got[7])
        assert_surface_equals(got, plain, want, "%d %s" % (n, params))
        if params.get("max_shift") == 0.0:
            assert got[0].tobytes() == plain[0].tobytes() and got[6] == 0
            if n == 257:
                assert got[1].any()
    if n == 257:
        want = N.cast_surface(ref, LEAF, o, d)
        hit = want["status"] == M.HIT
        # every path: misses, hits with and without a normal, plane depths taken and refused, depths that differ from the plain cast's
        assert {M.HIT, M.LEFT_BOX, M.BAD} <= set(want["status"].tolist())
        assert 0 < want["n_on_plane"] < hit.sum() and (want["normal"][hit] == 0).all(axis=1).any()
        assert (want["t"][want["on_plane"]] != M.cast(ref, LEAF, o, d)["t"][want["on_plane"]]).any()
    # on device arrays: the same bytes
    sizes = [12 * n, 12 * n, 4 * n, 12 * n, 12 * n, 4 * n, 3 * n, 4 * n]
    dev = [C.c_void_p() for _ in sizes]
    for p, s in zip(dev, sizes):
        assert hip.hipMalloc(C.byref(p), s) == 0
    assert hip.hipMemcpy(dev[0], vp(o), sizes[0], 1) == 0 and hip.hipMemcpy(dev[1], vp(d), sizes[1], 1) == 0
    st, on_plane = _lib.MapRaycastStats(), C.c_longlong(-1)
    assert hip_lib.rgbd360_map_raycast_surface(m._handle(), n, dev[0], dev[1], 1, None, None, *dev[2:], C.byref(on_plane), C.byref(st)) == 0
    out = [np.zeros(n, F), np.zeros((n, 3), F), np.zeros((n, 3), np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.uint8), np.zeros(n, np.int32)]
    for a, p, s in zip(out, dev[2:], sizes[2:]):
        assert hip.hipMemcpy(vp(a), p, s, 2) == 0
    for p in dev:
        hip.hipFree(p)
    host = m.raycast_surface(o, d)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(host[:6], out)) and on_plane.value == host[6]
    assert {k: getattr(st, k) for k in M.STAT_NAMES} == host[7]


def test_surface_panorama_through_its_three_entries(hip_lib, hip, reg):
    rows, cols = 32, 64
    n = rows * cols
    cloud = sphere_cloud(1.5, SPHERE_POINTS)
    ref = R.Map([(cloud, None, EYE)], LEAF, None)
    with new_map(reg, 1 << 15, box=None) as m:
        st = m.insert_cloud(cloud, None, EYE)
        assert not m.full and st["n_added"] == len(cloud)
        for t in ((0.0, 0.0, 0.0), OFF_CENTRE):
            pose = pose_at(t)
            want = N.cast_surface_sphere(ref, LEAF, rows, cols, pose)
            plain = m.raycast_sphere(rows, cols, pose)
            depth, normal, rgb, count, key3, on_plane, stats = m.raycast_surface_sphere(rows, cols, pose)
            print(t, on_plane, stats)
            assert all(a.tobytes() == b.tobytes() for a, b in zip((rgb, count, key3), plain[1:4])) and stats == plain[4]
            assert depth.tobytes() == want["depth"].tobytes() and normal.tobytes() == want["normal"].tobytes()
            assert np.array_equal(key3, want["key3"]) and on_plane == want["n_on_plane"] == n and stats["n_hits"] == n
            assert (depth != plain[0]).sum() > n // 2
            # the list entry on the panorama's rays
            o, d = M.sphere_rays(rows, cols, pose)
            lt, ln, lkey, lcount, lrgb, lstatus, lon, lstats = m.raycast_surface(o, d)
            assert lt.tobytes() == depth.tobytes() and ln.tobytes() == normal.tobytes() and lkey.tobytes() == key3.tobytes()
            assert lcount.tobytes() == count.tobytes() and lrgb.tobytes() == rgb.tobytes() and lon == on_plane and lstats == stats
            # the device entry
            sizes = [4 * n, 12 * n, 3 * n, 4 * n, 12 * n, 8, 72]
            dev = [C.c_void_p() for _ in sizes]
            for p, s in zip(dev, sizes):
                assert hip.hipMalloc(C.byref(p), s) == 0
            assert hip_lib.rgbd360_map_raycast_surface_sphere_dev(m._handle(), rows, cols, vp(cm(pose)), None, None, *dev) == 0
            assert hip_lib.rgbd360_sync(m._reg._ctx()) == 0
            out = [np.zeros((rows, cols), F), np.zeros((rows, cols, 3), F), np.zeros((rows, cols, 3), np.uint8), np.zeros((rows, cols), np.int32),
                   np.zeros((rows, cols, 3), np.int32), np.zeros(1, np.int64), np.zeros(9, np.int64)]
            for a, p, s in zip(out, dev, sizes):
                assert hip.hipMemcpy(vp(a), p, s, 2) == 0
                hip.hipFree(p)
            assert all(x.tobytes() == y.tobytes() for x, y in zip((depth, normal, rgb, count, key3), out[:5]))
            assert out[5][0] == on_plane and out[6].tolist() == [stats[k] for k in M.STAT_NAMES]
            # the model image goes into the dense alignment as it is
            reg.setTargetFrame(rgb, depth)


def test_contract(hip_lib, reg, scene):
    from rgbd360_amd import _lib
    from rgbd360_amd.register import Rgbd360Error
    zero = dict.fromkeys(N.STAT_NAMES, 0)
    o, d = ray_list(65)
    with new_map(reg, 1 << 12) as m:          # an empty map
        got = m.normals()
        assert all(len(a) == 0 for a in got[:6]) and got[6] == zero
        st = _lib.MapNormalStats(n_voxels=7, n_normals=7)
        buf = np.full(8, 7, np.int32)
        assert hip_lib.rgbd360_map_normals(m._handle(), None, None, 2, vp(buf), None, None, None, None, None, C.byref(st)) == 0
        assert {k: getattr(st, k) for k in N.STAT_NAMES} == zero and (buf == 7).all()
        t, normal, key3, count, rgb, status, on_plane, stats = m.raycast_surface(o, d)
        assert not t.any() and not normal.any() and not key3.any() and not count.any() and not status.any() and on_plane == 0
        assert stats == dict.fromkeys(M.STAT_NAMES, 0)
        depth, normal, _, count, _, on_plane, stats = m.raycast_surface_sphere(32, 64, EYE)
        assert not depth.any() and not normal.any() and not count.any() and on_plane == 0 and stats == dict.fromkeys(M.STAT_NAMES, 0)
    with new_map(reg) as m:
        fill(m, scene)
        n = len(m)
        before = (m.census(), m.extract())
        H = m._handle()
        # max_out below the map's size: the full count comes back, nothing is written past max_out
        shapes = [((n, 3), F), ((n, 3), F), ((n,), F), ((n,), np.int32), ((n,), np.int32), ((n, 3), np.int32)]
        sentinel = lambda: [np.full(s, 77, t) for s, t in shapes]
        bufs = sentinel()
        st = _lib.MapNormalStats()
        assert hip_lib.rgbd360_map_normals(H, None, None, 100, *map(vp, bufs), C.byref(st)) == n
        assert all((a[100:] == 77).all() for a in bufs) and {k: getattr(st, k) for k in N.STAT_NAMES} == want_normals(scene)["stats"]
        want = want_normals(scene)
        rows = np.searchsorted(M.packed_keys(want["key3"]), M.packed_keys(bufs[5][:100]))
        assert len(set(rows.tolist())) == 100
        for name, a in zip(OUT_NAMES, bufs):
            assert a[:100].tobytes() == want[name][rows].astype(a.dtype).tobytes(), name
        assert hip_lib.rgbd360_map_normals(H, None, None, 0, *map(vp, bufs), C.byref(st)) == n and st.n_voxels == n
        # every refusal: -1, nothing written
        nan = float("nan")
        bad_params = [dict(min_count=0), dict(min_support=0), dict(min_support=28), dict(max_flatness=-0.1), dict(max_flatness=nan), dict(max_shift=-1.0),
                      dict(max_shift=nan)]
        views = [np.array(v, F) for v in ((nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf))]
        ray_bufs = lambda: [np.full((65,), 77, F), np.full((65, 3), 77, F), np.full((65, 3), 77, np.int32), np.full((65,), 77, np.int32),
                            np.full((65, 3), 77, np.uint8), np.full((65,), 77, np.int32)]
        pano_bufs = lambda: [np.full((32, 64), 77, F), np.full((32, 64, 3), 77, F), np.full((32, 64, 3), 77, np.uint8), np.full((32, 64), 77, np.int32),
                             np.full((32, 64, 3), 77, np.int32)]
        for bad in bad_params:
            p = m.normal_params(**bad)
            bufs, st = sentinel(), _lib.MapNormalStats(n_voxels=77)
            assert hip_lib.rgbd360_map_normals(H, C.byref(p), None, n, *map(vp, bufs), C.byref(st)) == -1, bad
            assert all((a == 77).all() for a in bufs) and st.n_voxels == 77 and hip_lib.rgbd360_map_last_error(H)
            rb, rs, on = ray_bufs(), _lib.MapRaycastStats(n_rays=77), C.c_longlong(77)
            assert hip_lib.rgbd360_map_raycast_surface(H, 65, vp(o), vp(d), 0, None, C.byref(p), *map(vp, rb), C.byref(on), C.byref(rs)) == -1, bad
            assert all((a == 77).all() for a in rb) and rs.n_rays == 77 and on.value == 77
            pb = pano_bufs()
            assert hip_lib.rgbd360_map_raycast_surface_sphere(H, 32, 64, vp(cm(EYE)), None, C.byref(p), *map(vp, pb), C.byref(on), C.byref(rs)) == -1, bad
            assert all((a == 77).all() for a in pb) and rs.n_rays == 77 and on.value == 77
            assert hip_lib.rgbd360_map_raycast_surface_sphere_dev(H, 32, 64, vp(cm(EYE)), None, C.byref(p), None, None, None, None, None, None, None) == -1
            assert hip_lib.rgbd360_map_normals_dev(H, C.byref(p), None, n, None, None, None, None, None, None, None) == -1
        for view in views:
            bufs = sentinel()
            assert hip_lib.rgbd360_map_normals(H, None, vp(view), n, *map(vp, bufs), None) == -1
            assert all((a == 77).all() for a in bufs) and b"viewpoint" in hip_lib.rgbd360_map_last_error(H)
        assert hip_lib.rgbd360_map_normals(H, None, None, -1, *map(vp, sentinel()), None) == -1
        # the plain cast's refusals are the surface cast's
        with pytest.raises(Rgbd360Error, match=r"\(-1\): .*max_steps"):
            m.raycast_surface(o, d, max_steps=0)
        with pytest.raises(Rgbd360Error, match=r"\(-1\): .*(image|size)"):
            m.raycast_surface_sphere(1, 64, EYE)
        assert hip_lib.rgbd360_map_raycast_surface(H, 5, None, None, 0, None, None, None, None, None, None, None, None, None, None) == -1
        # NULL in every output position, and all of them NULL
        for skip in list(range(7)) + [None]:
            bufs, st = sentinel(), _lib.MapNormalStats()
            args = [vp(a) if k != skip and skip is not None else None for k, a in enumerate(bufs)]
            stats = None if skip in (6, None) else C.byref(st)
            assert hip_lib.rgbd360_map_normals(H, None, None, n, *args, stats) == n, skip
            planes = [a for k, a in enumerate(bufs) if k != skip and skip is not None]
            names = [nm for k, nm in enumerate(OUT_NAMES) if k != skip and skip is not None]
            if "key3" in names:
                order = np.argsort(M.packed_keys(bufs[5]), kind="stable")
                for nm, a in zip(names, planes):
                    assert a[order].tobytes() == want[nm].astype(a.dtype).tobytes(), (skip, nm)
        ref_cast = N.cast_surface(scene["ref"], LEAF, o, d)
        for skip in list(range(8)) + [None]:
            rb, rs, on = ray_bufs(), _lib.MapRaycastStats(), C.c_longlong(-1)
            args = [vp(a) if k != skip and skip is not None else None for k, a in enumerate(rb)]
            tail = [None if skip in (6, None) else C.byref(on), None if skip in (7, None) else C.byref(rs)]
            assert hip_lib.rgbd360_map_raycast_surface(H, 65, vp(o), vp(d), 0, None, None, *args, *tail) == 0, skip
            for k, name in enumerate(("t", "normal", "key3", "count", "rgb", "status")):
                if skip is not None and k != skip:
                    assert rb[k].tobytes() == ref_cast[name].astype(rb[k].dtype).tobytes(), (skip, name)
                else:
                    assert (rb[k] == 77).all()
            assert skip in (6, None) or on.value == ref_cast["n_on_plane"]
        normal = np.zeros((32, 64, 3), F)
        assert hip_lib.rgbd360_map_raycast_surface_sphere(H, 32, 64, vp(cm(scene["pose"])), None, None, None, vp(normal), None, None, None, None, None) == 0
        assert normal.tobytes() == N.cast_surface_sphere(scene["ref"], LEAF, 32, 64, scene["pose"])["normal"].tobytes() and normal.any()
        # nothing has written the table
        after = (m.census(), m.extract())
        assert before[0] == after[0] and all(a.tobytes() == b.tobytes() for a, b in zip(before[1], after[1]))
        R.assert_map_equals(after[1], scene["ref"])


def test_odometry_replay_writes_the_oriented_cloud_and_the_surface_panorama(reg, tmp_path):
    """examples/odometry_replay.cpp --map F --map-normals OUT --raycast-surface P: one line per voxel of F in OUT, the normals of unit
    length where the status is OK and facing the last pose, and P_depth.pfm / P_normal.pfm of a 256 x 128 frame behind their headers."""
    import os
    import subprocess
    import sys
    from tests.test_cpp_adapter import ROOT, build_example
    exe = build_example(tmp_path)
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "3", "256", "128"])
    out, prefix = tmp_path / "normals.txt", tmp_path / "surf"
    run = subprocess.run([exe, str(seq), "3", "256", "128", "--map", str(tmp_path / "map.txt"), "--map-normals", str(out), "--raycast-surface", str(prefix)],
                         text=True, capture_output=True, check=True)
    words = [l for l in run.stdout.splitlines() if l.startswith("normals ")][0].split()
    st = dict(zip(words[1::2], map(int, words[2::2])))
    rec = np.loadtxt(out)
    n_map = len((tmp_path / "map.txt").read_text().splitlines())
    assert len(rec) == st["voxels"] == n_map and st["normals"] > 1000
    ok = rec[:, 7] == N.OK
    assert ok.sum() == st["normals"] and np.abs(np.linalg.norm(rec[ok, 3:6], axis=1) - 1).max() < 1e-5 and not rec[~ok, 3:6].any()
    pose_t = [float(v) for v in [l for l in run.stdout.splitlines() if l.startswith("pair ")][-1].split()[-3:]]
    assert ((rec[ok, 3:6] * (np.array(pose_t) - rec[ok, 0:3])).sum(axis=1) > -1e-4).all()
    words = [l for l in run.stdout.splitlines() if l.startswith("raycast-surface ")][0].split()
    rs = dict(zip(words[1::2], map(int, words[2::2])))
    assert rs["rays"] == 256 * 128 and 0 < rs["on_plane"] <= rs["hits"] <= rs["rays"]
    pfm, nfm = (tmp_path / "surf_depth.pfm").read_bytes(), (tmp_path / "surf_normal.pfm").read_bytes()
    assert pfm.startswith(b"Pf\n256 128\n-1.0\n") and len(pfm) == len(b"Pf\n256 128\n-1.0\n") + 256 * 128 * 4
    assert nfm.startswith(b"PF\n256 128\n-1.0\n") and len(nfm) == len(b"PF\n256 128\n-1.0\n") + 256 * 128 * 12
    depth = np.frombuffer(pfm[len(b"Pf\n256 128\n-1.0\n"):], F)
    normal = np.frombuffer(nfm[len(b"PF\n256 128\n-1.0\n"):], F).reshape(-1, 3)
    assert int((depth > 0).sum()) == rs["hits"] and rs["on_plane"] <= int(normal.any(axis=1).sum()) <= rs["hits"]
    needs = subprocess.run([exe, str(seq), "3", "256", "128", "--map-normals", str(out)], text=True, capture_output=True)
    assert needs.returncode == 2 and "need --map" in needs.stderr
