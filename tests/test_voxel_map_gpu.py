"""The resident voxel-grid global map (rgbd360_map_*, csrc/voxel_map.h) on the device against the numpy restatement of its definition
(tests/voxel_map_reference.py), bit for bit: keys, counts, centroids, colours, order and the call statistics.  The shapes are the
smallest at which each mechanism can fail: several workgroups, ragged tiles, a workgroup whose points all share a voxel, one whose
points share none (the block table overflows into the direct path), probing near a full table, a table that is full."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import voxel_map_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def frame(reg, small_pair):
    """The synthetic pair's first frame (256 x 128, depth in the generator's type) with its convention-2 cloud from the device."""
    rgb, depth = small_pair[0]
    return dict(rgb=rgb, depth=depth, cloud=reg.sphere_cloud(depth, 2), colours=rgb.reshape(-1, 3))


@pytest.fixture(scope="module")
def frame_b(reg, small_pair):
    rgb, depth = small_pair[1]
    return dict(rgb=rgb, depth=depth, cloud=reg.sphere_cloud(depth, 2), colours=rgb.reshape(-1, 3))


def new_map(reg, leaf=0.05, capacity=1 << 16, box="default"):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, leaf, capacity)
    if box is None:
        m.set_box(None, None)
    elif box != "default":
        m.set_box(*box)
    return m


def check_stats(got, want):
    assert {k: got[k] for k in R.STAT_NAMES} == {k: want[k] for k in R.STAT_NAMES}


@pytest.mark.parametrize("pose", [EYE, R.general_pose()], ids=["identity", "general"])
def test_sphere_frame_equals_the_restatement_and_the_cloud_route(reg, frame, pose):
    ref = R.Map([(frame["cloud"], frame["colours"], pose)], 0.05)
    assert len(ref) > 1000 and ref.count.max() > 4 and ref.stats[0]["n_box_rejected"] > 0
    with new_map(reg) as m:
        st = m.insert_sphere(frame["rgb"], frame["depth"], pose, convention=2)
        assert not m.full
        check_stats(st, ref.stats[0])
        got = m.extract()
        R.assert_map_equals(got, ref)
    with new_map(reg) as m2:
        st2 = m2.insert_cloud(frame["cloud"], frame["colours"], pose)
        check_stats(st2, ref.stats[0])
        got2 = m2.extract()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, got2))


def test_a_strip_of_two_tiles_per_row(reg):
    """1100 x 24: a full tile and a ragged second one of 76 columns per row, the smallest shape in which all four point slots of a thread
    and the second blockIdx.x of the sphere route hold pixels (at 256 columns only the first slot ever does)."""
    from rgbd360_amd import synth
    rgb, depth = synth.render(synth.trajectory_pose(0, 7), 1100, 24, 7)
    cloud, colours, pose = reg.sphere_cloud(depth, 2), rgb.reshape(-1, 3), R.general_pose()
    ref = R.Map([(cloud, colours, pose)], 0.1)
    assert len(ref) > 200 and ref.count.max() > 4
    with new_map(reg, 0.1) as m:
        st = m.insert_sphere(rgb, depth, pose, convention=2)
        check_stats(st, ref.stats[0])
        got = m.extract()
        R.assert_map_equals(got, ref)
    with new_map(reg, 0.1) as m2:
        check_stats(m2.insert_cloud(cloud, colours, pose), ref.stats[0])
        got2 = m2.extract()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, got2))


def test_every_point_shares_a_few_voxels(reg, frame):
    """leaf 4 m: every workgroup hits the same few voxels -- on-chip combining and contention on a handful of slots."""
    pose = R.general_pose()
    ref = R.Map([(frame["cloud"], frame["colours"], pose)], 4.0, None)
    assert len(ref) <= 27 and ref.count.max() > 5000
    with new_map(reg, leaf=4.0, capacity=64, box=None) as m:
        check_stats(m.insert_sphere(frame["rgb"], frame["depth"], pose, convention=2), ref.stats[0])
        R.assert_map_equals(m.extract(), ref)


def test_almost_no_sharing(reg, frame):
    """64 x 32 pixels in cells of 4 mm: nearly every point claims a fresh slot and the workgroups' tables overflow."""
    depth = np.ascontiguousarray(frame["depth"][::4, ::4])
    rgb = np.ascontiguousarray(frame["rgb"][::4, ::4])
    cloud = reg.sphere_cloud(depth, 2)
    ref = R.Map([(cloud, rgb.reshape(-1, 3), EYE)], 0.004, None)
    assert depth.shape == (32, 64) and len(ref) > 0.9 * ref.n_passing > 1500
    with new_map(reg, leaf=0.004, capacity=4096, box=None) as m:
        check_stats(m.insert_sphere(rgb, depth, EYE, convention=2), ref.stats[0])
        R.assert_map_equals(m.extract(), ref)


def scattered_cloud(n_cells, n_points, seed, leaf=0.05):
    """n_points points in exactly n_cells distinct cells of a 16^3 block around the origin."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(16 ** 3, n_cells, replace=False)
    ijk = np.stack([cells % 16, cells // 16 % 16, cells // 256], axis=1) - 8
    which = np.concatenate([np.arange(n_cells), rng.integers(0, n_cells, n_points - n_cells)])
    xyz = ((ijk[which] + rng.uniform(0.2, 0.8, (n_points, 3))) * leaf).astype(np.float32)
    rgb = rng.integers(0, 256, (n_points, 3)).astype(np.uint8)
    return xyz, rgb


def test_probing_near_a_full_table(reg):
    xyz, rgb = scattered_cloud(900, 3000, seed=5)
    ref = R.Map([(xyz, rgb, EYE)], 0.05, None)
    assert len(ref) == 900
    with new_map(reg, capacity=1024, box=None) as m:
        assert m.bytes == 1024 * 64
        check_stats(m.insert_cloud(xyz, rgb, EYE), ref.stats[0])
        assert not m.full
        R.assert_map_equals(m.extract(), ref)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_ragged_cloud_sizes(reg, frame, n):
    sel = np.linspace(0, len(frame["cloud"]) - 1, n).astype(np.int64)
    xyz, rgb = frame["cloud"][sel], frame["colours"][sel]
    ref = R.Map([(xyz, rgb, R.general_pose())], 0.05)
    with new_map(reg, capacity=2048) as m:
        check_stats(m.insert_cloud(xyz, rgb, R.general_pose()), ref.stats[0])
        R.assert_map_equals(m.extract(), ref)


@pytest.mark.parametrize("depth_type", ["u16", "f32"])
@pytest.mark.parametrize("with_rgb", [True, False], ids=["rgb", "no_rgb"])
def test_ragged_strided_image(reg, frame, depth_type, with_rgb):
    """200 x 100 (no multiple of the tile) as a view of wider arrays: strided rows, both depth types, with and without colour."""
    d = frame["depth"]
    metres = d.astype(np.float32) * np.float32(0.001) if d.dtype == np.uint16 else d
    wide = np.round(metres * 1000).astype(np.uint16) if depth_type == "u16" else metres.astype(np.float32)
    depth = wide[10:110, 20:220]
    rgb = frame["rgb"][10:110, 20:220] if with_rgb else None
    assert depth.strides[0] > 200 * depth.itemsize
    cloud = reg.sphere_cloud(np.ascontiguousarray(depth), 2)
    ref = R.Map([(cloud, None if rgb is None else np.ascontiguousarray(rgb).reshape(-1, 3), R.general_pose())], 0.05)
    with new_map(reg) as m:
        check_stats(m.insert_sphere(rgb, depth, R.general_pose(), convention=2), ref.stats[0])
        got = m.extract()
        R.assert_map_equals(got, ref)
        if rgb is None:
            assert not got[1].any()


@pytest.mark.parametrize("convention", [0, 1])
def test_the_other_conventions(reg, frame, convention):
    cloud = reg.sphere_cloud(frame["depth"], convention)
    ref = R.Map([(cloud, frame["colours"], EYE)], 0.05)
    with new_map(reg) as m:
        check_stats(m.insert_sphere(frame["rgb"], frame["depth"], EYE, convention=convention), ref.stats[0])
        R.assert_map_equals(m.extract(), ref)


CASES = R.edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_edge_values_on_the_device(reg, case):
    name, xyz, rgb, pose, leaf, box = case
    ref = R.Map([(xyz, rgb, pose)], leaf, box)
    with new_map(reg, leaf=leaf, capacity=256, box=box) as m:
        check_stats(m.insert_cloud(xyz, rgb, pose), ref.stats[0])
        R.assert_map_equals(m.extract(), ref, name)


def test_accumulation_does_not_depend_on_the_order(reg, frame, frame_b):
    P, Q = R.general_pose(), EYE.copy()
    Q[:3, 3] = [-0.2, 0.3, 0.1]
    a = (frame["cloud"], frame["colours"], P)
    b = (frame_b["cloud"], frame_b["colours"], Q)
    ref = R.Map([a, b], 0.05)
    outs = []
    for order in ("ab", "ba", "ab"):
        with new_map(reg) as m:
            stats = []
            for which in order:
                f, T = (frame, P) if which == "a" else (frame_b, Q)
                stats.append(m.insert_sphere(f["rgb"], f["depth"], T, convention=2))
            if order == "ab":
                check_stats(stats[0], ref.stats[0])
                check_stats(stats[1], ref.stats[1])
            outs.append(m.extract())
    R.assert_map_equals(outs[0], ref)
    for o in outs[1:]:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(outs[0], o))


def test_full_table(reg):
    from rgbd360_amd.voxel_map import MAP_FULL
    xyz, rgb = scattered_cloud(1000, 2500, seed=9)
    ref = R.Map([(xyz, rgb, EYE)], 0.05, None)
    assert len(ref) == 1000
    with new_map(reg, capacity=50, box=None) as m:
        st = m.insert_cloud(xyz, rgb, EYE)
        assert m.last_status == MAP_FULL and m.full
        assert 0 < st["n_voxels"] <= 64 and st["n_voxels"] == len(m)
        assert st["n_dropped_full"] > 0 and st["n_added"] + st["n_dropped_full"] == ref.n_passing
        assert st["n_valid"] == ref.stats[0]["n_valid"]
        got_xyz, got_rgb, got_count, got_key = m.extract()
        want = {tuple(k): int(c) for k, c in zip(ref.key.tolist(), ref.count)}
        assert len(got_count) == st["n_voxels"] and int(got_count.sum()) == st["n_added"]
        for k, c in zip(got_key.tolist(), got_count):
            assert tuple(k) in want and 0 < int(c) <= want[tuple(k)]
        # points of voxels already in the table are still added: the same cloud again adds to the resident voxels only
        st2 = m.insert_cloud(xyz, rgb, EYE)
        assert m.full and st2["n_voxels"] == st["n_voxels"] and st2["n_added"] >= st["n_added"]


def test_device_extract_truncation_clear_and_reuse(reg, hip_lib, frame):
    pose = R.general_pose()
    ref = R.Map([(frame["cloud"], frame["colours"], pose)], 0.05)
    n = len(ref)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    with new_map(reg) as m:
        m.insert_sphere(frame["rgb"], frame["depth"], pose, convention=2)
        host = m.extract()
        sizes = (n * 12, n * 3, n * 4, n * 12)
        dev = []
        for s in sizes:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), s) == 0
            dev.append(p)
        assert hip_lib.rgbd360_map_extract_dev(m._handle(), n, *dev) == n
        out = [np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint8), np.zeros(n, np.int32), np.zeros((n, 3), np.int32)]
        for a, p in zip(out, dev):
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2) == 0
        for p in dev:
            hip.hipFree(p)
        order = np.lexsort((out[3][:, 0], out[3][:, 1], out[3][:, 2]))
        R.assert_map_equals([a[order] for a in out], ref, "device extract, sorted here")
        # max_out below the size: the size comes back, max_out records are written (the first of the sorted map)
        few = m.extract(max_out=10)
        assert all(len(a) == 10 for a in few) and all(a.tobytes() == b[:10].tobytes() for a, b in zip(few, host))
        key = np.full((12, 3), -7, np.int32)
        assert hip_lib.rgbd360_map_extract(m._handle(), 10, None, None, None, key.ctypes.data_as(C.c_void_p)) == n
        assert np.array_equal(key[:10], ref.key[:10]) and (key[10:] == -7).all()
        m.clear()
        assert len(m) == 0 and all(len(a) == 0 for a in m.extract())
        check_stats(m.insert_cloud(frame["cloud"], frame["colours"], pose), ref.stats[0])
        R.assert_map_equals(m.extract(), ref, "after clear")


def test_bad_arguments_and_empty_inputs(reg, hip_lib, frame):
    from rgbd360_amd import _lib
    ctx = reg._ctx()
    h = C.c_void_p()
    assert hip_lib.rgbd360_map_create(ctx, C.c_float(0.003), 1024, C.byref(h)) == -1 and not h.value
    assert hip_lib.rgbd360_map_create(ctx, C.c_float(0.05), 0, C.byref(h)) == -1 and not h.value
    assert hip_lib.rgbd360_map_create(ctx, C.c_float(float("nan")), 16, C.byref(h)) == -1
    assert hip_lib.rgbd360_map_create(None, C.c_float(0.05), 16, C.byref(h)) == -1
    with new_map(reg) as m:      # (room for the whole frame: the last step below inserts it)
        H = m._handle()
        d = np.ascontiguousarray(frame["depth"])
        dt = 0 if d.dtype == np.uint16 else 1
        pose = np.ascontiguousarray(EYE.T.reshape(16))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        st = _lib.MapStats()
        call = lambda depth, dtype, conv, p: hip_lib.rgbd360_map_insert_sphere(H, None, 0, depth, d.strides[0], dtype, d.shape[0], d.shape[1], conv, p, 0, C.byref(st))
        assert call(vp(d), dt, 3, vp(pose)) == -1 and call(vp(d), dt, -1, vp(pose)) == -1
        assert call(vp(d), 2, 2, vp(pose)) == -1
        assert call(None, dt, 2, vp(pose)) == -1 and call(vp(d), dt, 2, None) == -1
        assert b"" != hip_lib.rgbd360_map_last_error(H)
        assert hip_lib.rgbd360_map_insert_cloud(H, None, None, 5, vp(pose), 0, C.byref(st)) == -1
        assert hip_lib.rgbd360_map_insert_cloud(H, vp(d), None, -1, vp(pose), 0, C.byref(st)) == -1
        assert hip_lib.rgbd360_map_set_box(H, vp(pose), None) == -1
        assert len(m) == 0
        # n == 0 and an empty image: 0, nothing touched
        assert hip_lib.rgbd360_map_insert_cloud(H, None, None, 0, None, 0, C.byref(st)) == 0 and st.n_voxels == 0 and st.n_valid == 0
        assert hip_lib.rgbd360_map_insert_sphere(H, None, 0, vp(d), d.strides[0], dt, 0, d.shape[1], 2, vp(pose), 0, C.byref(st)) == 0
        assert len(m) == 0
        # and the map works afterwards
        ref = R.Map([(frame["cloud"], None, EYE)], 0.05)
        check_stats(m.insert_sphere(None, frame["depth"], EYE, convention=2), ref.stats[0])
        assert not m.full
        R.assert_map_equals(m.extract(), ref, "after the refused calls")


def test_real_panorama(reg, hip_lib):
    """Frame 1 of the sample pair, stitched on the device (1920 x 320, convention 0, u16 depth, colour; a fifth of it without depth):
    default box and leaf."""
    from rgbd360_amd.register import stitch_sphere
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import config1_samples as c1
    fr = c1.frames(1, "fixture")
    rgb, depth = stitch_sphere(reg, np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), np.stack(c1.load_extrinsics("fixture")))
    assert depth.shape == (320, 1920) and depth.dtype == np.uint16
    cloud = reg.sphere_cloud(depth, 0)
    pose = R.general_pose()
    ref = R.Map([(cloud, rgb.reshape(-1, 3), pose)], 0.05)
    assert ref.stats[0]["n_valid"] < 0.85 * depth.size and len(ref) > 5000
    with new_map(reg, capacity=1 << 17) as m:
        check_stats(m.insert_sphere(rgb, depth, pose, convention=0), ref.stats[0])
        R.assert_map_equals(m.extract(), ref)


def test_odometry_replay_writes_the_map(reg, tmp_path):
    """examples/odometry_replay.cpp --map: the same pose lines as without it, and a map file that is the map of the three frames at the
    poses the loop composes.  The count-weighted mean of the file's centroids is the mean of all kept points whatever their voxels are,
    so it is compared with the restatement's at the poses of the Python host (which agree with the example's to 2e-5 m,
    test_cpp_adapter): 0.5 mm.  The frames move 6 cm and 2 degrees a step, so a replay that inserted every frame at the identity, or
    at the pose of the step before, is centimetres away from it -- asserted on the restatement, so that the comparison binds."""
    import subprocess
    from rgbd360_amd import synth
    from rgbd360_amd.batch import align_sequence
    from rgbd360_amd.register import RegisterPhotoICP
    from tests.test_cpp_adapter import build_example
    exe = build_example(tmp_path)
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "3", "256", "128"])
    plain = subprocess.run([exe, str(seq), "3", "256", "128"], text=True, capture_output=True, check=True)
    out = tmp_path / "map.txt"
    mapped = subprocess.run([exe, str(seq), "3", "256", "128", "--map", str(out), "--leaf", "0.1"], text=True, capture_output=True, check=True)
    assert mapped.stdout == plain.stdout and len(plain.stdout.splitlines()) == 2
    ignored = subprocess.run([exe, str(seq), "3", "256", "128", "--sequence", "--map", str(tmp_path / "none.txt")], text=True, capture_output=True, check=True)
    assert "--map is ignored" in ignored.stderr and not (tmp_path / "none.txt").exists()
    rows = np.loadtxt(str(out)).reshape(-1, 7)
    frames = [synth.render(synth.trajectory_pose(k, 7), 256, 128, 7) for k in range(3)]
    clouds = [reg.sphere_cloud(depth, 0) for _, depth in frames]
    host = RegisterPhotoICP()
    host.setNumPyr(4)
    rel, status, _ = align_sequence(host, lambda k: frames[k], 0, 2, 2)
    host.close()
    assert (status == 0).all()
    P1 = rel[0]
    P2 = (P1.astype(np.float64) @ rel[1].astype(np.float64)).astype(np.float32)

    def mean_point(m):
        return (m.xyz.astype(np.float64) * m.count[:, None]).sum(0) / m.count.sum()

    ref, at_identity, a_step_late = (R.Map([(c, None, T) for c, T in zip(clouds, poses)], 0.1) for poses in ((EYE, P1, P2), (EYE, EYE, EYE), (EYE, EYE, P1)))
    kept = sum(st["n_added"] for st in ref.stats)
    assert len(rows) > 1000 and (rows[:, 6] >= 1).all() and int(rows[:, 6].sum()) == kept
    assert (rows[:, 3:6] >= 0).all() and (rows[:, 3:6] <= 255).all() and rows[:, 3:6].max() > 0
    got_mean = (rows[:, :3] * rows[:, 6:7]).sum(0) / rows[:, 6].sum()
    print("mean point: file", got_mean, "restatement", mean_point(ref), "at the identity", mean_point(at_identity), "a step late", mean_point(a_step_late),
          "voxels: file", len(rows), "restatement", len(ref))
    assert min(np.linalg.norm(mean_point(x) - mean_point(ref)) for x in (at_identity, a_step_late)) > 0.01
    assert np.linalg.norm(got_mean - mean_point(ref)) < 5e-4
    assert abs(len(rows) - len(ref)) <= 0.02 * len(ref)


@pytest.fixture(scope="module")
def input_forms(reg):
    import map_input_forms as F
    forms = F.Forms(reg)
    yield forms
    forms.close()


@pytest.mark.parametrize("form", ["f32_padded", "u16", "cloud"])
def test_an_insert_from_host_and_from_device_memory_is_the_same(reg, hip_lib, input_forms, form):
    """The 1100 x 24 strip (map_input_forms.py: padded row steps, uint16 without colour, the cloud) inserted with on_device = 0 and 1:
    the same statistics and the same map, byte for byte."""
    import map_input_forms as F
    host, dev = F.edit_on_both(hip_lib, reg, input_forms, form, "insert")
    assert host == dev
