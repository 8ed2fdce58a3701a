"""The voxel map rendered as a spherical frame (rgbd360_map_render_*, csrc/map_render.h) on the device against the numpy restatement of
its definition (tests/map_render_reference.py), bit for bit: depth, colour, count, key and the statistics; the seam, the poles and the
tie rule on single points; independence of insertion order and table capacity; a sphere scene with derivable bounds; and the
feature's point, the dense alignment of a frame against the rendered model.

Shapes: 256 x 128 and 64 x 32, leaf 0.05, tables of 2^12 .. 2^14 slots.  The room of three 256 x 128 frames holds 29 808 voxels under
the default box, which a 2^14-slot table cannot take: the bit-equality and order tests cut it with a box of +-1.3 m (about 10^4 voxels
in 2^14 slots), and the alignment test, which needs the walls, is the one test with a 2^16-slot table."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import map_render_reference as M
import voxel_map_reference as R
from test_map_render_cpu import SEAM_POLE_POINTS, sphere_scene_checks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
F = np.float32
LEAF = 0.05
SMALL_BOX = (np.array([-2.0, -1.3, -1.3], F), np.array([2.0, 1.3, 1.3], F))


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def new_map(reg, capacity=1 << 14, box=None):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, LEAF, capacity)
    if box is None:
        m.set_box(None, None)
    elif box != "default":
        m.set_box(*box)
    return m


@pytest.fixture(scope="module")
def room(reg):
    """Four frames of the synthetic room along its trajectory (256 x 128), their device clouds, colours and true poses (float32)."""
    from rgbd360_amd import synth
    frames = [synth.render(synth.trajectory_pose(k), 256, 128) for k in range(4)]
    return dict(frames=frames, clouds=[reg.sphere_cloud(d, 2) for _, d in frames], colours=[rgb.reshape(-1, 3) for rgb, _ in frames],
                poses=[synth.trajectory_pose(k).astype(F) for k in range(4)], truth=[synth.trajectory_pose(k) for k in range(4)])


@pytest.fixture(scope="module")
def room_map(reg, room):
    """Frames 0-2 in a 2^14-slot table under SMALL_BOX, with the restatement's map; shared and never written after this."""
    ref = R.Map([(room["clouds"][k], room["colours"][k], room["poses"][k]) for k in range(3)], LEAF, SMALL_BOX)
    assert 8000 < len(ref) < 0.8 * (1 << 14) and ref.count.max() > 20
    m = new_map(reg, box=SMALL_BOX)
    for k in range(3):
        rgb, depth = room["frames"][k]
        m.insert_sphere(rgb, depth, room["poses"][k], convention=2)
        assert not m.full
    yield m, ref
    m.close()


@pytest.mark.parametrize("rows,cols,params", [(128, 256, {}), (128, 256, dict(splat=0.0)), (128, 256, dict(max_half=0)), (128, 256, dict(min_count=3)),
                                              (32, 64, {}), (128, 256, dict(splat=3.0, max_half=5, near=1.0))],
                         ids=["defaults", "splat0", "max_half0", "min_count3", "64x32", "wide"])
def test_render_equals_the_restatement(room, room_map, rows, cols, params):
    m, ref = room_map
    want = M.render(ref, LEAF, rows, cols, room["poses"][3], **params)
    got = m.render_sphere(rows, cols, room["poses"][3], **params)
    print(params, got[4])
    assert want["stats"]["n_splatted"] > 1000 and want["stats"]["n_pixels_covered"] > (rows * cols) // 8
    if "min_count" in params:
        assert want["stats"]["n_below_min_count"] > 1000
    if not params and rows == 128:          # the footprints differ: single pixels far away, several pixels close by, and they overlap
        assert want["n_atomics"] > 1.5 * want["stats"]["n_splatted"] and want["n_atomics"] > want["stats"]["n_pixels_covered"]
    M.assert_render_equals(got, want, str(params))


def test_seam_and_poles(reg):
    rows, cols = 32, 64
    xyz = np.array(SEAM_POLE_POINTS, F)
    rgb = np.array([[10 * k + 1, 10 * k + 2, 10 * k + 3] for k in range(len(xyz))], np.uint8)
    ref = R.Map([(xyz, rgb, EYE)], LEAF, None)
    want = M.render(ref, LEAF, rows, cols, EYE)
    with new_map(reg, 1 << 12) as m:
        m.insert_cloud(xyz, rgb, EYE)
        got = m.render_sphere(rows, cols, EYE)
    M.assert_render_equals(got, want)
    owner = got[1][..., 0]
    cols_of = lambda k: set(np.nonzero((owner == 10 * k + 1).any(axis=0))[0].tolist())
    rows_of = lambda k: set(np.nonzero((owner == 10 * k + 1).any(axis=1))[0].tolist())
    assert {62, 63, 0, 1} <= cols_of(0) and {62, 63, 0, 1} <= cols_of(1)          # the footprints wrap in columns ...
    assert min(rows_of(2)) == 0 and len(rows_of(2)) >= 3 and max(rows_of(3)) == rows - 1 and len(rows_of(3)) >= 3      # ... and clip in rows


def test_tie_goes_to_the_smaller_key_whatever_the_order_and_capacity(reg):
    a, z = 2.0 ** -4, 0.25
    pts = np.array([(0.0, a, -z), (0.0, -a, -z)], F)
    rgb = np.array([[200, 0, 0], [0, 200, 0]], np.uint8)
    ref = R.Map([(pts, rgb, EYE)], LEAF, None)
    want = M.render(ref, LEAF, 32, 64, EYE, splat=4.0)
    renders = []
    for capacity in (1 << 12, 1 << 13):
        for order in ([0, 1], [1, 0]):
            with new_map(reg, capacity) as m:
                for k in order:
                    m.insert_cloud(pts[k:k + 1], rgb[k:k + 1], EYE)
                renders.append(m.render_sphere(32, 64, EYE, splat=4.0))
    depth, _, count, key3, _ = renders[0]
    bits = np.unique(depth[count > 0].view(np.uint32))
    assert len(bits) == 1          # both voxels have the same dist bits
    own = [(key3 == k).all(axis=2) & (count > 0) for k in ref.key]
    assert own[0].sum() > own[1].sum() > 0 and M.packed_keys(ref.key)[0] < M.packed_keys(ref.key)[1]          # the shared pixels carry the smaller key
    M.assert_render_equals(renders[0], want)
    for other in renders[1:]:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(renders[0][:4], other[:4])) and other[4] == renders[0][4]


def test_render_does_not_depend_on_the_order_of_insertion(reg, room, room_map):
    m, _ = room_map
    first = m.render_sphere(128, 256, room["poses"][3])
    with new_map(reg, box=SMALL_BOX) as m2:
        for k in (2, 0, 1):
            rgb, depth = room["frames"][k]
            m2.insert_sphere(rgb, depth, room["poses"][k], convention=2)
        second = m2.render_sphere(128, 256, room["poses"][3])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first[:4], second[:4])) and first[4] == second[4]


def test_sphere_scene(reg):
    """A frame of constant range R inserted and rendered at the same pose: every rendered dist lies in [R - leaf sqrt 3, R (1 + 2^-20)]
    (a centroid lies in the convex hull of points at range R within one cell), and the rows within 30 degrees of the equator have no
    hole (a centroid lies within leaf sqrt 3 of every surface point of its cell, and 2.5 cos 30 > sqrt 3).  Both hold on the
    restatement (tests/test_map_render_cpu.py)."""
    rows, cols, radius = 128, 256, 1.5
    depth = np.full((rows, cols), radius, F)
    P = R.general_pose()
    with new_map(reg) as m:
        st = m.insert_sphere(None, depth, P, convention=2)
        assert not m.full and st["n_added"] == rows * cols
        d, rgb, count, key3, stats = m.render_sphere(rows, cols, P, splat=2.5, max_half=32)
    print(stats, d[count > 0].min(), d[count > 0].max())
    sphere_scene_checks(dict(depth=d, count=count), rows, cols, radius, LEAF)


def test_dev_entry_equals_the_host_entry(hip_lib, hip, room, room_map):
    from rgbd360_amd import _lib
    from rgbd360_amd.register import pose_to_cm
    m, _ = room_map
    rows, cols = 128, 256
    n = rows * cols
    host = m.render_sphere(rows, cols, room["poses"][3])
    sizes = [4 * n, 3 * n, 4 * n, 12 * n, 40]
    dev = [C.c_void_p() for _ in sizes]
    for p, s in zip(dev, sizes):
        assert hip.hipMalloc(C.byref(p), s) == 0
    cm = pose_to_cm(room["poses"][3])
    rc = hip_lib.rgbd360_map_render_sphere_dev(m._handle(), rows, cols, cm.ctypes.data_as(C.c_void_p), None, *dev)
    assert rc == 0
    assert hip_lib.rgbd360_sync(m._reg._ctx()) == 0
    out = [np.zeros((rows, cols), F), np.zeros((rows, cols, 3), np.uint8), np.zeros((rows, cols), np.int32), np.zeros((rows, cols, 3), np.int32),
           np.zeros(5, np.int64)]
    for a, p, s in zip(out, dev, sizes):
        assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, s, 2) == 0
        hip.hipFree(p)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(host[:4], out[:4]))
    assert out[4].tolist() == [host[4][k] for k in M.STAT_NAMES]


def test_empty_map_bad_arguments_and_sizes(hip_lib, reg, room, room_map):
    from rgbd360_amd import _lib
    from rgbd360_amd.register import Rgbd360Error, pose_to_cm
    with new_map(reg, 1 << 12) as m:
        d, rgb, count, key3, stats = m.render_sphere(32, 64, EYE)
        assert not d.any() and not rgb.any() and not count.any() and not key3.any() and stats == dict.fromkeys(M.STAT_NAMES, 0)
        d, _, _, _, stats = m.render_sphere(0, 64, EYE)
        assert d.shape == (0, 64) and stats == dict.fromkeys(M.STAT_NAMES, 0)
        for bad in (dict(min_count=0), dict(max_half=-1), dict(max_half=65), dict(splat=-0.5), dict(splat=float("nan")), dict(near=-1.0)):
            with pytest.raises(Rgbd360Error, match=r"\(-1\): .*(min_count|max_half|splat|near)"):
                m.render_sphere(32, 64, EYE, **bad)
        for rows, cols in ((1, 64), (32, 4), (-1, 64), (4096, 4096), (2, 32768)):
            with pytest.raises(Rgbd360Error, match=r"\(-1\): .*(image|size)"):
                m.render_sphere(rows, cols, EYE)
        buf = np.zeros(32 * 64, F)
        assert hip_lib.rgbd360_map_render_sphere(m._handle(), 32, 64, None, None, buf.ctypes.data_as(C.c_void_p), None, None, None, None) == -1
        assert b"pose" in hip_lib.rgbd360_map_last_error(m._handle())
    # a second render at another size, smaller and larger, re-uses or grows the planes; any output may be left out
    m, ref = room_map
    pose = room["poses"][3]
    for rows, cols in ((32, 64), (128, 256), (32, 64)):
        M.assert_render_equals(m.render_sphere(rows, cols, pose), M.render(ref, LEAF, rows, cols, pose), "%d x %d" % (rows, cols))
    count = np.zeros((32, 64), np.int32)
    cm = pose_to_cm(pose)
    assert hip_lib.rgbd360_map_render_sphere(m._handle(), 32, 64, cm.ctypes.data_as(C.c_void_p), None, None, None, count.ctypes.data_as(C.c_void_p), None, None) == 0
    assert np.array_equal(count, M.render(ref, LEAF, 32, 64, pose)["count"])


def test_the_table_is_read_only(reg, room):
    rgb, depth = room["frames"][0]
    with new_map(reg, box=SMALL_BOX) as m:
        m.insert_sphere(rgb, depth, room["poses"][0], convention=2)
        before = m.extract()
        m.render_sphere(128, 256, room["poses"][3])
        m.render_sphere(32, 64, room["poses"][1], splat=3.0, min_count=2)
        after = m.extract()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        rgb_b, depth_b = room["frames"][1]
        m.insert_sphere(rgb_b, depth_b, room["poses"][1], convention=2)
        ref = R.Map([(room["clouds"][k], room["colours"][k], room["poses"][k]) for k in range(2)], LEAF, SMALL_BOX)
        R.assert_map_equals(m.extract(), ref, "insertion after a render")


def test_frame_to_model_alignment(reg, room):
    """Frames 0-2 at their true poses, the map rendered at pose 2 as the dense alignment's target, frame 3 aligned from the identity:
    the status is OK and the pose is closer to the truth than the guess in rotation and in translation.  The errors and those of the
    frame-to-frame alignment from the same guess are printed (recorded in DESIGN.md 3.14, not asserted)."""
    from rgbd360_amd import synth
    truth = np.linalg.inv(room["truth"][2]) @ room["truth"][3]          # source (frame 3) points -> target (pose 2) frame
    with new_map(reg, 1 << 16, box="default") as m:
        for k in range(3):
            rgb, depth = room["frames"][k]
            m.insert_sphere(rgb, depth, room["poses"][k], convention=2)
            assert not m.full
        depth, rgb, count, _, stats = m.render_sphere(128, 256, room["poses"][2])
    print("render", stats)
    rgb3, depth3 = room["frames"][3]
    reg.setTargetFrame(rgb, depth)
    reg.setSourceFrame(rgb3, depth3)
    status = reg.alignFrames360(np.eye(4), reg.PHOTO_DEPTH)
    model = synth.pose_error(reg.getOptimalPose(), truth)
    guess = synth.pose_error(np.eye(4), truth)
    reg.setTargetFrame(*room["frames"][2])
    status_ff = reg.alignFrames360(np.eye(4), reg.PHOTO_DEPTH)
    frame = synth.pose_error(reg.getOptimalPose(), truth)
    print("pose errors (rad, m): guess %.3e %.3e  frame-to-model %.3e %.3e (status %d)  frame-to-frame %.3e %.3e (status %d)  covered %d of %d pixels"
          % (guess + model + (status,) + frame + (status_ff,) + (stats["n_pixels_covered"], depth.size)))
    assert status == 0
    assert model[0] < guess[0] and model[1] < guess[1]


def test_odometry_replay_renders_the_map(reg, tmp_path):
    """examples/odometry_replay.cpp --map F --render-map P: the pose lines are what they are without the option, and P_rgb.ppm and
    P_depth.pfm have the size of a 256 x 128 frame behind their headers."""
    from tests.test_cpp_adapter import build_example
    exe = build_example(tmp_path)
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "3", "256", "128"])
    base = [exe, str(seq), "3", "256", "128", "--map"]
    plain = subprocess.run(base + [str(tmp_path / "a.txt")], text=True, capture_output=True, check=True)
    prefix = tmp_path / "view"
    shown = subprocess.run(base + [str(tmp_path / "b.txt"), "--render-map", str(prefix)], text=True, capture_output=True, check=True)
    lines = shown.stdout.splitlines()
    assert [l for l in lines if not l.startswith("render")] == plain.stdout.splitlines()
    words = [l for l in lines if l.startswith("render")][0].split()
    st = dict(zip(words[1::2], map(int, words[2::2])))
    assert st["voxels"] > 5000 and st["splatted"] > 5000 and 256 * 128 // 4 < st["pixels_covered"] <= 256 * 128
    ppm, pfm = (tmp_path / "view_rgb.ppm").read_bytes(), (tmp_path / "view_depth.pfm").read_bytes()
    assert ppm.startswith(b"P6\n256 128\n255\n") and len(ppm) == len(b"P6\n256 128\n255\n") + 256 * 128 * 3
    assert pfm.startswith(b"Pf\n256 128\n-1.0\n") and len(pfm) == len(b"Pf\n256 128\n-1.0\n") + 256 * 128 * 4
    depth = np.frombuffer(pfm[len(b"Pf\n256 128\n-1.0\n"):], F)
    assert int((depth > 0).sum()) == st["pixels_covered"] and depth.max() < 8.0
    no_map = subprocess.run([exe, str(seq), "3", "256", "128", "--render-map", str(prefix)], text=True, capture_output=True)
    assert no_map.returncode == 2 and "--render-map needs --map" in no_map.stderr
