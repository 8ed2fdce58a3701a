"""Editing the resident voxel map on the device (rgbd360_map_remove_* / _move_* / _rehash / _census, csrc/map_edit.h) against the numpy
restatements (tests/voxel_map_reference.py, tests/voxel_map_edit_reference.py), bit for bit: a removal leaves the map that never saw
the frame, a revival brings it back, the readers take tombstones as absent, a rehash changes no reader's bits, and outside the
contract the counters are those of the definition and no count wraps.  The shapes are those of the insert tests
(tests/test_voxel_map_gpu.py): the smallest at which each mechanism of the kernel can fail."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import voxel_map_edit_reference as E
import voxel_map_reference as R
from test_voxel_map_gpu import scattered_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
LEAF = 0.05


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


@pytest.fixture(scope="module")
def frames(reg):
    """Three frames of the conftest pair's scene along its trajectory, each with its convention-2 cloud from the device and its pose."""
    from rgbd360_amd import synth
    out = []
    for k in range(3):
        T = synth.trajectory_pose(k)
        rgb, depth = synth.render(T, 256, 128, 1234)
        out.append(dict(rgb=rgb, depth=depth, cloud=reg.sphere_cloud(depth, 2), colours=rgb.reshape(-1, 3), pose=T.astype(np.float32)))
    return out


def triple(f, pose=None, colour=True):
    return (f["cloud"], f["colours"] if colour else None, f["pose"] if pose is None else pose)


@pytest.fixture(scope="module")
def refs(frames):
    """The restated maps the tests share, and the three classes of voxels the removal of frame 1 meets."""
    all3, without1 = R.Map([triple(f) for f in frames], LEAF), R.Map([triple(frames[0]), triple(frames[2])], LEAF)
    only1 = R.Map([triple(frames[1])], LEAF)
    touched = len(only1)
    emptied = len(all3) - len(without1)
    assert min(emptied, touched - emptied, len(all3) - touched) > 1000      # emptied, touched and surviving, untouched
    return dict(all3=all3, without1=without1, only1=only1, emptied=emptied)


def new_map(reg, leaf=LEAF, capacity=1 << 16, box="default"):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, leaf, capacity)
    if box is None:
        m.set_box(None, None)
    elif box != "default":
        m.set_box(*box)
    return m


def check_edit(got, want):
    assert {k: got[k] for k in E.EDIT_STAT_NAMES} == {k: want[k] for k in E.EDIT_STAT_NAMES}


def check_census(m, ref, tombstones):
    c = m.census()
    assert (c["n_live"], c["n_tombstones"], c["n_points"], c["n_inconsistent"]) == (len(ref), tombstones, int(ref.count.sum()), 0), c
    assert c["n_slots"] * 64 == m.bytes and len(m) == len(ref)
    return c


def insert(m, f, route="sphere", pose=None, colour=True):
    pose = f["pose"] if pose is None else pose
    if route == "sphere":
        return m.insert_sphere(f["rgb"] if colour else None, f["depth"], pose, convention=2)
    return m.insert_cloud(f["cloud"], f["colours"] if colour else None, pose)


def remove(m, f, route="sphere", pose=None, colour=True):
    pose = f["pose"] if pose is None else pose
    if route == "sphere":
        return m.remove_sphere(f["rgb"] if colour else None, f["depth"], pose, convention=2)
    return m.remove_cloud(f["cloud"], f["colours"] if colour else None, pose)


def map_without_frame_1(reg, frames, route="sphere"):
    m = new_map(reg)
    for f in frames:
        insert(m, f, route)
    st = remove(m, frames[1], route)
    return m, st


# ---- 1 exact inverse ---------------------------------------------------------------------------------------------------------------
def test_removal_is_the_exact_inverse_on_both_routes(reg, frames, refs):
    ref = refs["without1"]
    outs = []
    for route in ("sphere", "cloud"):
        m, st = map_without_frame_1(reg, frames, route)
        with m:
            assert not m.mismatch and m.last_status == 0
            assert st["n_voxels_emptied"] == refs["emptied"] and st["n_removed"] == refs["only1"].n_passing and st["n_missing"] == st["n_underflow"] == 0
            assert {k: st[k] for k in ("n_valid", "n_box_rejected", "n_out_of_range")} == {k: refs["only1"].stats[0][k] for k in ("n_valid", "n_box_rejected", "n_out_of_range")}
            assert st["n_voxels"] == len(m) == len(ref)
            got = m.extract()
            R.assert_map_equals(got, ref, route)
            check_census(m, ref, refs["emptied"])
            outs.append(got)
            if route == "sphere":       # the other two leave as well: nothing is left, and nothing is inconsistent
                remove(m, frames[0])
                st = remove(m, frames[2])
                assert not m.mismatch and st["n_voxels"] == 0 and len(m) == 0 and all(len(a) == 0 for a in m.extract())
                c = m.census()
                assert (c["n_live"], c["n_tombstones"], c["n_points"], c["n_inconsistent"]) == (0, len(refs["all3"]), 0, 0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))


# ---- 2 revival ----------------------------------------------------------------------------------------------------------------------
def test_an_insert_revives_the_tombstones(reg, frames, refs):
    m, _ = map_without_frame_1(reg, frames)
    with m:
        st = insert(m, frames[1])
        assert st["n_voxels"] == len(m) == len(refs["all3"]) and st["n_added"] == refs["only1"].n_passing and not m.full
        R.assert_map_equals(m.extract(), refs["all3"], "revived")
        check_census(m, refs["all3"], 0)      # live + tombstones as before the removal: no key holds a second slot


# ---- 3 the readers ------------------------------------------------------------------------------------------------------------------
def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_evals(hip_lib, hip, m, depth, pose):
    """Per point key3 and d2 of rgbd360_map_align_eval and rgbd360_map_align_plane_eval at `pose`, with both sets of sums."""
    from rgbd360_amd.register import pose_to_cm
    n = depth.size
    key, d2 = np.zeros((n, 3), np.int32), np.zeros(n, np.float32)
    dk, dd = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dk), key.nbytes) == 0 and hip.hipMalloc(C.byref(dd), d2.nbytes) == 0
    cm = pose_to_cm(pose)
    src = (vp(depth), depth.strides[0], 0 if depth.dtype == np.uint16 else 1, depth.shape[0], depth.shape[1], 2, None, 0)
    out = {}
    s17, c3 = np.zeros(17, np.float64), np.zeros(3, np.int64)
    p = m.align_params()
    assert hip_lib.rgbd360_map_align_eval(m._handle(), *src, vp(cm), 0, C.byref(p), vp(s17), vp(c3), dk, dd, 0, None, None) == 0
    assert hip.hipMemcpy(vp(key), dk, key.nbytes, 2) == 0 and hip.hipMemcpy(vp(d2), dd, d2.nbytes, 2) == 0
    out["point"] = (key.copy(), d2.copy(), s17, c3)
    s30, c5 = np.zeros(30, np.float64), np.zeros(5, np.int64)
    pp = m.align_plane_params()
    assert hip_lib.rgbd360_map_align_plane_eval(m._handle(), *src, vp(cm), 0, C.byref(pp), vp(s30), vp(c5), dk, dd, None, None) == 0
    assert hip.hipMemcpy(vp(key), dk, key.nbytes, 2) == 0 and hip.hipMemcpy(vp(d2), dd, d2.nbytes, 2) == 0
    out["plane"] = (key.copy(), d2.copy(), s30, c5)
    hip.hipFree(dk)
    hip.hipFree(dd)
    return out


def assert_same_readers(a, b, what):
    """Two (render, evals) results: planes, statistics, keys and d2 byte-equal; the sums (double atomics, order-dependent) to the project's
    bound for sums (2e-6 relative)."""
    (ra, ea), (rb, eb) = a, b
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ra[:4], rb[:4])) and ra[4] == rb[4], what
    for kind in ("point", "plane"):
        ka, da, sa, ca = ea[kind]
        kb, db, sb, cb = eb[kind]
        assert np.array_equal(ka, kb) and da.tobytes() == db.tobytes() and ca.tolist() == cb.tolist() and sa[0] == sb[0] > 1000, (what, kind)
        assert np.all(np.abs(sa - sb) <= 2e-6 * np.abs(sb) + 1e-9), (what, kind, sa, sb)


def readers(hip_lib, hip, m, frames):
    return m.render_sphere(128, 256, frames[2]["pose"]), device_evals(hip_lib, hip, m, frames[2]["depth"], frames[2]["pose"])


def test_readers_take_tombstones_as_absent_and_a_rehash_changes_no_bits(reg, hip_lib, hip, frames, refs):
    with new_map(reg) as fresh:
        insert(fresh, frames[0])
        insert(fresh, frames[2])
        want = readers(hip_lib, hip, fresh, frames)
    assert want[0][4]["n_voxels"] == len(refs["without1"]) and want[0][4]["n_pixels_covered"] > 10000
    m, _ = map_without_frame_1(reg, frames)
    with m:
        assert_same_readers(readers(hip_lib, hip, m, frames), want, "with tombstones")
        # rehash(0) drops exactly the tombstones, and every reader gives the bits it gave
        before = m.extract()
        assert m.rehash(0) == 0 and m.bytes == (1 << 16) * 64
        check_census(m, refs["without1"], 0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, m.extract()))
        assert_same_readers(readers(hip_lib, hip, m, frames), want, "rehashed in place")
        assert m.rehash(1 << 15) == 0 and m.bytes == (1 << 15) * 64
        assert_same_readers(readers(hip_lib, hip, m, frames), want, "rehashed into half the slots")
        R.assert_map_equals(m.extract(), refs["without1"], "rehashed twice")


# ---- 4 the kernel's mechanisms at their smallest shapes --------------------------------------------------------------------------------
def run_mirrored(reg, steps, leaf, capacity, box="default", route="cloud"):
    """steps: [("insert" | "remove", cloud, colours, pose, images or None), ...] on the device and on the restatement: statistics after
    every step, the read-out and the census after every removal."""
    mirror = E.EditMap(leaf, R.DEFAULT_BOX if box == "default" else box)
    with new_map(reg, leaf, capacity, box) as m:
        for what, cloud, colours, pose, images in steps:
            if what == "insert":
                want = mirror.insert(cloud, colours, pose)
                got = m.insert_cloud(cloud, colours, pose) if images is None else m.insert_sphere(images[0], images[1], pose, convention=2)
                assert not m.full and {k: got[k] for k in R.STAT_NAMES} == {k: want[k] for k in R.STAT_NAMES}
                continue
            want = mirror.remove(cloud, colours, pose)
            got = m.remove_cloud(cloud, colours, pose) if images is None else m.remove_sphere(images[0], images[1], pose, convention=2)
            check_edit(got, want)
            assert not m.mismatch
            ref = mirror.read_out()
            R.assert_map_equals(m.extract(), ref)
            c = mirror.census()
            check_census(m, ref, c["n_tombstones"])
    return mirror


def test_removal_from_a_strip_of_two_tiles_per_row(reg):
    """1100 x 24: a full tile and a ragged second one per row (test_a_strip_of_two_tiles_per_row), inserted at two poses; one leaves."""
    from rgbd360_amd import synth
    rgb, depth = synth.render(synth.trajectory_pose(0, 7), 1100, 24, 7)
    cloud, colours = reg.sphere_cloud(depth, 2), rgb.reshape(-1, 3)
    a = (cloud, colours, R.general_pose(), (rgb, depth))
    b = (cloud, colours, EYE, (rgb, depth))
    mirror = run_mirrored(reg, [("insert",) + a, ("insert",) + b, ("remove",) + a, ("remove",) + b], 0.1, 1 << 16)
    assert len(mirror) == 0 and len(mirror.rows) > 400


def test_removal_where_every_point_shares_a_few_voxels(reg, frames):
    """leaf 4 m, 64 slots: every workgroup takes its points off the same few count words -- the compare-and-swap loop under contention."""
    f = frames[0]
    a = (f["cloud"], f["colours"], R.general_pose(), (f["rgb"], f["depth"]))
    b = (f["cloud"], f["colours"], EYE, (f["rgb"], f["depth"]))
    mirror = run_mirrored(reg, [("insert",) + a, ("insert",) + b, ("remove",) + a, ("remove",) + b], 4.0, 64, None)
    assert 0 < len(mirror.rows) <= 54


def test_removal_with_almost_no_sharing(reg, frames):
    """64 x 32 pixels in cells of 4 mm (test_almost_no_sharing): the workgroups' tables overflow and points leave on the direct path;
    the frame is inserted twice, so the first removal leaves every voxel live and the second empties every one."""
    depth = np.ascontiguousarray(frames[0]["depth"][::4, ::4])
    rgb = np.ascontiguousarray(frames[0]["rgb"][::4, ::4])
    a = (reg.sphere_cloud(depth, 2), rgb.reshape(-1, 3), EYE, (rgb, depth))
    mirror = run_mirrored(reg, [("insert",) + a, ("insert",) + a, ("remove",) + a, ("remove",) + a], 0.004, 4096, None)
    assert len(mirror) == 0 and len(mirror.rows) > 1500


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_removal_of_ragged_clouds(reg, frames, n):
    sel = np.linspace(0, len(frames[0]["cloud"]) - 1, n).astype(np.int64)
    xyz, rgb = frames[0]["cloud"][sel], frames[0]["colours"][sel]
    a, b = (xyz, rgb, R.general_pose(), None), (xyz, rgb, EYE, None)
    run_mirrored(reg, [("insert",) + a, ("insert",) + b, ("remove",) + a], LEAF, 2048)


def test_removal_without_colour(reg, frames):
    f0, f1 = frames[0], frames[1]
    a, b = (f0["cloud"], None, f0["pose"], (None, f0["depth"])), (f1["cloud"], None, f1["pose"], (None, f1["depth"]))
    mirror = run_mirrored(reg, [("insert",) + a, ("insert",) + b, ("remove",) + b], LEAF, 1 << 16)
    assert not mirror.read_out().C.any()


def test_removal_from_a_crowded_table(reg):
    """900 voxels in 1024 slots (test_probing_near_a_full_table): the read-only lookup walks long probe runs."""
    xyz, rgb = scattered_cloud(900, 3000, seed=5)
    a, b = (xyz[:1500], rgb[:1500], EYE, None), (xyz[1500:], rgb[1500:], EYE, None)
    mirror = run_mirrored(reg, [("insert",) + a, ("insert",) + b, ("remove",) + b, ("remove",) + a], LEAF, 1024, None)
    assert len(mirror.rows) == 900


# ---- 5 move -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["sphere", "cloud"])
def test_move_takes_a_frame_to_its_true_pose(reg, frames, refs, route):
    G = R.general_pose()
    misplaced = R.Map([triple(frames[1], G)], LEAF)
    with new_map(reg) as m:
        insert(m, frames[0], route)
        insert(m, frames[1], route, pose=G)
        insert(m, frames[2], route)
        if route == "sphere":
            removed, inserted = m.move_sphere(frames[1]["rgb"], frames[1]["depth"], G, frames[1]["pose"], convention=2)
        else:
            removed, inserted = m.move_cloud(frames[1]["cloud"], frames[1]["colours"], G, frames[1]["pose"])
        assert m.last_status == 0 and not m.mismatch and not m.full
        assert removed["n_removed"] == misplaced.n_passing and removed["n_missing"] == removed["n_underflow"] == 0 and removed["n_voxels_emptied"] > 1000
        assert inserted["n_added"] == refs["only1"].n_passing and inserted["n_dropped_full"] == 0
        assert removed["n_voxels"] == inserted["n_voxels"] == len(m) == len(refs["all3"])
        R.assert_map_equals(m.extract(), refs["all3"], route)
        assert m.census()["n_inconsistent"] == 0


# ---- 6 outside the contract (deterministic cases: the counters are those of a point-by-point removal, whichever workgroup comes first) ----
def test_removing_what_the_map_does_not_hold(reg):
    from rgbd360_amd.voxel_map import MAP_MISMATCH
    A, B = scattered_cloud(900, 3000, seed=5), scattered_cloud(700, 2500, seed=6)
    refA, refB = R.Map([A + (EYE,)], LEAF, None), R.Map([B + (EYE,)], LEAF, None)
    keysA, keysB = ({tuple(k) for k in r.key.tolist()} for r in (refA, refB))
    assert (len(keysA | keysB), len(keysB - keysA), len(keysA & keysB)) == (1437, 537, 163)
    mirror = E.EditMap(LEAF, None)
    mirror.insert(*A, EYE)
    want = mirror.remove(*B, EYE)
    only_b = sum(int(c) for k, c in zip(refB.key.tolist(), refB.count) if tuple(k) not in keysA)
    assert want["n_missing"] == only_b and want["n_underflow"] > 0 and want["n_removed"] > 0
    with new_map(reg, capacity=2048, box=None) as m:
        m.insert_cloud(*A, EYE)
        got = m.remove_cloud(*B, EYE)
        assert m.last_status == MAP_MISMATCH and m.mismatch
        check_edit(got, want)
        count = m.extract()[2]
        assert len(count) == len(m) == len(mirror) and count.min() >= 1 and count.max() <= 3000
        c = m.census()
        assert (c["n_live"], c["n_tombstones"], c["n_points"]) == (len(mirror), want["n_voxels_emptied"], mirror.census()["n_points"])
        assert c["n_points"] == int(count.sum()) == refA.n_passing - want["n_removed"]


def test_removing_a_cloud_twice(reg):
    A = scattered_cloud(900, 3000, seed=5)
    with new_map(reg, capacity=2048, box=None) as m:
        m.insert_cloud(*A, EYE)
        first = m.remove_cloud(*A, EYE)
        assert not m.mismatch and first["n_removed"] == 3000 and first["n_voxels_emptied"] == 900 and len(m) == 0
        second = m.remove_cloud(*A, EYE)
        assert m.mismatch and second["n_removed"] == 0 and second["n_missing"] + second["n_underflow"] == 3000 and second["n_voxels_emptied"] == 0
        c = m.census()
        assert (c["n_live"], c["n_tombstones"], c["n_points"], c["n_inconsistent"]) == (0, 900, 0, 0)
        assert len(m) == 0 and all(len(a) == 0 for a in m.extract())


# ---- 7 rehash -----------------------------------------------------------------------------------------------------------------------
def test_rehash_grows_shrinks_and_refuses(reg):
    from rgbd360_amd.register import Rgbd360Error
    A, B = scattered_cloud(900, 3000, seed=5), scattered_cloud(700, 2500, seed=6)
    refA, refAB = R.Map([A + (EYE,)], LEAF, None), R.Map([A + (EYE,), B + (EYE,)], LEAF, None)
    with new_map(reg, capacity=1024, box=None) as m:      # grow: 1437 voxels do not fit 1024 slots
        m.insert_cloud(*A, EYE)
        assert m.rehash(4096) == 0 and m.bytes == 4096 * 64
        st = m.insert_cloud(*B, EYE)
        assert not m.full and st["n_voxels"] == len(refAB)
        R.assert_map_equals(m.extract(), refAB, "grown")
    with new_map(reg, capacity=4096, box=None) as m:      # shrink after a removal
        m.insert_cloud(*A, EYE)
        m.insert_cloud(*B, EYE)
        m.remove_cloud(*B, EYE)
        assert m.census()["n_tombstones"] == 537
        assert m.rehash(1024) == 0 and m.bytes == 1024 * 64
        R.assert_map_equals(m.extract(), refA, "shrunk")
        check_census(m, refA, 0)
        # a capacity below the occupied voxels: refused, the map unchanged
        before = m.extract()
        with pytest.raises(Rgbd360Error):
            m.rehash(512)
        assert m.bytes == 1024 * 64 and all(a.tobytes() == b.tobytes() for a, b in zip(before, m.extract()))
        # and after a rehash an insert counts its new voxels as a map without tombstones does
        assert m.rehash(4096) == 0
        st = m.insert_cloud(*B, EYE)
        assert not m.full and st["n_voxels"] == len(m) == len(refAB)
        R.assert_map_equals(m.extract(), refAB, "shrunk, grown, filled")
    # an exact fit: the whole table lies within the probe bound
    full = scattered_cloud(1024, 2000, seed=11)
    ref = R.Map([full + (EYE,)], LEAF, None)
    assert len(ref) == 1024
    with new_map(reg, capacity=2048, box=None) as m:
        m.insert_cloud(*full, EYE)
        assert m.rehash(1024) == 0 and m.bytes == 1024 * 64 and len(m) == 1024
        R.assert_map_equals(m.extract(), ref, "exact fit")
        assert m.census()["n_live"] == 1024


# ---- 8 the example ------------------------------------------------------------------------------------------------------------------
def test_odometry_replay_keeps_a_window_of_two_frames(reg, tmp_path):
    """examples/odometry_replay.cpp --map-window 2 over four frames: every `window` line is what the same inserts and removals give here at
    the poses the line carries (hexadecimal floats: exact), and the file is the map of the last two frames built fresh."""
    from rgbd360_amd import synth
    from tests.test_cpp_adapter import build_example
    exe = build_example(tmp_path)
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "4", "256", "128"])
    plain = subprocess.run([exe, str(seq), "4", "256", "128", "--map", str(tmp_path / "all.txt")], text=True, capture_output=True, check=True)
    assert "window" not in plain.stdout and len(plain.stdout.splitlines()) == 3
    out = tmp_path / "window.txt"
    run = subprocess.run([exe, str(seq), "4", "256", "128", "--map", str(out), "--map-window", "2"], text=True, capture_output=True, check=True)
    assert [l for l in run.stdout.splitlines() if not l.startswith("window")] == plain.stdout.splitlines()
    lines = [l.split() for l in run.stdout.splitlines() if l.startswith("window")]
    assert len(lines) == 4 and [int(l[1]) for l in lines] == [0, 1, 2, 3]
    assert subprocess.run([exe, str(seq), "4", "256", "128", "--map-window", "2"], capture_output=True).returncode == 2      # needs --map
    frames = [synth.render(synth.trajectory_pose(k, 7), 256, 128, 7) for k in range(4)]
    poses = []
    with new_map(reg) as m:      # the example's map: the default leaf and box
        for k, l in enumerate(lines):
            assert l[2::2][:4] == ["live", "tombstones", "emptied", "rehashed"] and l[10] == "pose"
            poses.append(np.array([float.fromhex(v) for v in l[11:27]], np.float32).reshape(4, 4).T)
            m.insert_sphere(frames[k][0], frames[k][1], poses[k], convention=0)
            emptied = m.remove_sphere(frames[k - 2][0], frames[k - 2][1], poses[k - 2], convention=0)["n_voxels_emptied"] if k >= 2 else 0
            assert not m.mismatch
            c = m.census()
            rebuilt = c["n_tombstones"] > c["n_live"]
            if rebuilt:
                assert m.rehash() == 0
                c = m.census()
            assert [int(v) for v in l[3:10:2]] == [c["n_live"], c["n_tombstones"], emptied, int(rebuilt)], (k, l, c)
        assert int(lines[3][7]) > 1000
    with new_map(reg) as fresh:
        for k in (2, 3):
            fresh.insert_sphere(frames[k][0], frames[k][1], poses[k], convention=0)
        xyz, rgb, count, _ = fresh.extract()
    want = ["%.6f %.6f %.6f %d %d %d %d" % (x, y, z, r, g, b, n) for (x, y, z), (r, g, b), n in zip(xyz.tolist(), rgb.tolist(), count.tolist())]
    assert out.read_text().splitlines() == want and len(want) == int(lines[3][3]) > 1000


@pytest.fixture(scope="module")
def input_forms(reg):
    import map_input_forms as F
    forms = F.Forms(reg)
    yield forms
    forms.close()


@pytest.mark.parametrize("op", ["remove", "move"])
@pytest.mark.parametrize("form", ["f32_padded", "u16", "cloud"])
def test_an_edit_from_host_and_from_device_memory_is_the_same(reg, hip_lib, input_forms, form, op):
    """The 1100 x 24 strip (map_input_forms.py) removed from, or moved in, a map that holds it at two poses, with on_device = 0 and 1: the
    same statistics of both kinds and the same map, byte for byte."""
    import map_input_forms as F
    host, dev = F.edit_on_both(hip_lib, reg, input_forms, form, op)
    assert host == dev
