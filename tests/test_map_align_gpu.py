"""The alignment of a frame against the voxel map (rgbd360_map_align_*, csrc/map_align.h) on the device against the numpy restatement
of its definition (tests/map_align_reference.py): per point the matched key and d2 bit for bit, exact counters, the 17 sums to the
project's bound for sums (2e-6 relative; H to 2e-5 max|H|), and the whole loop: status, iteration count, the matches per
iteration, and the pose to the device-mode bound (5e-6 rad, 5e-6 m)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import map_align_reference as A
import voxel_map_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
SEED = 6          # tests/test_map_align_cpu.py: every stop / continue decision of the restatement is a factor > 3 from eps
POSE_TOL = 5e-6


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


def new_map(reg, leaf=0.05, capacity=1 << 16, box="default"):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, leaf, capacity)
    if box is None:
        m.set_box(None, None)
    elif box != "default":
        m.set_box(*box)
    return m


@pytest.fixture(scope="module")
def frame(reg, small_pair):
    rgb, depth = small_pair[0]
    return dict(rgb=rgb, depth=depth, cloud=reg.sphere_cloud(depth, 2))


@pytest.fixture(scope="module")
def world(reg, frame):
    """The frame in maps of 0.05 m and 0.2 m at the general pose, on the device and restated.  An alignment never changes a map, so
    the tests share them (test_the_table_is_read_only holds that)."""
    P = R.general_pose()
    maps = {leaf: new_map(reg, leaf) for leaf in (0.05, 0.2)}
    for m in maps.values():
        m.insert_sphere(None, frame["depth"], P, convention=2)
    yield dict(P=P, guess=A.perturbed(P, 0.01, 0.003, SEED), dev=maps, ref={leaf: R.Map([(frame["cloud"], None, P)], leaf) for leaf in maps})
    for m in maps.values():
        m.close()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_eval(hip_lib, hip, m, pose, depth=None, convention=2, xyz=None, **params):
    """rgbd360_map_align_eval: (key3, d2, sums, counters dict)."""
    from rgbd360_amd.register import pose_to_cm
    n = depth.size if depth is not None else len(xyz)
    key, d2 = np.zeros((max(n, 1), 3), np.int32), np.zeros(max(n, 1), np.float32)
    dk, dd = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dk), key.nbytes) == 0 and hip.hipMalloc(C.byref(dd), d2.nbytes) == 0
    sums, counters = np.zeros(17, np.float64), np.zeros(3, np.int64)
    p = m.align_params(**params)
    cm = pose_to_cm(pose)
    if depth is not None:
        rc = hip_lib.rgbd360_map_align_eval(m._handle(), vp(depth), depth.strides[0], 0 if depth.dtype == np.uint16 else 1, depth.shape[0], depth.shape[1],
                                            convention, None, 0, vp(cm), 0, C.byref(p), vp(sums), vp(counters), dk, dd, 0, None, None)
    else:
        x = np.ascontiguousarray(xyz, np.float32)
        rc = hip_lib.rgbd360_map_align_eval(m._handle(), None, 0, 0, 0, 0, 0, vp(x), len(x), vp(cm), 0, C.byref(p), vp(sums), vp(counters), dk, dd, 0, None, None)
    assert rc == 0, (rc, hip_lib.rgbd360_map_last_error(m._handle()))
    assert hip.hipMemcpy(vp(key), dk, key.nbytes, 2) == 0 and hip.hipMemcpy(vp(d2), dd, d2.nbytes, 2) == 0
    hip.hipFree(dk)
    hip.hipFree(dd)
    return key[:n], d2[:n], sums, dict(zip(("n_valid", "n_box_rejected", "n_out_of_range"), counters.tolist()))


def check_eval(got, ref, what=""):
    key, d2, sums, counters = got
    assert np.array_equal(key, ref.key3), what
    assert d2.tobytes() == ref.d2.tobytes(), what
    assert counters == ref.counters, what
    assert sums[0] == ref.n, what
    print(what, "n", ref.n, "largest relative difference of a sum", np.max(np.abs(sums - ref.sums) / np.maximum(np.abs(ref.sums), 1e-300)))
    assert np.all(np.abs(sums - ref.sums) <= 2e-6 * np.abs(ref.sums) + 1e-9), (what, sums, ref.sums)


def check_normal_equations(H, g, ref_H, ref_g):
    assert np.abs(H - ref_H).max() <= 2e-5 * np.abs(ref_H).max()
    assert np.abs(g - ref_g).max() <= 2e-5 * max(np.abs(ref_g).max(), 1e-30) + 2e-6 * np.abs(ref_H).max() * 1e-3


@pytest.mark.parametrize("at", ["map_pose", "perturbed"])
@pytest.mark.parametrize("leaf", [0.05, 0.2])
def test_evaluation_equals_the_restatement_and_the_cloud_route(hip_lib, hip, frame, world, leaf, at):
    pose = world["P"] if at == "map_pose" else world["guess"]
    ref = A.Evaluation(world["ref"][leaf], frame["cloud"], pose, leaf, R.DEFAULT_BOX, leaf)
    assert ref.n > 15000 and ref.counters["n_box_rejected"] > 0
    a = device_eval(hip_lib, hip, world["dev"][leaf], pose, depth=frame["depth"])
    check_eval(a, ref, "sphere")
    b = device_eval(hip_lib, hip, world["dev"][leaf], pose, xyz=frame["cloud"])
    check_eval(b, ref, "cloud")
    assert a[2].tobytes() != b"" and np.array_equal(a[0], b[0])


def test_evaluation_at_the_identity(hip_lib, hip, reg, frame):
    ref_map = R.Map([(frame["cloud"], None, EYE)], 0.05)
    shifted = EYE.copy()
    shifted[:3, 3] = [0.004, -0.003, 0.002]
    with new_map(reg) as m:
        m.insert_sphere(None, frame["depth"], EYE, convention=2)
        for pose in (EYE, shifted):
            check_eval(device_eval(hip_lib, hip, m, pose, depth=frame["depth"]), A.Evaluation(ref_map, frame["cloud"], pose, 0.05, R.DEFAULT_BOX, 0.05))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_ragged_cloud_sizes(hip_lib, hip, frame, world, n):
    valid = np.nonzero(np.isfinite(frame["cloud"]).all(axis=1))[0]
    xyz = frame["cloud"][valid[np.linspace(0, len(valid) - 1, n).astype(np.int64)]]
    ref = A.Evaluation(world["ref"][0.05], xyz, world["guess"], 0.05, R.DEFAULT_BOX, 0.05)
    check_eval(device_eval(hip_lib, hip, world["dev"][0.05], world["guess"], xyz=xyz), ref)


@pytest.mark.parametrize("depth_type", ["u16", "f32"])
def test_ragged_strided_image(hip_lib, hip, reg, frame, world, depth_type):
    """200 x 100 (no multiple of the tile) as a view of a wider array, both depth types."""
    d = frame["depth"]
    metres = d.astype(np.float32) * np.float32(0.001) if d.dtype == np.uint16 else d
    wide = np.round(metres * 1000).astype(np.uint16) if depth_type == "u16" else metres.astype(np.float32)
    depth = wide[10:110, 20:220]
    assert depth.strides[0] > 200 * depth.itemsize
    # (the view's columns are not the full turn: its own cloud, from the device's tables for 200 columns)
    cloud = reg.sphere_cloud(np.ascontiguousarray(depth), 2)
    with new_map(reg) as m:
        m.insert_cloud(cloud, None, world["P"])
        ref = A.Evaluation(R.Map([(cloud, None, world["P"])], 0.05), cloud, world["guess"], 0.05, R.DEFAULT_BOX, 0.05)
        assert ref.n > 5000
        check_eval(device_eval(hip_lib, hip, m, world["guess"], depth=depth), ref)


def test_a_strip_of_two_tiles_per_row(hip_lib, hip, reg, world):
    """1100 x 24: a full tile and a ragged second one of 76 columns per row, the smallest shape in which all four point slots of a thread
    and the second blockIdx.x of the sphere route hold pixels (at 256 and 200 columns only the first slot ever does)."""
    from rgbd360_amd import synth
    depth = synth.render(synth.trajectory_pose(0, 7), 1100, 24, 7)[1]
    cloud = reg.sphere_cloud(depth, 2)
    with new_map(reg, 0.1) as m:
        m.insert_sphere(None, depth, world["P"], convention=2)
        ref = A.Evaluation(R.Map([(cloud, None, world["P"])], 0.1), cloud, world["guess"], 0.1, R.DEFAULT_BOX, 0.1)
        assert ref.n > 5000
        check_eval(device_eval(hip_lib, hip, m, world["guess"], depth=depth), ref)


@pytest.mark.parametrize("convention", [0, 1])
def test_the_other_conventions(hip_lib, hip, reg, frame, world, convention):
    cloud = reg.sphere_cloud(frame["depth"], convention)
    with new_map(reg) as m:
        m.insert_cloud(cloud, None, EYE)
        shifted = EYE.copy()
        shifted[:3, 3] = [0.004, -0.003, 0.002]
        ref = A.Evaluation(R.Map([(cloud, None, EYE)], 0.05), cloud, shifted, 0.05, R.DEFAULT_BOX, 0.05)
        assert ref.n > 5000
        check_eval(device_eval(hip_lib, hip, m, shifted, depth=frame["depth"], convention=convention), ref)


CASES = R.edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_edge_values_on_the_device(hip_lib, hip, reg, case):
    """The map's edge values (NaN, +-Inf, the box limits, |w| at 4096) and negative voxel indices: the case's cloud against its own map,
    at the case's pose and a hair beside it."""
    name, xyz, rgb, pose, leaf, box = case
    ref_map = R.Map([(xyz, rgb, pose)], leaf, box)
    beside = np.array(pose, np.float32)
    beside[:3, 3] += np.float32(0.3 * leaf) * np.array([1, -1, 1], np.float32)
    with new_map(reg, leaf=leaf, capacity=256, box=box) as m:
        m.insert_cloud(xyz, rgb, pose)
        for T in (pose, beside):
            ref = A.Evaluation(ref_map, xyz, T, leaf, box, leaf)
            check_eval(device_eval(hip_lib, hip, m, T, xyz=xyz), ref, name)
    if name.startswith("signs"):
        assert ref_map.key.min() < 0 and ref.n > 0


def test_a_tie_goes_to_the_earlier_candidate(hip_lib, hip, reg):
    """Cells of 0.25 m (inv_leaf = 4 exactly) and binary fractions: the distances are exact."""
    target = np.array([(0.125, 0.125, 0.125), (0.375, 0.125, 0.125), (0.875, 0.125, 0.125), (1.375, 0.125, 0.125)], np.float32)
    # 0.25: in cell 1, midway between the centroids of cells 0 and 1 -> the centre cell comes first: cell 1
    # 1.125: in the empty cell 4, midway between the centroids of cells 3 (dx = -1) and 5 (dx = +1) -> dx = -1 comes first: cell 3
    query = np.array([(0.25, 0.125, 0.125), (1.125, 0.125, 0.125)], np.float32)
    ref_map = R.Map([(target, None, EYE)], 0.25, None)
    assert ref_map.key[:, 0].tolist() == [0, 1, 3, 5]
    ref = A.Evaluation(ref_map, query, EYE, 0.25, None, 0.25)
    assert ref.key3.tolist() == [[1, 0, 0], [3, 0, 0]] and ref.d2.tolist() == [0.015625, 0.0625]
    with new_map(reg, leaf=0.25, capacity=64, box=None) as m:
        m.insert_cloud(target, None, EYE)
        got = device_eval(hip_lib, hip, m, EYE, xyz=query)
        check_eval(got, ref)
        # d2 == max_dist^2 is kept; the next float below max_dist drops the second point
        less = device_eval(hip_lib, hip, m, EYE, xyz=query, max_dist=float(np.nextafter(np.float32(0.25), np.float32(0))))
        check_eval(less, A.Evaluation(ref_map, query, EYE, 0.25, None, np.nextafter(np.float32(0.25), np.float32(0))))
        assert less[0].tolist() == [[1, 0, 0], [A.NO_KEY] * 3]


def test_min_count_ignores_singletons(hip_lib, hip, frame, world):
    ref1 = A.Evaluation(world["ref"][0.05], frame["cloud"], world["guess"], 0.05, R.DEFAULT_BOX, 0.05, 1)
    ref2 = A.Evaluation(world["ref"][0.05], frame["cloud"], world["guess"], 0.05, R.DEFAULT_BOX, 0.05, 2)
    assert (world["ref"][0.05].count == 1).sum() > 1000 and not np.array_equal(ref1.key3, ref2.key3) and 0 < ref2.n < ref1.n
    check_eval(device_eval(hip_lib, hip, world["dev"][0.05], world["guess"], depth=frame["depth"], min_count=2), ref2)


def test_lookups_in_a_nearly_full_table(hip_lib, hip, reg):
    """900 voxels in 1024 slots (above 85 % load): a lookup walks past foreign keys, a missing key's ends at an empty slot or at the
    bound (the whole table here)."""
    from test_voxel_map_gpu import scattered_cloud
    xyz, rgb = scattered_cloud(900, 3000, seed=5)
    ref_map = R.Map([(xyz, rgb, EYE)], 0.05, None)
    assert len(ref_map) == 900
    shifted = EYE.copy()
    shifted[:3, 3] = [0.02, 0.015, -0.02]
    with new_map(reg, capacity=1024, box=None) as m:
        m.insert_cloud(xyz, rgb, EYE)
        assert not m.full
        for T in (EYE, shifted):
            ref = A.Evaluation(ref_map, xyz, T, 0.05, None, 0.05)
            assert ref.n > 2000
            check_eval(device_eval(hip_lib, hip, m, T, xyz=xyz), ref)
    # and a table that is full to the last slot: every lookup of a missing key runs into the bound
    xyz2, _ = scattered_cloud(64, 200, seed=3)
    ref_map = R.Map([(xyz2, None, EYE)], 0.05, None)
    with new_map(reg, capacity=64, box=None) as m:
        m.insert_cloud(xyz2, None, EYE)
        assert len(m) == 64 and not m.full
        check_eval(device_eval(hip_lib, hip, m, shifted, xyz=xyz2), A.Evaluation(ref_map, xyz2, shifted, 0.05, None, 0.05))


def test_an_empty_map(hip_lib, hip, reg, frame, world):
    from rgbd360_amd.register import pose_from_cm
    with new_map(reg) as m:
        ref = A.Evaluation(R.Map([], 0.05), frame["cloud"], world["guess"], 0.05, R.DEFAULT_BOX, 0.05)
        assert ref.n == 0 and ref.counters["n_valid"] > 0
        check_eval(device_eval(hip_lib, hip, m, world["guess"], depth=frame["depth"]), ref)
        pose, res = m.align_sphere(frame["depth"], world["guess"], convention=2)
        assert res["status"] == A.NO_VALID_PIXELS and res["iterations"] == 0 and res["n_matched"] == 0 and res["fitness"] == 0.0
        assert pose.tobytes() == world["guess"].tobytes() and res["n_valid"] == ref.counters["n_valid"] and len(m) == 0


def check_alignment(m, run, ref, P=None):
    pose, res = run()
    trace = m.align_trace()
    print("status", res["status"], "iterations", res["iterations"], "converged", res["converged"], "matches", [t[0] for t in trace], "restated",
          [t[0] for t in ref.trace], "margins", ref.margins, "pose difference", A.pose_error(pose, ref.pose))
    assert (res["status"], res["iterations"], res["converged"]) == (ref.status, ref.iterations, ref.converged)
    assert [t[0] for t in trace] == [t[0] for t in ref.trace]
    assert all(mg >= 2.0 for mg in ref.margins)
    for (n, ss, u), (rn, rss, ru) in zip(trace, ref.trace):
        assert abs(ss - rss) <= 2e-6 * rss + 1e-12 and np.abs(u - ru).max() <= POSE_TOL
    dr, dt = A.pose_error(pose, ref.pose)
    assert dr <= POSE_TOL and dt <= POSE_TOL
    assert res["n_matched"] == ref.n_matched and abs(res["fitness"] - ref.fitness) <= 2e-6 * ref.fitness + 1e-15
    for k in ("n_valid", "n_box_rejected", "n_out_of_range"):
        assert res[k] == ref.final.counters[k]
    if ref.n_matched:
        check_normal_equations(res["hessian"], res["gradient"], ref.hessian, ref.gradient)
    if P is not None:
        (r1, t1), (r0, t0) = A.pose_error(pose, P), A.pose_error(ref.pose, P)
        assert r1 <= r0 + POSE_TOL and t1 <= t0 + POSE_TOL
    # the same bytes from run to run
    pose2, res2 = run()
    trace2 = m.align_trace()
    assert pose2.tobytes() == pose.tobytes() and all(np.array_equal(np.asarray(res[k]), np.asarray(res2[k])) for k in res)
    assert len(trace) == len(trace2) and all(a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() for a, b in zip(trace, trace2))
    return pose, res


@pytest.mark.parametrize("route", ["sphere", "cloud"])
@pytest.mark.parametrize("leaf", [0.05, 0.2])
def test_the_whole_loop(frame, world, leaf, route):
    m = world["dev"][leaf]
    ref = A.Alignment(world["ref"][leaf], frame["cloud"], world["guess"], leaf, R.DEFAULT_BOX, leaf)
    assert ref.status == A.OK and ref.converged == 1 and ref.iterations >= 2
    run = (lambda: m.align_sphere(frame["depth"], world["guess"], convention=2)) if route == "sphere" else (lambda: m.align_cloud(frame["cloud"], world["guess"]))
    pose, res = check_alignment(m, run, ref, world["P"])
    r0, t0 = A.pose_error(world["guess"], world["P"])
    r1, t1 = A.pose_error(pose, world["P"])
    assert r1 <= 0.5 * r0 and t1 <= 0.5 * t0


def test_the_iteration_limit(frame, world):
    m = world["dev"][0.05]
    ref = A.Alignment(world["ref"][0.05], frame["cloud"], world["guess"], 0.05, R.DEFAULT_BOX, 0.05, max_iters=1)
    assert ref.iterations == 1 and ref.converged == 0 and ref.status == A.OK
    check_alignment(m, lambda: m.align_sphere(frame["depth"], world["guess"], convention=2, max_iters=1), ref)
    # no step at all: the final evaluation only, pose_out = guess
    ref0 = A.Alignment(world["ref"][0.05], frame["cloud"], world["guess"], 0.05, R.DEFAULT_BOX, 0.05, max_iters=0)
    pose, res = check_alignment(m, lambda: m.align_sphere(frame["depth"], world["guess"], convention=2, max_iters=0), ref0)
    assert pose.tobytes() == world["guess"].tobytes() and res["iterations"] == 0 and res["n_matched"] > 15000 and m.align_trace() == []


def test_the_table_is_read_only(reg, frame, world, small_pair):
    P = world["P"]
    with new_map(reg) as m:
        m.insert_sphere(frame["rgb"], frame["depth"], P, convention=2)
        before = m.extract()
        m.align_sphere(frame["depth"], world["guess"], convention=2)
        m.align_cloud(frame["cloud"], world["guess"], min_count=2)
        after = m.extract()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        rgb_b, depth_b = small_pair[1]
        Q = EYE.copy()
        Q[:3, 3] = [-0.2, 0.3, 0.1]
        m.insert_sphere(rgb_b, depth_b, Q, convention=2)
        ref = R.Map([(frame["cloud"], frame["rgb"].reshape(-1, 3), P), (reg.sphere_cloud(depth_b, 2), rgb_b.reshape(-1, 3), Q)], 0.05)
        R.assert_map_equals(m.extract(), ref, "insertion after an alignment")


def test_degenerate_inputs(hip_lib, reg, frame, world):
    from rgbd360_amd import _lib
    from rgbd360_amd.register import pose_to_cm
    # all points on a line through the origin along x: the rotation about it is not observable, H has an exact zero row
    line = np.zeros((200, 3), np.float32)
    line[:, 0] = np.linspace(-1.0, 1.0, 200, dtype=np.float32)
    ref_map = R.Map([(line, None, EYE)], 0.05, None)
    with new_map(reg, box=None) as m:
        m.insert_cloud(line, None, EYE)
        guess = EYE.copy()
        guess[0, 3] = 0.01
        ref = A.Alignment(ref_map, line, guess, 0.05, None, 0.05)
        assert ref.status == A.ILL_POSED and ref.iterations == 0 and ref.n_matched > 100
        pose, res = check_alignment(m, lambda: m.align_cloud(line, guess), ref)
        assert pose.tobytes() == guess.tobytes()
        # fewer matches than min_matches
        ref = A.Alignment(ref_map, line[:5], guess, 0.05, None, 0.05)
        assert ref.status == A.NO_VALID_PIXELS and ref.n_matched == 5
        pose, res = check_alignment(m, lambda: m.align_cloud(line[:5], guess), ref)
        assert pose.tobytes() == guess.tobytes()
    # refused calls: -1, nothing launched
    m = world["dev"][0.05]
    H = m._handle()
    d = np.ascontiguousarray(frame["depth"])
    dt = 0 if d.dtype == np.uint16 else 1
    g, out, res = pose_to_cm(world["guess"]), np.full(16, 7, np.float32), _lib.MapAlignResult()

    def sphere(depth=d, dtype=dt, conv=2, guess=g, pose_out=out, **kw):
        p = m.align_params(**kw)
        return hip_lib.rgbd360_map_align_sphere(H, vp(depth), d.strides[0], dtype, d.shape[0], d.shape[1], conv, vp(guess), 0, C.byref(p), vp(pose_out), C.byref(res))

    nxt = float(np.nextafter(np.float32(0.05), np.float32(1)))
    assert sphere(max_dist=0.0) == -1 and sphere(max_dist=-1.0) == -1 and sphere(max_dist=nxt) == -1 and sphere(max_dist=float("nan")) == -1
    assert sphere(max_iters=-1) == -1 and sphere(min_count=0) == -1
    assert sphere(depth=None) == -1 and sphere(guess=None) == -1 and sphere(pose_out=None) == -1
    assert sphere(conv=3) == -1 and sphere(conv=-1) == -1 and sphere(dtype=2) == -1
    assert hip_lib.rgbd360_map_last_error(H) != b"" and (out == 7).all()
    p = m.align_params()
    assert hip_lib.rgbd360_map_align_cloud(H, None, 5, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == -1
    assert hip_lib.rgbd360_map_align_cloud(H, vp(d), -1, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == -1
    # empty inputs: NO_VALID_PIXELS, pose_out = guess
    assert hip_lib.rgbd360_map_align_cloud(H, None, 0, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == A.NO_VALID_PIXELS
    assert out.tobytes() == g.tobytes() and res.status == A.NO_VALID_PIXELS and res.n_matched == 0
    out[:] = 7
    assert hip_lib.rgbd360_map_align_sphere(H, vp(d), d.strides[0], dt, 0, d.shape[1], 2, vp(g), 0, None, vp(out), None) == A.NO_VALID_PIXELS
    assert out.tobytes() == g.tobytes()
    # and the map aligns afterwards (params NULL: the defaults)
    assert hip_lib.rgbd360_map_align_sphere(H, vp(d), d.strides[0], dt, d.shape[0], d.shape[1], 2, vp(g), 0, None, vp(out), C.byref(res)) == 0
    assert res.converged == 1 and res.n_matched > 15000


@pytest.mark.parametrize("leaf", [0.05, 0.2])
def test_real_panoramas(reg, leaf):
    """Frame 10 of the sample pair against a map of frame 1 (1920 x 320, convention 0, a fifth of the pixels without depth), two steps
    from the identity (the restatement of a ten-step alignment of 600 000 points takes a quarter of a minute)."""
    from rgbd360_amd.register import stitch_sphere
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import config1_samples as c1
    ext = np.stack(c1.load_extrinsics("fixture"))
    depths = []
    for k in (1, 10):
        fr = c1.frames(k, "fixture")
        depths.append(stitch_sphere(reg, np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), ext)[1])
    clouds = [reg.sphere_cloud(d, 0) for d in depths]
    ref = A.Alignment(R.Map([(clouds[0], None, EYE)], leaf), clouds[1], EYE, leaf, R.DEFAULT_BOX, leaf, max_iters=2)
    assert ref.iterations == 2 and ref.n_matched > 100000
    with new_map(reg, leaf, capacity=1 << 18) as m:
        m.insert_sphere(None, depths[0], EYE, convention=0)
        check_alignment(m, lambda: m.align_sphere(depths[1], EYE, convention=0, max_iters=2), ref)


def test_odometry_replay_refines_on_the_map(reg, tmp_path):
    """examples/odometry_replay.cpp --map F --refine-on-map: one "refine" line per frame with an accepted refinement against the map,
    the dense alignment's lines of the first pair untouched; without the option the output and the map file are what they are without
    it (twice the same)."""
    from tests.test_cpp_adapter import build_example
    exe = build_example(tmp_path)
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "3", "256", "128"])
    base = [exe, str(seq), "3", "256", "128", "--map"]
    plain = subprocess.run(base + [str(tmp_path / "a.txt"), "--leaf", "0.1"], text=True, capture_output=True, check=True)
    again = subprocess.run(base + [str(tmp_path / "b.txt"), "--leaf", "0.1"], text=True, capture_output=True, check=True)
    assert plain.stdout == again.stdout and "refine" not in plain.stdout and (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()
    refined = subprocess.run(base + [str(tmp_path / "c.txt"), "--leaf", "0.1", "--refine-on-map"], text=True, capture_output=True, check=True)
    lines = refined.stdout.splitlines()
    pairs, refines = [l for l in lines if l.startswith("pair")], [l.split() for l in lines if l.startswith("refine")]
    assert len(pairs) == 2 and len(refines) == 2 and pairs[0] == plain.stdout.splitlines()[0]
    for r in refines:
        assert r[2:4] == ["status", "0"] and int(r[7]) > 5000 and float(r[9]) < 0.1 ** 2
    rows = np.loadtxt(str(tmp_path / "c.txt")).reshape(-1, 7)
    assert len(rows) > 1000 and int(rows[:, 6].sum()) == int(np.loadtxt(str(tmp_path / "a.txt")).reshape(-1, 7)[:, 6].sum())


@pytest.mark.parametrize("form", ["f32_padded", "u16"])
def test_an_alignment_from_host_and_from_device_memory_is_the_same(reg, hip_lib, form):
    """The 1100 x 24 strip (map_input_forms.py: float32 depth with a padded row step, uint16 depth) aligned with on_device = 0 and 1: the
    same pose bits and the same result struct."""
    import map_input_forms as F
    from rgbd360_amd import _lib
    forms = F.Forms(reg)
    try:
        p = _lib.MapAlignParams()
        hip_lib.rgbd360_map_default_align_params(None, C.byref(p))
        p.max_dist = F.LEAF
        host, dev = F.align_on_both(hip_lib, reg, forms, form, hip_lib.rgbd360_map_align_sphere, p, _lib.MapAlignResult)
    finally:
        forms.close()
    assert host == dev
