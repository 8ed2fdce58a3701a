"""The point-to-plane alignment of a frame against the voxel map (rgbd360_map_align_plane_*, csrc/map_align_plane.h) on the device
against the numpy restatement of its definition (tests/map_align_plane_reference.py): per point the matched key and d2 bit for bit (and
equal to rgbd360_map_align_eval's), the class exact, the normal and r bit for bit in float64, exact counters, the 30 sums to the
project's bound for sums (2e-6 relative; H to 2e-5 max|H|), and the whole loop: status, iteration count, the contributing
points per iteration, and the pose to the device-mode bound (5e-6 rad, 5e-6 m).  The helpers repeat those of tests/test_map_align_gpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import map_align_plane_reference as PL
import map_align_reference as A
import voxel_map_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
SEED = 8          # of the perturbed guess (1 cm, 3 mrad): every stop / continue decision of the restated loops is a factor > 8 from eps at both leaves
POSE_TOL = 5e-6
LEAVES = (0.05, 0.1)
# tests/test_map_align_plane_cpu.py: the restatement's point-to-plane errors on the corner scene, the largest over seeds 1, 2, 3
MEASURED_PLANE_ERR = (7.85e-4, 2.52e-3)


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
    """The frame in maps of 0.05 m and 0.1 m at the general pose, on the device and restated; an alignment never changes a map."""
    P = R.general_pose()
    maps = {leaf: new_map(reg, leaf) for leaf in LEAVES}
    for m in maps.values():
        m.insert_sphere(None, frame["depth"], P, convention=2)
    yield dict(P=P, guess=A.perturbed(P, 0.01, 0.003, SEED), dev=maps, ref={leaf: R.Map([(frame["cloud"], None, P)], leaf) for leaf in maps})
    for m in maps.values():
        m.close()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


COUNTERS = ("n_valid", "n_box_rejected", "n_out_of_range", "n_unsupported", "n_nonplanar")


def device_eval(hip_lib, hip, m, pose, depth=None, convention=2, xyz=None, point_too=False, **params):
    """rgbd360_map_align_plane_eval: dict(key3, d2, normal_r, cls, sums, counters); point_too: rgbd360_map_align_eval's key3 and d2 of
    the same inputs are compared on the spot."""
    from rgbd360_amd.register import pose_to_cm
    n = depth.size if depth is not None else len(xyz)
    k = max(n, 1)
    host = dict(key3=np.zeros((k, 3), np.int32), d2=np.zeros(k, np.float32), normal_r=np.zeros((k, 4), np.float64), cls=np.full(k, 9, np.uint8))
    dev = {}
    for name, a in host.items():
        dev[name] = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev[name]), a.nbytes) == 0
    sums, counters = np.zeros(30, np.float64), np.zeros(5, np.int64)
    p = m.align_plane_params(**params)
    cm = pose_to_cm(pose)
    x = None if xyz is None else np.ascontiguousarray(xyz, np.float32)
    if depth is not None:
        src = (vp(depth), depth.strides[0], 0 if depth.dtype == np.uint16 else 1, depth.shape[0], depth.shape[1], convention, None, 0)
    else:
        src = (None, 0, 0, 0, 0, 0, vp(x), len(x))
    rc = hip_lib.rgbd360_map_align_plane_eval(m._handle(), *src, vp(cm), 0, C.byref(p), vp(sums), vp(counters), dev["key3"], dev["d2"], dev["normal_r"],
                                              dev["cls"])
    assert rc == 0, (rc, hip_lib.rgbd360_map_last_error(m._handle()))
    for name, a in host.items():
        assert hip.hipMemcpy(vp(a), dev[name], a.nbytes, 2) == 0
    out = {name: a[:n] for name, a in host.items()}
    if point_too:
        key, d2 = np.zeros((k, 3), np.int32), np.zeros(k, np.float32)
        pp = m.align_params(**{f: v for f, v in params.items() if f not in ("min_support", "max_flatness")})
        s17, c3 = np.zeros(17, np.float64), np.zeros(3, np.int64)
        rc = hip_lib.rgbd360_map_align_eval(m._handle(), *src, vp(cm), 0, C.byref(pp), vp(s17), vp(c3), dev["key3"], dev["d2"], 0, None, None)
        assert rc == 0 and hip.hipMemcpy(vp(key), dev["key3"], key.nbytes, 2) == 0 and hip.hipMemcpy(vp(d2), dev["d2"], d2.nbytes, 2) == 0
        assert np.array_equal(key[:n], out["key3"]) and d2[:n].tobytes() == out["d2"].tobytes()
        assert c3.tolist() == counters[:3].tolist()
    for d in dev.values():
        hip.hipFree(d)
    out.update(sums=sums, counters=dict(zip(COUNTERS, counters.tolist())))
    return out


def check_eval(got, ref, what=""):
    assert np.array_equal(got["key3"], ref.key3), what
    assert got["d2"].tobytes() == ref.d2.tobytes(), what
    assert np.array_equal(got["cls"], ref.cls), (what, np.bincount(got["cls"], minlength=4), np.bincount(ref.cls, minlength=4))
    assert got["counters"] == ref.counters, what
    assert got["sums"][0] == ref.n, what
    differ = np.nonzero((got["normal_r"] != ref.normal_r).any(axis=1))[0]
    assert got["normal_r"].tobytes() == ref.normal_r.tobytes(), (what, len(differ), got["normal_r"][differ[:3]], ref.normal_r[differ[:3]])
    scale = np.maximum(np.abs(ref.sums), 1e-300)
    print(what, "contributing", ref.n, ref.counters, "largest relative difference of a sum", np.max(np.abs(got["sums"] - ref.sums) / scale))
    assert np.all(np.abs(got["sums"] - ref.sums) <= 2e-6 * np.abs(ref.sums) + 1e-9), (what, got["sums"], ref.sums)


def check_normal_equations(H, g, ref_H, ref_g):
    assert np.abs(H - ref_H).max() <= 2e-5 * np.abs(ref_H).max()
    assert np.abs(g - ref_g).max() <= 2e-5 * max(np.abs(ref_g).max(), 1e-30) + 2e-6 * np.abs(ref_H).max() * 1e-3


def restated(world, leaf, xyz, pose, box=R.DEFAULT_BOX, **kw):
    return PL.PlaneEvaluation(world["ref"][leaf], xyz, pose, leaf, box, kw.pop("max_dist", leaf), **kw)


@pytest.mark.parametrize("at", ["map_pose", "perturbed"])
@pytest.mark.parametrize("leaf", LEAVES)
def test_evaluation_equals_the_restatement_and_the_cloud_route(hip_lib, hip, frame, world, leaf, at):
    pose = world["P"] if at == "map_pose" else world["guess"]
    ref = restated(world, leaf, frame["cloud"], pose)
    assert ref.n > 1000 and ref.counters["n_box_rejected"] > 0 and ref.counters["n_unsupported"] > 0
    assert leaf == 0.05 or ref.counters["n_nonplanar"] > 0       # (at 0.05 m the 256-column frame's samples are too sparse for a corner's support)
    a = device_eval(hip_lib, hip, world["dev"][leaf], pose, depth=frame["depth"], point_too=True)
    check_eval(a, ref, "sphere")
    b = device_eval(hip_lib, hip, world["dev"][leaf], pose, xyz=frame["cloud"], point_too=True)
    check_eval(b, ref, "cloud")
    # the same row from both routes: the same points and bits per point, another tiling (a workgroup per image row / per 1024 points),
    # so the float64 sums agree to the bound above, not to the last bit
    assert a["sums"][0] == b["sums"][0] and a["counters"] == b["counters"] and a["normal_r"].tobytes() == b["normal_r"].tobytes()
    assert np.all(np.abs(a["sums"] - b["sums"]) <= 2e-6 * np.abs(ref.sums) + 1e-9)


@pytest.mark.parametrize("n", [1, 1023, 1025, 2 * 1024 + 37])
def test_ragged_cloud_sizes(hip_lib, hip, frame, world, n):
    """One lane, a ragged tile, several workgroups with a tail."""
    valid = np.nonzero(np.isfinite(frame["cloud"]).all(axis=1))[0]
    xyz = frame["cloud"][valid[np.linspace(0, len(valid) - 1, n).astype(np.int64)]]
    ref = restated(world, 0.1, xyz, world["guess"])
    assert n == 1 or ref.n > 100
    check_eval(device_eval(hip_lib, hip, world["dev"][0.1], world["guess"], xyz=xyz), ref)


@pytest.mark.parametrize("depth_type", ["u16", "f32"])
def test_ragged_strided_image(hip_lib, hip, reg, frame, world, depth_type):
    """250 x 9 (no multiple of the tile) as a view of a wider array, both depth types."""
    d = frame["depth"]
    metres = d.astype(np.float32) * np.float32(0.001) if d.dtype == np.uint16 else d
    wide = np.round(metres * 1000).astype(np.uint16) if depth_type == "u16" else metres.astype(np.float32)
    depth = wide[60:69, 3:253]
    assert depth.shape == (9, 250) and depth.strides[0] > 250 * depth.itemsize
    cloud = reg.sphere_cloud(np.ascontiguousarray(depth), 2)
    with new_map(reg, 0.1) as m:
        m.insert_cloud(cloud, None, world["P"])
        ref = PL.PlaneEvaluation(R.Map([(cloud, None, world["P"])], 0.1), cloud, world["guess"], 0.1, R.DEFAULT_BOX, 0.1, min_support=3)
        assert ref.n > 100
        check_eval(device_eval(hip_lib, hip, m, world["guess"], depth=depth, min_support=3), ref)


def test_a_strip_of_two_tiles_per_row(hip_lib, hip, reg, world):
    """1100 x 24: a full tile and a ragged second one of 76 columns per row, the smallest shape in which all four point slots of a thread
    and the second blockIdx.x of the sphere route hold pixels (at 256 and 250 columns only the first slot ever does)."""
    from rgbd360_amd import synth
    depth = synth.render(synth.trajectory_pose(0, 7), 1100, 24, 7)[1]
    cloud = reg.sphere_cloud(depth, 2)
    with new_map(reg, 0.1) as m:
        m.insert_sphere(None, depth, world["P"], convention=2)
        ref = PL.PlaneEvaluation(R.Map([(cloud, None, world["P"])], 0.1), cloud, world["guess"], 0.1, R.DEFAULT_BOX, 0.1)
        assert ref.n > 1000
        check_eval(device_eval(hip_lib, hip, m, world["guess"], depth=depth, point_too=True), ref)


@pytest.mark.parametrize("convention", [0, 1])
def test_the_other_conventions(hip_lib, hip, reg, frame, convention):
    cloud = reg.sphere_cloud(frame["depth"], convention)
    with new_map(reg, 0.1) as m:
        m.insert_cloud(cloud, None, EYE)
        shifted = EYE.copy()
        shifted[:3, 3] = [0.004, -0.003, 0.002]
        ref = PL.PlaneEvaluation(R.Map([(cloud, None, EYE)], 0.1), cloud, shifted, 0.1, R.DEFAULT_BOX, 0.1)
        assert ref.n > 1000
        check_eval(device_eval(hip_lib, hip, m, shifted, depth=frame["depth"], convention=convention), ref)


CASES = R.edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_edge_values_on_the_device(hip_lib, hip, reg, case):
    """The map's edge values (NaN, +-Inf, the box limits, |w| at 4096: a neighbour index at the edge of the 21-bit key range) and negative
    voxel indices: the case's cloud against its own map, at the case's pose and a hair beside it; min_support 1 so that every kept match
    reaches the plane function, whatever its support."""
    name, xyz, rgb, pose, leaf, box = case
    ref_map = R.Map([(xyz, rgb, pose)], leaf, box)
    beside = np.array(pose, np.float32)
    beside[:3, 3] += np.float32(0.3 * leaf) * np.array([1, -1, 1], np.float32)
    with new_map(reg, leaf=leaf, capacity=256, box=box) as m:
        m.insert_cloud(xyz, rgb, pose)
        for T in (pose, beside):
            for min_support in (1, 5):
                ref = PL.PlaneEvaluation(ref_map, xyz, T, leaf, box, leaf, min_support=min_support)
                check_eval(device_eval(hip_lib, hip, m, T, xyz=xyz, min_support=min_support), ref, name)


def test_the_edge_of_the_key_range(hip_lib, hip, reg):
    """The smallest leaf, 0.004, and |w| just below 4096: the largest voxel indices a map can hold, 1023999 and -1024000 (the bias of
    2^20 leaves the 21-bit fields room for their neighbours, which are looked up like any other and not found).  A small wall at either
    end."""
    rng = np.random.default_rng(3)
    leaf = 0.004
    top = np.float32(4096.0) - np.float32(0.0005)
    wall = np.c_[np.full(400, top), rng.uniform(0, 0.03, 400), rng.uniform(0, 0.03, 400)].astype(np.float32)
    xyz = np.concatenate([wall, -wall])
    ref_map = R.Map([(xyz, None, EYE)], leaf, None)
    assert ref_map.key.max() == 1023999 and ref_map.key.min() == -1024000
    with new_map(reg, leaf=leaf, capacity=4096, box=None) as m:
        m.insert_cloud(xyz, None, EYE)
        for min_support in (1, 5):
            ref = PL.PlaneEvaluation(ref_map, xyz, EYE, leaf, None, leaf, min_support=min_support)
            assert ref.counters["n_out_of_range"] == 0 and (ref.cls != PL.NONE).sum() == 800
            check_eval(device_eval(hip_lib, hip, m, EYE, xyz=xyz, min_support=min_support, point_too=True), ref)


@pytest.mark.parametrize("params", [dict(min_support=27), dict(min_support=1), dict(max_flatness=0.0), dict(max_flatness=0.5, min_count=2)],
                         ids=["support27", "support1", "flatness0", "flatness05_count2"])
def test_support_and_flatness_settings(hip_lib, hip, frame, world, params):
    ref = restated(world, 0.1, frame["cloud"], world["guess"], **params)
    searched = (ref.cls != PL.NONE).sum()
    if params.get("min_support") == 27:
        assert ref.counters["n_unsupported"] > 0.9 * searched
    if params.get("min_support") == 1:
        assert ref.counters["n_unsupported"] == 0
    if params.get("max_flatness") == 0.0:
        assert ref.counters["n_nonplanar"] > 0.9 * searched
    check_eval(device_eval(hip_lib, hip, world["dev"][0.1], world["guess"], depth=frame["depth"], point_too=True, **params), ref, str(params))


def test_lookups_in_a_nearly_full_table(hip_lib, hip, reg):
    """900 voxels in 1024 slots (long probe chains, neighbours found late), then a table of 64 slots full to the last."""
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
            ref = PL.PlaneEvaluation(ref_map, xyz, T, 0.05, None, 0.05, min_support=2)
            assert (ref.cls != PL.NONE).sum() > 2000
            check_eval(device_eval(hip_lib, hip, m, T, xyz=xyz, min_support=2, point_too=True), ref)
    xyz2, _ = scattered_cloud(64, 200, seed=3)
    ref_map = R.Map([(xyz2, None, EYE)], 0.05, None)
    with new_map(reg, capacity=64, box=None) as m:
        m.insert_cloud(xyz2, None, EYE)
        assert len(m) == 64 and not m.full
        check_eval(device_eval(hip_lib, hip, m, shifted, xyz=xyz2, min_support=1), PL.PlaneEvaluation(ref_map, xyz2, shifted, 0.05, None, 0.05, min_support=1))


def test_an_empty_map(hip_lib, hip, reg, frame, world):
    with new_map(reg) as m:
        ref = PL.PlaneEvaluation(R.Map([], 0.05), frame["cloud"], world["guess"], 0.05, R.DEFAULT_BOX, 0.05)
        assert ref.n == 0 and ref.counters["n_valid"] > 0
        check_eval(device_eval(hip_lib, hip, m, world["guess"], depth=frame["depth"]), ref)
        pose, res = m.align_sphere_plane(frame["depth"], world["guess"], convention=2)
        assert res["status"] == A.NO_VALID_PIXELS and res["iterations"] == 0 and res["n_matched"] == 0 and res["fitness"] == 0.0 and res["fitness_point"] == 0.0
        assert pose.tobytes() == world["guess"].tobytes() and res["n_valid"] == ref.counters["n_valid"] and len(m) == 0


def check_alignment(m, run, ref, P=None):
    pose, res = run()
    trace = m.align_trace()
    print("status", res["status"], "iterations", res["iterations"], "converged", res["converged"], "contributing", [t[0] for t in trace], "restated",
          [t[0] for t in ref.trace], "margins", ref.margins, "pose difference", A.pose_error(pose, ref.pose))
    assert (res["status"], res["iterations"], res["converged"]) == (ref.status, ref.iterations, ref.converged)
    assert [t[0] for t in trace] == [t[0] for t in ref.trace]
    assert all(mg >= 2.0 for mg in ref.margins)
    for (n, ss, u), (rn, rss, ru) in zip(trace, ref.trace):
        assert abs(ss - rss) <= 2e-6 * rss + 1e-12 and np.abs(u - ru).max() <= POSE_TOL
    dr, dt = A.pose_error(pose, ref.pose)
    assert dr <= POSE_TOL and dt <= POSE_TOL
    assert res["n_matched"] == ref.n_matched and abs(res["fitness"] - ref.fitness) <= 2e-6 * ref.fitness + 1e-15
    assert abs(res["fitness_point"] - ref.fitness_point) <= 2e-6 * ref.fitness_point + 1e-15
    for k in COUNTERS:
        assert res[k] == ref.final.counters[k], k
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


@pytest.fixture(scope="module")
def loops(frame, world):
    """The restated loop per leaf, shared by the routes."""
    return {leaf: PL.PlaneAlignment(world["ref"][leaf], frame["cloud"], world["guess"], leaf, R.DEFAULT_BOX, leaf) for leaf in LEAVES}


@pytest.mark.parametrize("route", ["sphere", "cloud"])
@pytest.mark.parametrize("leaf", LEAVES)
def test_the_whole_loop(frame, world, loops, leaf, route):
    m, ref = world["dev"][leaf], loops[leaf]
    assert ref.status == A.OK and ref.iterations >= 2
    run = ((lambda: m.align_sphere_plane(frame["depth"], world["guess"], convention=2)) if route == "sphere"
           else (lambda: m.align_cloud_plane(frame["cloud"], world["guess"])))
    pose, res = check_alignment(m, run, ref, world["P"])
    r0, t0 = A.pose_error(world["guess"], world["P"])
    r1, t1 = A.pose_error(pose, world["P"])
    assert r1 <= 0.5 * r0 and t1 <= 0.5 * t0


def test_the_iteration_limit(frame, world):
    m = world["dev"][0.1]
    ref = PL.PlaneAlignment(world["ref"][0.1], frame["cloud"], world["guess"], 0.1, R.DEFAULT_BOX, 0.1, max_iters=1)
    assert ref.iterations == 1 and ref.converged == 0 and ref.status == A.OK
    check_alignment(m, lambda: m.align_sphere_plane(frame["depth"], world["guess"], convention=2, max_iters=1), ref)
    ref0 = PL.PlaneAlignment(world["ref"][0.1], frame["cloud"], world["guess"], 0.1, R.DEFAULT_BOX, 0.1, max_iters=0)
    pose, res = check_alignment(m, lambda: m.align_sphere_plane(frame["depth"], world["guess"], convention=2, max_iters=0), ref0)
    assert pose.tobytes() == world["guess"].tobytes() and res["iterations"] == 0 and res["n_matched"] > 1000 and m.align_trace() == []


def test_the_table_is_read_only_and_point_to_point_is_unchanged(reg, frame, world):
    P = world["P"]
    with new_map(reg, 0.1) as m:
        m.insert_sphere(frame["rgb"], frame["depth"], P, convention=2)
        before = m.extract()
        point_before = m.align_sphere(frame["depth"], world["guess"], convention=2)
        m.align_sphere_plane(frame["depth"], world["guess"], convention=2)
        m.align_cloud_plane(frame["cloud"], world["guess"], min_count=2, min_support=3)
        after = m.extract()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        # a point-to-point alignment behind a point-to-plane one (which left a wider row and a larger state in the shared buffers)
        point_after = m.align_sphere(frame["depth"], world["guess"], convention=2)
        assert point_after[0].tobytes() == point_before[0].tobytes()
        assert all(np.array_equal(np.asarray(point_before[1][k]), np.asarray(point_after[1][k])) for k in point_before[1])


def test_degenerate_inputs(hip_lib, reg, frame, world):
    from rgbd360_amd import _lib
    from rgbd360_amd.register import pose_to_cm
    # a single wall: the translation in it and the rotation about its normal are not observable
    wall = PL.corner_scene(5)[:40000:4]
    ref_map = R.Map([(wall, None, EYE)], 0.05, None)
    with new_map(reg, box=None) as m:
        m.insert_cloud(wall, None, EYE)
        guess = EYE.copy()
        guess[0, 3] = 0.01
        ref = PL.PlaneAlignment(ref_map, wall, guess, 0.05, None, 0.05)
        assert ref.status == A.ILL_POSED and ref.iterations == 0 and ref.n_matched > 5000
        pose, res = check_alignment(m, lambda: m.align_cloud_plane(wall, guess), ref)
        assert pose.tobytes() == guess.tobytes()
        # fewer contributing points than min_matches
        ref = PL.PlaneAlignment(ref_map, wall[:5], guess, 0.05, None, 0.05)
        assert ref.status == A.NO_VALID_PIXELS and 0 < ref.n_matched < 6
        pose, res = check_alignment(m, lambda: m.align_cloud_plane(wall[:5], guess), ref)
        assert pose.tobytes() == guess.tobytes()
    # refused calls: -1, nothing launched
    m = world["dev"][0.05]
    H = m._handle()
    d = np.ascontiguousarray(frame["depth"])
    dt = 0 if d.dtype == np.uint16 else 1
    g, out, res = pose_to_cm(world["guess"]), np.full(16, 7, np.float32), _lib.MapAlignPlaneResult()

    def sphere(depth=d, dtype=dt, conv=2, guess=g, pose_out=out, **kw):
        p = m.align_plane_params(**kw)
        return hip_lib.rgbd360_map_align_plane_sphere(H, vp(depth), d.strides[0], dtype, d.shape[0], d.shape[1], conv, vp(guess), 0, C.byref(p), vp(pose_out),
                                                      C.byref(res))

    nxt = float(np.nextafter(np.float32(0.05), np.float32(1)))
    assert sphere(max_dist=0.0) == -1 and sphere(max_dist=-1.0) == -1 and sphere(max_dist=nxt) == -1 and sphere(max_dist=float("nan")) == -1
    assert sphere(max_iters=-1) == -1 and sphere(min_count=0) == -1
    assert sphere(min_support=0) == -1 and sphere(min_support=28) == -1 and sphere(max_flatness=-0.01) == -1 and sphere(max_flatness=float("nan")) == -1
    assert sphere(depth=None) == -1 and sphere(guess=None) == -1 and sphere(pose_out=None) == -1
    assert sphere(conv=3) == -1 and sphere(conv=-1) == -1 and sphere(dtype=2) == -1
    assert hip_lib.rgbd360_map_last_error(H) != b"" and (out == 7).all()
    p = m.align_plane_params()
    assert hip_lib.rgbd360_map_align_plane_cloud(H, None, 5, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == -1
    assert hip_lib.rgbd360_map_align_plane_cloud(H, vp(d), -1, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == -1
    assert hip_lib.rgbd360_map_align_plane_eval(H, None, 0, 0, 0, 0, 0, vp(d), 5, None, 0, C.byref(p), None, None, None, None, None, None) == -1
    # empty inputs: NO_VALID_PIXELS, pose_out = guess
    assert hip_lib.rgbd360_map_align_plane_cloud(H, None, 0, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == A.NO_VALID_PIXELS
    assert out.tobytes() == g.tobytes() and res.status == A.NO_VALID_PIXELS and res.n_matched == 0
    out[:] = 7
    assert hip_lib.rgbd360_map_align_plane_sphere(H, vp(d), d.strides[0], dt, 0, d.shape[1], 2, vp(g), 0, None, vp(out), None) == A.NO_VALID_PIXELS
    assert out.tobytes() == g.tobytes()
    # and the map aligns afterwards (params NULL: the defaults)
    assert hip_lib.rgbd360_map_align_plane_sphere(H, vp(d), d.strides[0], dt, d.shape[0], d.shape[1], 2, vp(g), 0, None, vp(out), C.byref(res)) == 0
    assert res.n_matched > 1000 and res.n_unsupported > 0


CORNER_SEEDS = (1, 2, 3)


@pytest.mark.parametrize("seed", CORNER_SEEDS)
def test_the_room_corner_on_the_device(reg, seed):
    """tests/test_map_align_plane_cpu.py's scene: point-to-plane ends closer to the true pose than point-to-point, in rotation and in
    translation, and below 4 x the largest error the restatement measured; seed 1 also against the restated loop itself (one seed: the
    restatement of a ten-step alignment of 120 000 points takes ten seconds)."""
    P = R.general_pose()
    target, src = PL.corner_scene(100 + seed), PL.corner_scene(200 + seed, P)
    guess = A.perturbed(P, 0.02, np.radians(0.5), seed)
    with new_map(reg, box=None) as m:
        m.insert_cloud(target, None, EYE)
        point, pres = m.align_cloud(src, guess)
        plane, lres = m.align_cloud_plane(src, guess)
        (rp, tp), (rl, tl) = A.pose_error(point, P), A.pose_error(plane, P)
        print("seed", seed, "point-to-point", (rp, tp), pres["iterations"], "point-to-plane", (rl, tl), lres["iterations"], "contributing", lres["n_matched"],
              "nonplanar", lres["n_nonplanar"], "unsupported", lres["n_unsupported"], "fitness", lres["fitness"], lres["fitness_point"], pres["fitness"])
        assert pres["status"] == A.OK and lres["status"] == A.OK
        assert rl <= rp and tl <= tp
        assert rl <= 4 * MEASURED_PLANE_ERR[0] and tl <= 4 * MEASURED_PLANE_ERR[1]
        assert lres["n_nonplanar"] > 0 and lres["n_matched"] > 100000
        if seed == CORNER_SEEDS[0]:
            ref = PL.PlaneAlignment(R.Map([(target, None, EYE)], 0.05, None), src, guess, 0.05, None, 0.05)
            check_alignment(m, lambda: m.align_cloud_plane(src, guess), ref, P)


def test_real_panoramas(reg):
    """Frame 10 of the sample pair against a map of frame 1 at the oracle's pose for it, the identity (1920 x 320, convention 0, a
    fifth of the pixels without depth), two steps (the restatement of more steps over 600 000 points takes too long for a test)."""
    from rgbd360_amd.register import stitch_sphere
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import config1_samples as c1
    ext = np.stack(c1.load_extrinsics("fixture"))
    depths = []
    for k in (1, 10):
        fr = c1.frames(k, "fixture")
        depths.append(stitch_sphere(reg, np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), ext)[1])
    clouds = [reg.sphere_cloud(d, 0) for d in depths]
    leaf = 0.05
    ref = PL.PlaneAlignment(R.Map([(clouds[0], None, EYE)], leaf), clouds[1], EYE, leaf, R.DEFAULT_BOX, leaf, max_iters=2)
    assert ref.status == A.OK and ref.iterations == 2 and ref.n_matched > 50000
    with new_map(reg, leaf, capacity=1 << 18) as m:
        m.insert_sphere(None, depths[0], EYE, convention=0)
        pose, res = check_alignment(m, lambda: m.align_sphere_plane(depths[1], EYE, convention=0, max_iters=2), ref)
        assert res["status"] == A.OK and res["n_matched"] > 0


def test_odometry_replay_refines_on_the_map_by_planes(reg, tmp_path):
    """examples/odometry_replay.cpp --map F --refine-on-map-plane: one "refine-plane" line per frame; without the option the output is
    what it is without it, and --refine-on-map prints what it printed."""
    from tests.test_cpp_adapter import build_example
    exe = build_example(tmp_path)
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "3", "256", "128"])
    base = [exe, str(seq), "3", "256", "128", "--map"]
    plain = subprocess.run(base + [str(tmp_path / "a.txt"), "--leaf", "0.1"], text=True, capture_output=True, check=True)
    assert "refine" not in plain.stdout and len(plain.stdout.splitlines()) == 2
    point = subprocess.run(base + [str(tmp_path / "b.txt"), "--leaf", "0.1", "--refine-on-map"], text=True, capture_output=True, check=True)
    assert "refine-plane" not in point.stdout and sum(l.startswith("refine ") for l in point.stdout.splitlines()) == 2
    refined = subprocess.run(base + [str(tmp_path / "c.txt"), "--leaf", "0.1", "--refine-on-map-plane"], text=True, capture_output=True, check=True)
    lines = refined.stdout.splitlines()
    pairs, refines = [l for l in lines if l.startswith("pair")], [l.split() for l in lines if l.startswith("refine-plane")]
    assert len(pairs) == 2 and len(refines) == 2 and pairs[0] == plain.stdout.splitlines()[0] and not any(l.startswith("refine ") for l in lines)
    for r in refines:
        assert r[2:4] == ["status", "0"] and int(r[7]) > 1000 and float(r[9]) < 0.1 ** 2
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
        p = _lib.MapAlignPlaneParams()
        hip_lib.rgbd360_map_default_align_plane_params(None, C.byref(p))
        p.max_dist = F.LEAF
        host, dev = F.align_on_both(hip_lib, reg, forms, form, hip_lib.rgbd360_map_align_plane_sphere, p, _lib.MapAlignPlaneResult)
    finally:
        forms.close()
    assert host == dev
