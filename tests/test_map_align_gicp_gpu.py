"""Generalized ICP against the voxel map (rgbd360_map_align_gicp_*, csrc/map_align_gicp.h) on the device against the numpy restatement
of its definition (tests/map_align_gicp_reference.py): per point the matched key and d2 bit for bit (and equal to
rgbd360_map_align_eval's), the class byte exact, the weight M and the cost bit for bit in float64, exact counters, the 30 sums to the
project's bound for sums (2e-6 relative; H to 2e-5 max|H|), and the whole loop: status, iteration count, the matches per
iteration, and the pose to the device-mode bound (5e-6 rad, 5e-6 m).  The fixtures and helpers repeat those of
tests/test_map_align_plane_gpu.py.

The bound on the sums with weights of 1 / epsilon = 1000 in them: the restated rows of the four evaluations of the first test below were
summed in three orders on the CPU (numpy's pairwise sum, a running sum forwards and one backwards); the largest difference of a sum
between two orders was 3.9e-8 of the project's bound 2e-6 |sum| + 1e-9 for that sum.  The bound does not bind and stays as it is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_align_gicp_reference as GI
import map_align_reference as A
import map_normals_reference as N
import voxel_map_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EYE = np.eye(4, dtype=np.float32)
# Of the perturbed guess (1 cm, 3 mrad).  Every stop / continue decision of the restated loops below lies a factor of more than 8 from
# eps: measured on the CPU over seeds 1 .. 12, seed 5 has the factors 98 (frame, no source normals) and 99 (frame, per-point normals) at
# 0.05 m, 99.6 and 99.7 at 0.1 m, and 96 for the map of frame b as the source at 0.1 m.
SEED = 5
# ... and of the guess of the point-to-point limit, where the loop compared with is the device's own point method (the restated point
# loop's factors: 8.2 at 0.05 m with seed 6, 2.4 at 0.1 m with seed 4, the largest of the twelve seeds at either leaf)
LIMIT_SEED = {0.05: 6, 0.1: 4}
POSE_TOL = 5e-6
LEAVES = (0.05, 0.1)
COUNTERS = GI.COUNTERS


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


def point_normals(cloud, leaf):
    """A normal per point of a frame's cloud: that of the voxel the point feeds in the restated map of the cloud alone at the identity
    (zero where the voxel has none, and for the points the map's box or the range test drops)."""
    ref = R.Map([(cloud, None, EYE)], leaf)
    layer = N.layer(ref)
    w, idx, _ = R.passing(cloud, EYE, R.DEFAULT_BOX)
    row = np.searchsorted(A.packed_keys(ref.key), A.packed_keys(R.voxel_index(w, leaf)))
    out = np.zeros((len(cloud), 3), np.float32)
    out[idx] = layer["normal"][row]
    return out


@pytest.fixture(scope="module")
def frame(reg, small_pair):
    (rgb, depth), (_, depth_b), t_rel = small_pair
    cloud = reg.sphere_cloud(depth, 2)
    return dict(rgb=rgb, depth=depth, cloud=cloud, normals={leaf: point_normals(cloud, leaf) for leaf in LEAVES}, depth_b=depth_b,
                cloud_b=reg.sphere_cloud(depth_b, 2), t_rel=t_rel)


@pytest.fixture(scope="module")
def world(reg, frame):
    """The frame in maps of 0.05 m and 0.1 m at the general pose, on the device and restated; an alignment never changes a map."""
    P = R.general_pose()
    maps = {leaf: new_map(reg, leaf) for leaf in LEAVES}
    for m in maps.values():
        m.insert_sphere(None, frame["depth"], P, convention=2)
    ref = {leaf: R.Map([(frame["cloud"], None, P)], leaf) for leaf in maps}
    yield dict(P=P, guess=A.perturbed(P, 0.01, 0.003, SEED), dev=maps, ref=ref, layers={leaf: GI.Layers(ref[leaf]) for leaf in maps},
               P_b=(np.asarray(P, np.float64) @ frame["t_rel"]).astype(np.float32))
    for m in maps.values():
        m.close()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_eval(hip_lib, hip, m, pose, depth=None, convention=2, xyz=None, normals=None, point_too=False, **params):
    """rgbd360_map_align_gicp_eval: dict(key3, d2, weight_cost, cls, sums, counters); point_too: rgbd360_map_align_eval's key3 and d2 of
    the same inputs are compared on the spot."""
    from rgbd360_amd.register import pose_to_cm
    n = depth.size if depth is not None else len(xyz)
    k = max(n, 1)
    host = dict(key3=np.zeros((k, 3), np.int32), d2=np.zeros(k, np.float32), weight_cost=np.full((k, 7), 9.0, np.float64), cls=np.full(k, 99, np.uint8))
    dev = {}
    for name, a in host.items():
        dev[name] = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev[name]), a.nbytes) == 0
    sums, counters = np.zeros(30, np.float64), np.zeros(6, np.int64)
    p = m.align_gicp_params(**params)
    cm = pose_to_cm(pose)
    x = None if xyz is None else np.ascontiguousarray(xyz, np.float32)
    nr = None if normals is None else np.ascontiguousarray(normals, np.float32)
    if depth is not None:
        src = (vp(depth), depth.strides[0], 0 if depth.dtype == np.uint16 else 1, depth.shape[0], depth.shape[1], convention, None, None, 0)
    else:
        assert nr is None or nr.shape == x.shape
        src = (None, 0, 0, 0, 0, 0, vp(x), vp(nr), len(x))
    rc = hip_lib.rgbd360_map_align_gicp_eval(m._handle(), *src, vp(cm), 0, C.byref(p), vp(sums), vp(counters), dev["key3"], dev["d2"], dev["weight_cost"],
                                             dev["cls"])
    assert rc == 0, (rc, hip_lib.rgbd360_map_last_error(m._handle()))
    for name, a in host.items():
        assert hip.hipMemcpy(vp(a), dev[name], a.nbytes, 2) == 0
    out = {name: a[:n] for name, a in host.items()}
    if point_too:
        key, d2 = np.zeros((k, 3), np.int32), np.zeros(k, np.float32)
        pp = m.align_params(**{f: v for f, v in params.items() if f in ("max_dist", "max_iters", "eps", "min_count", "min_matches")})
        s17, c3 = np.zeros(17, np.float64), np.zeros(3, np.int64)
        rc = hip_lib.rgbd360_map_align_eval(m._handle(), *src[:7], src[8], vp(cm), 0, C.byref(pp), vp(s17), vp(c3), dev["key3"], dev["d2"], 0, None, None)
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
    assert np.array_equal(got["cls"], ref.cls), (what, np.bincount(got["cls"], minlength=8), np.bincount(ref.cls, minlength=8))
    assert got["counters"] == ref.counters, (what, got["counters"], ref.counters)
    assert got["sums"][0] == ref.n, what
    differ = np.nonzero((got["weight_cost"] != ref.weight_cost).any(axis=1))[0]
    assert got["weight_cost"].tobytes() == ref.weight_cost.tobytes(), (what, len(differ), got["weight_cost"][differ[:3]], ref.weight_cost[differ[:3]])
    scale = np.maximum(np.abs(ref.sums), 1e-300)
    print(what, "kept", ref.n, ref.counters, "largest relative difference of a sum", np.max(np.abs(got["sums"] - ref.sums) / scale))
    assert np.all(np.abs(got["sums"] - ref.sums) <= 2e-6 * np.abs(ref.sums) + 1e-9), (what, got["sums"], ref.sums)


def check_normal_equations(H, g, ref_H, ref_g):
    assert np.abs(H - ref_H).max() <= 2e-5 * np.abs(ref_H).max()
    assert np.abs(g - ref_g).max() <= 2e-5 * max(np.abs(ref_g).max(), 1e-30) + 2e-6 * np.abs(ref_H).max() * 1e-3


def restated(world, leaf, xyz, pose, normals=None, box=R.DEFAULT_BOX, **kw):
    return GI.GicpEvaluation(world["ref"][leaf], xyz, pose, leaf, box, kw.pop("max_dist", leaf), normals=normals, layers=world["layers"][leaf], **kw)


@pytest.mark.parametrize("at", ["map_pose", "perturbed"])
@pytest.mark.parametrize("leaf", LEAVES)
def test_evaluation_equals_the_restatement_and_the_cloud_route(hip_lib, hip, frame, world, leaf, at):
    pose = world["P"] if at == "map_pose" else world["guess"]
    m = world["dev"][leaf]
    ref = restated(world, leaf, frame["cloud"], pose)
    c = ref.counters
    assert ref.n > 1000 and c["n_box_rejected"] > 0 and 0 < c["n_target_planes"] < ref.n and c["n_source_planes"] == 0
    a = device_eval(hip_lib, hip, m, pose, depth=frame["depth"], point_too=True)
    check_eval(a, ref, "sphere")
    b = device_eval(hip_lib, hip, m, pose, xyz=frame["cloud"], point_too=True)
    check_eval(b, ref, "cloud")
    # the same row from both routes: the same points and bytes per point, another tiling (a workgroup per image row / per 1024 points),
    # so the float64 sums agree to the bound above, not to the last bit
    assert a["sums"][0] == b["sums"][0] and a["counters"] == b["counters"]
    assert a["weight_cost"].tobytes() == b["weight_cost"].tobytes() and a["cls"].tobytes() == b["cls"].tobytes()
    assert np.all(np.abs(a["sums"] - b["sums"]) <= 2e-6 * np.abs(ref.sums) + 1e-9)
    # with a normal per source point: plane pairs, target planes alone, source planes alone and plain points in one evaluation
    nrm = frame["normals"][leaf]
    ref2 = restated(world, leaf, frame["cloud"], pose, normals=nrm)
    c = ref2.counters
    assert c["n_plane_pairs"] > 0 and c["n_target_planes"] > c["n_plane_pairs"] and c["n_source_planes"] > c["n_plane_pairs"]
    assert set(np.unique(ref2.cls)) == {0, 1, 3, 5, 7}
    check_eval(device_eval(hip_lib, hip, m, pose, xyz=frame["cloud"], normals=nrm, point_too=True), ref2, "cloud with normals")


def test_source_normals(hip_lib, hip, frame, world):
    """The voxels of a map of frame b as the source: with the map's own normals, without any, and with some normals struck out (zero,
    NaN, infinite): the class bits and the counters follow."""
    leaf = 0.1
    m = world["dev"][leaf]
    sx, sn = GI.map_source(R.Map([(frame["cloud_b"], None, EYE)], leaf))
    assert len(sx) > 5000 and 0 < (sn != 0).any(axis=1).sum() < len(sx)
    pose = A.perturbed(world["P_b"], 0.01, 0.003, SEED)
    with_normals = restated(world, leaf, sx, pose, normals=sn)
    check_eval(device_eval(hip_lib, hip, m, pose, xyz=sx, normals=sn), with_normals, "own normals")
    without = restated(world, leaf, sx, pose)
    assert without.counters["n_source_planes"] == 0 and with_normals.counters["n_source_planes"] > 1000
    check_eval(device_eval(hip_lib, hip, m, pose, xyz=sx), without, "no normals")
    struck = sn.copy()
    has = np.nonzero((with_normals.cls & GI.SOURCE) != 0)[0]
    struck[has[0::4]] = 0.0
    struck[has[1::4], 1] = np.nan
    struck[has[2::4], 2] = -np.inf
    struck[has[3::4]] *= np.float32(7.5)          # any length
    ref = restated(world, leaf, sx, pose, normals=struck)
    assert ref.counters["n_source_planes"] == len(has[3::4]) and ((ref.cls[has[3::4]] & GI.SOURCE) != 0).all()
    assert ((ref.cls[np.concatenate([has[0::4], has[1::4], has[2::4]])] & GI.SOURCE) == 0).all()
    assert ref.counters["n_target_planes"] == with_normals.counters["n_target_planes"]
    check_eval(device_eval(hip_lib, hip, m, pose, xyz=sx, normals=struck), ref, "struck out")


@pytest.mark.parametrize("n", [1, 1023, 1025, 2 * 1024 + 37])
def test_ragged_cloud_sizes(hip_lib, hip, frame, world, n):
    """One lane, a ragged tile, several workgroups with a tail, each with a normal array."""
    valid = np.nonzero(np.isfinite(frame["cloud"]).all(axis=1))[0]
    pick = valid[np.linspace(0, len(valid) - 1, n).astype(np.int64)]
    xyz, nrm = frame["cloud"][pick], frame["normals"][0.1][pick]
    ref = restated(world, 0.1, xyz, world["guess"], normals=nrm)
    assert n == 1 or (ref.n > 100 and ref.counters["n_plane_pairs"] > 0)
    check_eval(device_eval(hip_lib, hip, world["dev"][0.1], world["guess"], xyz=xyz, normals=nrm), ref)


def test_a_strip_of_two_tiles_per_row(hip_lib, hip, reg, world):
    """1100 x 24: a full tile and a ragged second one per row, the smallest shape in which all four point slots of a thread and the
    second blockIdx.x of the sphere route hold pixels."""
    from rgbd360_amd import synth
    depth = synth.render(synth.trajectory_pose(0, 7), 1100, 24, 7)[1]
    cloud = reg.sphere_cloud(depth, 2)
    with new_map(reg, 0.1) as m:
        m.insert_sphere(None, depth, world["P"], convention=2)
        ref = GI.GicpEvaluation(R.Map([(cloud, None, world["P"])], 0.1), cloud, world["guess"], 0.1, R.DEFAULT_BOX, 0.1)
        assert ref.n > 1000 and ref.counters["n_target_planes"] > 0
        check_eval(device_eval(hip_lib, hip, m, world["guess"], depth=depth, point_too=True), ref)


@pytest.mark.parametrize("params", [dict(min_support=3, max_flatness=0.2), dict(min_count=2), dict(epsilon=0.25), dict(max_dist=0.06)],
                         ids=["support3_flatness02", "count2", "epsilon025", "max_dist"])
def test_the_layer_and_weight_settings(hip_lib, hip, frame, world, params):
    ref = restated(world, 0.1, frame["cloud"], world["guess"], normals=frame["normals"][0.1], **params)
    assert ref.n > 1000 and ref.counters["n_target_planes"] > 0
    check_eval(device_eval(hip_lib, hip, world["dev"][0.1], world["guess"], xyz=frame["cloud"], normals=frame["normals"][0.1], point_too=True, **params),
               ref, str(params))


@pytest.mark.parametrize("leaf", LEAVES)
def test_the_point_to_point_limit(hip_lib, hip, frame, world, leaf):
    """use_target_normals = 0 without source normals: every weight is the identity's bits, and H, g and the final pose are those of
    rgbd360_map_align_cloud to the bounds for sums and poses (the point method assembles H from 17 sums, this one sums its 21 terms)."""
    m = world["dev"][leaf]
    guess = A.perturbed(world["P"], 0.01, 0.003, LIMIT_SEED[leaf])
    got = device_eval(hip_lib, hip, m, guess, xyz=frame["cloud"], use_target_normals=0)
    kept = got["cls"] != 0
    assert set(np.unique(got["cls"])) == {0, 1} and kept.sum() > 1000
    assert got["weight_cost"][kept, :6].tobytes() == np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), (kept.sum(), 1)).tobytes()
    check_eval(got, restated(world, leaf, frame["cloud"], guess, use_target_normals=0))
    assert got["sums"][28] == got["sums"][29]        # the cost is e.e
    pose_g, res_g = m.align_cloud_gicp(frame["cloud"], guess, use_target_normals=0)
    pose_p, res_p = m.align_cloud(frame["cloud"], guess)
    dr, dt = A.pose_error(pose_g, pose_p)
    print("leaf", leaf, "generalized ICP in its point-to-point limit against the point method: pose difference", (dr, dt), res_g["iterations"])
    assert (res_g["status"], res_g["iterations"], res_g["converged"], res_g["n_matched"]) == (res_p["status"], res_p["iterations"], res_p["converged"],
                                                                                            res_p["n_matched"])
    assert res_p["status"] == A.OK and dr <= POSE_TOL and dt <= POSE_TOL
    check_normal_equations(res_g["hessian"], res_g["gradient"], res_p["hessian"], res_p["gradient"])
    assert abs(res_g["fitness"] - res_p["fitness"]) <= 2e-6 * res_p["fitness"] and res_g["fitness_point"] == res_g["fitness"]
    assert res_g["n_target_planes"] == res_g["n_source_planes"] == res_g["n_plane_pairs"] == 0


def test_epsilon_one_makes_every_side_isotropic(hip_lib, hip, frame, world):
    """epsilon = 1: C_B = I and, where there is a source normal, C_A = I: the weights are the identity and half the identity."""
    nrm = frame["normals"][0.1]
    ref = restated(world, 0.1, frame["cloud"], world["guess"], normals=nrm, epsilon=1.0)
    got = device_eval(hip_lib, hip, world["dev"][0.1], world["guess"], xyz=frame["cloud"], normals=nrm, epsilon=1.0)
    check_eval(got, ref)
    kept, source = got["cls"] != 0, (got["cls"] & GI.SOURCE) != 0
    assert source.sum() > 1000 and (kept & ~source).sum() > 100
    diag = np.where(source, 0.5, 1.0)[kept]
    assert np.array_equal(got["weight_cost"][kept][:, [0, 3, 5]], np.repeat(diag[:, None], 3, axis=1)) and (got["weight_cost"][kept][:, [1, 2, 4]] == 0).all()


RESULT_COUNTERS = COUNTERS


def check_alignment(m, run, ref, P=None):
    pose, res = run()
    trace = m.align_trace()
    print("status", res["status"], "iterations", res["iterations"], "converged", res["converged"], "matches", [t[0] for t in trace], "restated",
          [t[0] for t in ref.trace], "margins", ref.margins, "pose difference", A.pose_error(pose, ref.pose))
    assert (res["status"], res["iterations"], res["converged"]) == (ref.status, ref.iterations, ref.converged)
    assert [t[0] for t in trace] == [t[0] for t in ref.trace]
    assert all(mg > 8.0 for mg in ref.margins)
    for (n, ss, u), (rn, rss, ru) in zip(trace, ref.trace):
        assert abs(ss - rss) <= 2e-6 * rss + 1e-12 and np.abs(u - ru).max() <= POSE_TOL
    dr, dt = A.pose_error(pose, ref.pose)
    assert dr <= POSE_TOL and dt <= POSE_TOL
    assert res["n_matched"] == ref.n_matched and abs(res["fitness"] - ref.fitness) <= 2e-6 * ref.fitness + 1e-15
    assert abs(res["fitness_point"] - ref.fitness_point) <= 2e-6 * ref.fitness_point + 1e-15
    for k in RESULT_COUNTERS:
        assert res[k] == ref.final.counters[k], k
    if ref.n_matched:
        check_normal_equations(res["hessian"], res["gradient"], ref.hessian, ref.gradient)
    if P is not None:
        (r1, t1), (r0, t0) = A.pose_error(pose, P), A.pose_error(ref.pose, P)
        assert r1 <= r0 + POSE_TOL and t1 <= t0 + POSE_TOL
    # the same bytes from run to run: the pose, the result and the trace
    pose2, res2 = run()
    trace2 = m.align_trace()
    assert pose2.tobytes() == pose.tobytes() and all(np.array_equal(np.asarray(res[k]), np.asarray(res2[k])) for k in res)
    assert len(trace) == len(trace2) and all(a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() for a, b in zip(trace, trace2))
    return pose, res


@pytest.mark.parametrize("route", ["sphere", "cloud", "cloud_normals"])
@pytest.mark.parametrize("leaf", LEAVES)
def test_the_whole_loop(frame, world, leaf, route):
    m = world["dev"][leaf]
    nrm = frame["normals"][leaf] if route == "cloud_normals" else None
    ref = GI.GicpAlignment(world["ref"][leaf], frame["cloud"], world["guess"], leaf, R.DEFAULT_BOX, leaf, normals=nrm, layers=world["layers"][leaf])
    assert ref.status == A.OK and ref.iterations >= 2 and ref.converged == 1
    assert (ref.final.counters["n_plane_pairs"] > 0) == (nrm is not None)
    run = ((lambda: m.align_sphere_gicp(frame["depth"], world["guess"], convention=2)) if route == "sphere"
           else (lambda: m.align_cloud_gicp(frame["cloud"], world["guess"], normals=nrm)))
    pose, res = check_alignment(m, run, ref, world["P"])
    r0, t0 = A.pose_error(world["guess"], world["P"])
    r1, t1 = A.pose_error(pose, world["P"])
    assert r1 <= 0.5 * r0 and t1 <= 0.5 * t0


def test_the_iteration_limit(frame, world):
    m = world["dev"][0.1]
    ref = GI.GicpAlignment(world["ref"][0.1], frame["cloud"], world["guess"], 0.1, R.DEFAULT_BOX, 0.1, max_iters=1, layers=world["layers"][0.1])
    assert ref.iterations == 1 and ref.converged == 0 and ref.status == A.OK
    check_alignment(m, lambda: m.align_sphere_gicp(frame["depth"], world["guess"], convention=2, max_iters=1), ref)
    ref0 = GI.GicpAlignment(world["ref"][0.1], frame["cloud"], world["guess"], 0.1, R.DEFAULT_BOX, 0.1, max_iters=0, layers=world["layers"][0.1])
    pose, res = check_alignment(m, lambda: m.align_sphere_gicp(frame["depth"], world["guess"], convention=2, max_iters=0), ref0)
    assert pose.tobytes() == world["guess"].tobytes() and res["iterations"] == 0 and res["n_matched"] > 1000 and m.align_trace() == []


def same_result(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(np.array_equal(np.asarray(a[1][k]), np.asarray(b[1][k])) for k in a[1])


def test_the_layer_follows_the_map(reg, frame, world):
    """Align, insert a second frame, align again: the normal layer is rebuilt behind the insert, and the result is that of a fresh map
    that holds both frames, byte for byte; with the second frame removed again (tombstones stay behind) it is the first result."""
    leaf, P, P_b, guess = 0.1, world["P"], world["P_b"], world["guess"]
    run = lambda mp: mp.align_sphere_gicp(frame["depth"], guess, convention=2)
    with new_map(reg, leaf) as m, new_map(reg, leaf) as both:
        m.insert_sphere(None, frame["depth"], P, convention=2)
        first = run(m)
        assert same_result(first, run(world["dev"][leaf]))
        m.insert_sphere(None, frame["depth_b"], P_b, convention=2)
        second = run(m)
        both.insert_sphere(None, frame["depth_b"], P_b, convention=2)          # the other order of insertion: other slots, the same voxels
        both.insert_sphere(None, frame["depth"], P, convention=2)
        assert len(both) == len(m) > len(world["dev"][leaf])
        assert same_result(second, run(both))
        assert second[1]["n_target_planes"] != first[1]["n_target_planes"] or second[0].tobytes() != first[0].tobytes()
        ref = GI.GicpAlignment(R.Map([(frame["cloud"], None, P), (frame["cloud_b"], None, P_b)], leaf), frame["cloud"], guess, leaf, R.DEFAULT_BOX, leaf)
        assert (second[1]["status"], second[1]["iterations"], second[1]["n_matched"]) == (ref.status, ref.iterations, ref.n_matched)
        assert second[1]["n_target_planes"] == ref.final.counters["n_target_planes"] and max(A.pose_error(second[0], ref.pose)) <= POSE_TOL
        st = m.remove_sphere(None, frame["depth_b"], P_b, convention=2)
        assert st["n_voxels_emptied"] > 0 and not m.mismatch and len(m) == len(world["dev"][leaf])
        assert m.census()["n_tombstones"] > 0
        assert same_result(first, run(m))


def test_a_map_as_the_source(reg, frame, world):
    """align_map_gicp: a map of frame b (at the identity: its world is the frame) against the map of frame a; the source is the list of
    b's voxels with their normals in ascending (i_z, i_y, i_x) order, the restated loop runs on the same list."""
    leaf = 0.1
    m = world["dev"][leaf]
    guess = A.perturbed(world["P_b"], 0.01, 0.003, SEED)
    with new_map(reg, leaf) as src:
        src.insert_sphere(None, frame["depth_b"], EYE, convention=2)
        sx, sn = GI.map_source(R.Map([(frame["cloud_b"], None, EYE)], leaf))
        dx, dn = src.gicp_source()
        assert dx.tobytes() == sx.tobytes() and dn.tobytes() == sn.tobytes()
        ref = GI.GicpAlignment(world["ref"][leaf], sx, guess, leaf, R.DEFAULT_BOX, leaf, normals=sn, layers=world["layers"][leaf])
        assert ref.status == A.OK and ref.converged == 1 and ref.final.counters["n_plane_pairs"] > 1000
        pose, res = check_alignment(m, lambda: m.align_map_gicp(src, guess), ref)
        r0, t0 = A.pose_error(guess, world["P_b"])
        r1, t1 = A.pose_error(pose, world["P_b"])
        print("map against map: guess", (r0, t0), "result", (r1, t1), res["n_plane_pairs"])
        assert res["status"] == A.OK and r1 < r0 and t1 < t0


def test_the_table_is_read_only_and_the_other_methods_are_unchanged(reg, frame, world):
    P = world["P"]
    with new_map(reg, 0.1) as m:
        m.insert_sphere(frame["rgb"], frame["depth"], P, convention=2)
        before, size = m.extract(), len(m)
        point_before = m.align_sphere(frame["depth"], world["guess"], convention=2)
        plane_before = m.align_sphere_plane(frame["depth"], world["guess"], convention=2)
        m.align_sphere_gicp(frame["depth"], world["guess"], convention=2)
        m.align_cloud_gicp(frame["cloud"], world["guess"], normals=frame["normals"][0.1], min_count=2, min_support=3)
        after = m.extract()
        assert len(m) == size and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        # the other methods behind this one, which left the widest row and the largest state in the shared buffers
        assert same_result(point_before, m.align_sphere(frame["depth"], world["guess"], convention=2))
        assert same_result(plane_before, m.align_sphere_plane(frame["depth"], world["guess"], convention=2))


def test_refusals_and_empties(hip_lib, hip, reg, frame, world):
    from rgbd360_amd import _lib
    from rgbd360_amd.register import pose_to_cm
    m = world["dev"][0.05]
    H = m._handle()
    d = np.ascontiguousarray(frame["depth"])
    dt = 0 if d.dtype == np.uint16 else 1
    x = np.ascontiguousarray(frame["cloud"])
    g, out, res = pose_to_cm(world["guess"]), np.full(16, 7, np.float32), _lib.MapAlignGicpResult()

    def sphere(depth=d, dtype=dt, conv=2, guess=g, pose_out=out, **kw):
        p = m.align_gicp_params(**kw)
        return hip_lib.rgbd360_map_align_gicp_sphere(H, vp(depth), d.strides[0], dtype, d.shape[0], d.shape[1], conv, vp(guess), 0, C.byref(p), vp(pose_out),
                                                     C.byref(res))

    def cloud(**kw):
        p = m.align_gicp_params(**kw)
        return hip_lib.rgbd360_map_align_gicp_cloud(H, vp(x), None, len(x), vp(g), 0, C.byref(p), vp(out), C.byref(res))

    nxt = float(np.nextafter(np.float32(0.05), np.float32(1)))
    above_one = float(np.nextafter(np.float32(1), np.float32(2)))
    for call in (sphere, cloud):
        assert call(max_dist=0.0) == -1 and call(max_dist=-1.0) == -1 and call(max_dist=nxt) == -1 and call(max_dist=float("nan")) == -1
        assert call(max_iters=-1) == -1 and call(max_iters=1001) == -1 and call(min_count=0) == -1 and call(eps=-1.0) == -1
        assert call(epsilon=0.0) == -1 and call(epsilon=-0.5) == -1 and call(epsilon=above_one) == -1 and call(epsilon=float("nan")) == -1
        assert call(min_support=0) == -1 and call(min_support=28) == -1 and call(max_flatness=-0.01) == -1 and call(max_flatness=float("nan")) == -1
    assert sphere(depth=None) == -1 and sphere(guess=None) == -1 and sphere(pose_out=None) == -1
    assert sphere(conv=3) == -1 and sphere(conv=-1) == -1 and sphere(dtype=2) == -1
    assert hip_lib.rgbd360_map_last_error(H) != b"" and (out == 7).all()
    p = m.align_gicp_params()
    assert hip_lib.rgbd360_map_align_gicp_cloud(H, None, None, 5, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == -1
    assert hip_lib.rgbd360_map_align_gicp_cloud(H, vp(x), None, -1, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == -1
    assert hip_lib.rgbd360_map_align_gicp_eval(H, None, 0, 0, 0, 0, 0, vp(x), None, 5, None, 0, C.byref(p), None, None, None, None, None, None) == -1
    bad = m.align_gicp_params(epsilon=2.0)
    assert hip_lib.rgbd360_map_align_gicp_eval(H, None, 0, 0, 0, 0, 0, vp(x), None, 5, vp(g), 0, C.byref(bad), None, None, None, None, None, None) == -1
    assert (out == 7).all()
    # empty inputs: NO_VALID_PIXELS, pose_out = guess
    assert hip_lib.rgbd360_map_align_gicp_cloud(H, None, None, 0, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == A.NO_VALID_PIXELS
    assert out.tobytes() == g.tobytes() and res.status == A.NO_VALID_PIXELS and res.n_matched == 0
    out[:] = 7
    assert hip_lib.rgbd360_map_align_gicp_sphere(H, vp(d), d.strides[0], dt, 0, d.shape[1], 2, vp(g), 0, None, vp(out), None) == A.NO_VALID_PIXELS
    assert out.tobytes() == g.tobytes()
    # an empty map: every point is searched, none matches
    with new_map(reg) as empty:
        ref = GI.GicpEvaluation(R.Map([], 0.05), frame["cloud"], world["guess"], 0.05, R.DEFAULT_BOX, 0.05)
        assert ref.n == 0 and ref.counters["n_valid"] > 0
        check_eval(device_eval(hip_lib, hip, empty, world["guess"], depth=frame["depth"]), ref)
        for run in (lambda: empty.align_sphere_gicp(frame["depth"], world["guess"], convention=2),
                    lambda: empty.align_cloud_gicp(frame["cloud"], world["guess"], normals=frame["normals"][0.05])):
            pose, r = run()
            assert r["status"] == A.NO_VALID_PIXELS and r["iterations"] == 0 and r["n_matched"] == 0 and r["fitness"] == 0.0 and r["fitness_point"] == 0.0
            assert pose.tobytes() == world["guess"].tobytes() and r["n_valid"] == ref.counters["n_valid"] and len(empty) == 0
    # and the map aligns afterwards (params NULL: the defaults)
    assert hip_lib.rgbd360_map_align_gicp_sphere(H, vp(d), d.strides[0], dt, d.shape[0], d.shape[1], 2, vp(g), 0, None, vp(out), C.byref(res)) == 0
    assert res.n_matched > 1000 and res.n_target_planes > 0 and res.n_source_planes == 0


ADAPTER_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "rgbd360/GlobalMap.hpp"
static std::vector<float> read(FILE* f) {
    long long n = 0;
    if (fread(&n, sizeof n, 1, f) != 1) return {};
    std::vector<float> v((size_t)n);
    if (n && fread(v.data(), sizeof(float), (size_t)n, f) != (size_t)n) return {};
    return v;
}
static void show(const char* what, int rc, const rgbd360::Mat4f& pose, const rgbd360_map_align_gicp_result& r) {
    printf("%s %d %d %d %lld %lld %lld %lld %a %a", what, rc, r.iterations, r.converged, r.n_matched, r.n_target_planes, r.n_source_planes, r.n_plane_pairs,
           r.fitness, r.fitness_point);
    for (int k = 0; k < 16; ++k) printf(" %a", (double)pose.m[k]);
    printf("\n");
}
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    const std::vector<float> a = read(f), b = read(f), pose_a = read(f), guess_v = read(f);
    fclose(f);
    rgbd360::RegisterPhotoICP align;
    rgbd360::GlobalMap target(align, rgbd360::FilterPointCloud(0.1f), 1 << 16), source(align, rgbd360::FilterPointCloud(0.1f), 1 << 16);
    rgbd360::Mat4f P, guess, pose;
    for (int k = 0; k < 16; ++k) P.m[k] = pose_a[k], guess.m[k] = guess_v[k];
    if (!target.insert(a.data(), nullptr, (long long)(a.size() / 3), P)) return 4;
    if (!source.insert(b.data(), nullptr, (long long)(b.size() / 3), rgbd360::Mat4f::Identity())) return 5;
    int rc = target.alignMapGICP(source, guess, pose);
    show("map", rc, pose, target.alignGicpResult());
    rgbd360_map_align_gicp_params p = target.alignGicpParams();
    p.use_target_normals = 0;
    rc = target.alignCloudGICP(b.data(), nullptr, (long long)(b.size() / 3), guess, pose, &p);
    show("cloud", rc, pose, target.alignGicpResult());
    return 0;
}
"""


def test_cpp_adapter_gives_the_python_wrappers_result(tmp_path, frame, world):
    """GlobalMap::alignMapGICP (the source's voxels read out, ordered and passed on in C++) and alignCloudGICP against
    VoxelMap.align_map_gicp / align_cloud_gicp on the same maps: the same bytes."""
    from rgbd360_amd import build
    from rgbd360_amd.register import pose_to_cm
    lib = build.build()
    guess = A.perturbed(world["P_b"], 0.01, 0.003, SEED)
    data = tmp_path / "pair.bin"
    with open(data, "wb") as f:
        for a in (frame["cloud"], frame["cloud_b"], pose_to_cm(world["P"]), pose_to_cm(guess)):
            f.write(np.int64(a.size).tobytes())
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    src = tmp_path / "gicp_adapter.cpp"
    src.write_text(ADAPTER_PROGRAM)
    exe = str(tmp_path / "gicp_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.dirname(lib),
                           "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = [l.split() for l in subprocess.check_output([exe, str(data)], text=True).strip().splitlines()]
    assert [l[0] for l in out] == ["map", "cloud"]
    m = world["dev"][0.1]           # (frame a inserted as a sphere image there, as a cloud in the adapter: the same points, the same map)
    with new_map(world["dev"][0.1]._reg, 0.1) as source:
        source.insert_cloud(frame["cloud_b"], None, EYE)
        runs = [m.align_map_gicp(source, guess), m.align_cloud_gicp(frame["cloud_b"], guess, use_target_normals=0)]
    for line, (pose, res) in zip(out, runs):
        assert [int(v) for v in line[1:8]] == [res["status"], res["iterations"], res["converged"], res["n_matched"], res["n_target_planes"],
                                               res["n_source_planes"], res["n_plane_pairs"]], line
        assert float.fromhex(line[8]) == res["fitness"] and float.fromhex(line[9]) == res["fitness_point"]
        assert np.array([float.fromhex(v) for v in line[10:]], np.float32).tobytes() == pose_to_cm(pose).tobytes()
    assert runs[0][1]["status"] == A.OK and runs[0][1]["n_plane_pairs"] > 1000
