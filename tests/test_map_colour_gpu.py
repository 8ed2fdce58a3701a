"""The voxel map's colour layer (rgbd360_map_colours, csrc/map_colour.h) and coloured ICP against the map (rgbd360_map_align_colour_*,
csrc/map_align_colour.h) on the device against the numpy restatement of their definitions (tests/map_colour_reference.py): the layer's
read-out bit for bit (intensity, gradient, status, order) whatever the order of insertion, the capacity or a rehash, and behind every
kind of write; per source point the matched key and d2 bit for bit (and equal to rgbd360_map_align_eval's), the class byte exact, both
residuals bit for bit in float64, exact counters, the 31 sums to the project's bound for sums (2e-6 |sum| + 1e-9; H to 2e-5 max|H|,
DESIGN.md 4); the whole loop -- status, iteration count, the matches per iteration -- and the pose to the device-mode bound (5e-6 rad,
5e-6 m); the sliding scene of tests/test_map_colour_cpu.py on the device.  The fixtures and helpers repeat those of
tests/test_map_align_gicp_gpu.py.

The guess of the loop tests (1 cm, 3 mrad, seed 6): every stop / continue decision of the restated loops lies a factor of more than 8
from eps.  Measured on the CPU (with numpy's sphere cloud, a few ulp from the device's) over seeds 1 .. 12: seed 6 has the smallest factor
25.1 at leaf 0.05 (2 steps) and 97.9 at leaf 0.1 (2 steps); the other seeds' smallest factors at 0.05 lie between 1.1 and 5.0.  On the
sliding scene (guess 10 cm along the free axis) the factors are 1.1e4, 2.5 and 1.3e3 at leaf 0.05 and 1.2e4, 24.5 and 5.5 at leaf 0.1: the
decisions there are not a factor of 8 from eps, so that test asserts the final pose against the restated one and the truth and, only where
the restated factors allow it, the iteration count."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_align_reference as A
import map_colour_reference as CR
import voxel_map_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
F = np.float32
SEED = 6
POSE_TOL = 5e-6
LEAVES = (0.05, 0.1)
COUNTERS = CR.COUNTERS
SLIDING_MEASURED = {0.05: (3.18e-6, 6.41e-5), 0.1: (2.51e-6, 7.63e-5)}          # tests/test_map_colour_cpu.py


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
    (rgb, depth), (rgb_b, depth_b), t_rel = small_pair
    return dict(rgb=np.ascontiguousarray(rgb), depth=depth, cloud=reg.sphere_cloud(depth, 2), colours=np.ascontiguousarray(rgb).reshape(-1, 3),
                rgb_b=np.ascontiguousarray(rgb_b), depth_b=depth_b, cloud_b=reg.sphere_cloud(depth_b, 2), t_rel=t_rel)


@pytest.fixture(scope="module")
def world(reg, frame):
    """The frame with its colours in maps of 0.05 m and 0.1 m at the general pose, on the device and restated; an alignment never changes
    a map."""
    P = R.general_pose()
    maps = {leaf: new_map(reg, leaf) for leaf in LEAVES}
    for m in maps.values():
        m.insert_sphere(frame["rgb"], frame["depth"], P, convention=2)
    ref = {leaf: R.Map([(frame["cloud"], frame["colours"], P)], leaf) for leaf in maps}
    yield dict(P=P, guess=A.perturbed(P, 0.01, 0.003, SEED), dev=maps, ref=ref, layers={leaf: CR.Layers(ref[leaf]) for leaf in maps},
               P_b=(np.asarray(P, np.float64) @ frame["t_rel"]).astype(np.float32))
    for m in maps.values():
        m.close()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the layer ----------------------------------------------------------------------------------------------------------------------------
def assert_colours_equal(got, ref, what=""):
    """got: VoxelMap.colours(); ref: CR.colours() -- bit for bit, the order included."""
    xyz, intensity, gradient, status, count, key3, stats = got
    assert np.array_equal(key3, ref["key3"]), what
    assert np.array_equal(count, ref["count"]) and xyz.tobytes() == ref["xyz"].tobytes(), what
    assert np.array_equal(status, ref["status"]), (what, np.bincount(status, minlength=4), np.bincount(ref["status"], minlength=4))
    assert intensity.tobytes() == ref["intensity"].tobytes(), what
    differ = np.nonzero((gradient != ref["gradient"]).any(axis=1))[0]
    assert gradient.tobytes() == ref["gradient"].tobytes(), (what, len(differ), gradient[differ[:3]], ref["gradient"][differ[:3]])
    assert stats == ref["stats"], (what, stats, ref["stats"])


LAYER_PARAMS = {"defaults": {}, "support6_spread01": dict(min_gradient_support=6, min_spread=0.1), "count2_support3": dict(min_count=2, min_support=3)}


@pytest.mark.parametrize("params", list(LAYER_PARAMS), ids=list(LAYER_PARAMS))
@pytest.mark.parametrize("leaf", LEAVES)
def test_the_layer_equals_the_restatement(reg, frame, world, leaf, params):
    kw = LAYER_PARAMS[params]
    ref = CR.colours(world["ref"][leaf], **kw)
    st = ref["stats"]
    print("leaf", leaf, params, st)
    # no class goes untested: every leaf meets all of them under the second parameter set, the third adds voxels below min_count
    if params == "support6_spread01":
        assert st["n_gradients"] > 1000 and st["n_no_normal"] >= 1 and st["n_no_gradient"] >= 1
    if params == "count2_support3":
        assert st["n_below_min_count"] >= 1 and st["n_gradients"] > 1000
    assert st["n_gradients"] > 1000 and st["n_no_normal"] >= 1
    m = world["dev"][leaf]
    got = m.colours(**kw)
    assert_colours_equal(got, ref, "the world's map")
    assert (got[1] >= 0).all() and (got[1] <= 1).all() and not got[2][got[3] != CR.OK].any()
    if params != "defaults":
        return
    # another order of insertion (the cloud's halves swapped), another capacity, and after a rehash: other slots, the same layer
    half = len(frame["cloud"]) // 2
    with new_map(reg, leaf, capacity=1 << 17) as other:
        other.insert_cloud(frame["cloud"][half:], frame["colours"][half:], world["P"])
        other.insert_cloud(frame["cloud"][:half], frame["colours"][:half], world["P"])
        assert_colours_equal(other.colours(), ref, "another order and capacity")
        assert other.rehash(1 << 15) == 0
        assert_colours_equal(other.colours(), ref, "after rehash")
        few = other.colours(max_out=100)
        assert all(a.tobytes() == b[:100].tobytes() for a, b in zip(few[:6], got[:6])) and few[6] == got[6]


def test_the_layer_follows_the_map(reg, frame, world):
    """Rebuilt behind an insert, a removal and a carve -- each time the layer of the table as it then stands, restated from the table's own
    records -- reused otherwise (the same bytes), released and built again; the table's bytes never change."""
    leaf, P, P_b = 0.1, world["P"], world["P_b"]
    with new_map(reg, leaf) as m:
        m.insert_sphere(frame["rgb"], frame["depth"], P, convention=2)
        table_bytes = m.bytes
        assert m.colour_bytes == 0
        first = m.colours()
        assert_colours_equal(first, CR.colours(world["ref"][leaf]), "first")
        assert m.colour_bytes == 16 * (1 << 16) and m.bytes == table_bytes
        again = m.colours()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:6], again[:6])) and first[6] == again[6]
        loose = m.colours(min_gradient_support=8)
        assert_colours_equal(loose, CR.colours(world["ref"][leaf], min_gradient_support=8), "another parameter")
        assert loose[6]["n_no_gradient"] > first[6]["n_no_gradient"]
        assert_colours_equal(m.colours(), CR.colours(world["ref"][leaf]), "the parameter back")
        m.insert_sphere(frame["rgb_b"], frame["depth_b"], P_b, convention=2)
        both = CR.colours(R.Map([(frame["cloud"], frame["colours"], P), (frame["cloud_b"], frame["rgb_b"].reshape(-1, 3), P_b)], leaf))
        second = m.colours()
        assert_colours_equal(second, both, "after an insert")
        assert len(second[0]) > len(first[0])
        assert_colours_equal(m.colours(), CR.colours(CR.RecordMap(m.records())), "... which is what the records restate")
        st = m.remove_sphere(frame["rgb_b"], frame["depth_b"], P_b, convention=2)
        assert st["n_voxels_emptied"] > 0 and not m.mismatch and m.census()["n_tombstones"] > 0
        third = m.colours()
        assert_colours_equal(third, CR.colours(world["ref"][leaf]), "after the removal")
        wrong = P_b.copy()          # frame b once more, 0.4 m off: a ghost that frame a looks through and the carve erases
        wrong[0, 3] += np.float32(0.4)
        m.insert_sphere(frame["rgb_b"], frame["depth_b"], wrong, convention=2)
        ghosted = m.colours()
        m.observe_sphere(frame["depth"], P, convention=2)
        carved = m.carve()
        assert carved["n_voxels_carved"] > 0 and len(m) < len(ghosted[0]), carved
        fourth = m.colours()
        assert_colours_equal(fourth, CR.colours(CR.RecordMap(m.records())), "after a carve")
        assert m.release_colours() is None and m.colour_bytes == 0 and m.bytes == table_bytes
        assert_colours_equal(m.colours(), CR.colours(CR.RecordMap(m.records())), "after release")
        assert m.colour_bytes == 16 * (1 << 16) and m.bytes == table_bytes
    # a map fed without colours: zero intensities and zero gradients, nothing tells
    with new_map(reg, leaf) as grey:
        grey.insert_sphere(None, frame["depth"], P, convention=2)
        got = grey.colours()
        assert not got[1].any() and not got[2].any() and (got[3] == CR.OK).sum() > 1000


# ---- the evaluation -----------------------------------------------------------------------------------------------------------------------
def device_eval(hip_lib, hip, m, pose, rgb=None, depth=None, convention=2, xyz=None, rgb3=None, point_too=False, **params):
    """rgbd360_map_align_colour_eval: dict(key3, d2, residuals, cls, sums, counters); point_too: rgbd360_map_align_eval's key3 and d2 of the
    same inputs are compared on the spot."""
    from rgbd360_amd.register import pose_to_cm
    n = depth.size if depth is not None else len(xyz)
    k = max(n, 1)
    host = dict(key3=np.zeros((k, 3), np.int32), d2=np.zeros(k, np.float32), residuals=np.full((k, 2), 9.0, np.float64), cls=np.full(k, 99, np.uint8))
    dev = {}
    for name, a in host.items():
        dev[name] = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev[name]), a.nbytes) == 0
    sums, counters = np.zeros(31, np.float64), np.zeros(5, np.int64)
    p = m.align_colour_params(**params)
    cm = pose_to_cm(pose)
    x = None if xyz is None else np.ascontiguousarray(xyz, np.float32)
    c3 = None if rgb3 is None else np.ascontiguousarray(rgb3, np.uint8)
    if depth is not None:
        src = (vp(rgb), rgb.strides[0], vp(depth), depth.strides[0], 0 if depth.dtype == np.uint16 else 1, depth.shape[0], depth.shape[1], convention,
               None, None, 0)
    else:
        assert c3.shape == x.shape
        src = (None, 0, None, 0, 0, 0, 0, 0, vp(x), vp(c3), len(x))
    rc = hip_lib.rgbd360_map_align_colour_eval(m._handle(), *src, vp(cm), 0, C.byref(p), vp(sums), vp(counters), dev["key3"], dev["d2"], dev["residuals"],
                                               dev["cls"])
    assert rc == 0, (rc, hip_lib.rgbd360_map_last_error(m._handle()))
    for name, a in host.items():
        assert hip.hipMemcpy(vp(a), dev[name], a.nbytes, 2) == 0
    out = {name: a[:n] for name, a in host.items()}
    if point_too:
        key, d2 = np.zeros((k, 3), np.int32), np.zeros(k, np.float32)
        pp = m.align_params(**{f: v for f, v in params.items() if f in ("max_dist", "max_iters", "eps", "min_count", "min_matches")})
        s17, cc = np.zeros(17, np.float64), np.zeros(3, np.int64)
        rc = hip_lib.rgbd360_map_align_eval(m._handle(), *src[2:9], src[10], vp(cm), 0, C.byref(pp), vp(s17), vp(cc), dev["key3"], dev["d2"], 0, None, None)
        assert rc == 0 and hip.hipMemcpy(vp(key), dev["key3"], key.nbytes, 2) == 0 and hip.hipMemcpy(vp(d2), dev["d2"], d2.nbytes, 2) == 0
        assert np.array_equal(key[:n], out["key3"]) and d2[:n].tobytes() == out["d2"].tobytes()
        assert cc.tolist() == counters[:3].tolist()
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
    differ = np.nonzero((got["residuals"] != ref.residuals).any(axis=1))[0]
    assert got["residuals"].tobytes() == ref.residuals.tobytes(), (what, len(differ), got["residuals"][differ[:3]], ref.residuals[differ[:3]])
    scale = np.maximum(np.abs(ref.sums), 1e-300)
    print(what, "contributing", ref.n, ref.counters, "largest relative difference of a sum", np.max(np.abs(got["sums"] - ref.sums) / scale))
    assert np.all(np.abs(got["sums"] - ref.sums) <= 2e-6 * np.abs(ref.sums) + 1e-9), (what, got["sums"], ref.sums)


def check_normal_equations(H, g, ref_H, ref_g):
    assert np.abs(H - ref_H).max() <= 2e-5 * np.abs(ref_H).max()
    assert np.abs(g - ref_g).max() <= 2e-5 * max(np.abs(ref_g).max(), 1e-30) + 2e-6 * np.abs(ref_H).max() * 1e-3


def restated(world, leaf, xyz, rgb3, pose, box=R.DEFAULT_BOX, **kw):
    return CR.ColourEvaluation(world["ref"][leaf], xyz, rgb3, pose, leaf, box, kw.pop("max_dist", leaf), layers=world["layers"][leaf], **kw)


@pytest.mark.parametrize("at", ["map_pose", "perturbed"])
@pytest.mark.parametrize("leaf", LEAVES)
def test_evaluation_equals_the_restatement_and_the_cloud_route(hip_lib, hip, frame, world, leaf, at):
    pose = world["P"] if at == "map_pose" else world["guess"]
    m = world["dev"][leaf]
    ref = restated(world, leaf, frame["cloud"], frame["colours"], pose)
    c = ref.counters
    assert ref.n > 1000 and c["n_box_rejected"] > 0 and c["n_no_normal"] > 0
    assert {0, CR.KEPT, CR.KEPT | CR.DROPPED_NO_NORMAL} <= set(np.unique(ref.cls))
    a = device_eval(hip_lib, hip, m, pose, rgb=frame["rgb"], depth=frame["depth"], point_too=True)
    check_eval(a, ref, "sphere")
    b = device_eval(hip_lib, hip, m, pose, xyz=frame["cloud"], rgb3=frame["colours"], point_too=True)
    check_eval(b, ref, "cloud")
    # the same row from both routes: the same points and bytes per point, another tiling, so the float64 sums agree to the bound
    assert a["sums"][0] == b["sums"][0] and a["counters"] == b["counters"]
    assert a["residuals"].tobytes() == b["residuals"].tobytes() and a["cls"].tobytes() == b["cls"].tobytes()
    assert np.all(np.abs(a["sums"] - b["sums"]) <= 2e-6 * np.abs(ref.sums) + 1e-9)
    # voxels without a gradient contribute with d = 0: a stricter support brings the class in at either leaf
    ref2 = restated(world, leaf, frame["cloud"], frame["colours"], pose, min_gradient_support=6)
    assert ref2.counters["n_no_gradient"] > 0 and (CR.KEPT | CR.ZERO_GRADIENT) in set(np.unique(ref2.cls)) and ref2.n == ref.n
    check_eval(device_eval(hip_lib, hip, m, pose, xyz=frame["cloud"], rgb3=frame["colours"], min_gradient_support=6), ref2, "support 6")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025])
def test_ragged_cloud_sizes(hip_lib, hip, frame, world, n):
    """One lane, a wave less one / full / plus one, a tile less one / full / plus one (a second workgroup of one point)."""
    valid = np.nonzero(np.isfinite(frame["cloud"]).all(axis=1))[0]
    pick = valid[np.linspace(0, len(valid) - 1, n).astype(np.int64)]
    xyz, col = frame["cloud"][pick], frame["colours"][pick]
    ref = restated(world, 0.1, xyz, col, world["guess"])
    assert n < 63 or ref.n > n // 4
    check_eval(device_eval(hip_lib, hip, world["dev"][0.1], world["guess"], xyz=xyz, rgb3=col, point_too=True), ref, "n %d" % n)


def test_a_strip_of_two_tiles_per_row(hip_lib, hip, reg, world):
    """1100 x 24: a full tile and a ragged second one per row, the smallest shape in which all four point slots of a thread and the
    second blockIdx.x of the sphere route hold pixels; the colour rows are read at their own step."""
    from rgbd360_amd import synth
    rgb, depth = synth.render(synth.trajectory_pose(0, 7), 1100, 24, 7)[:2]
    rgb = np.ascontiguousarray(rgb)
    cloud = reg.sphere_cloud(depth, 2)
    with new_map(reg, 0.1) as m:
        m.insert_sphere(rgb, depth, world["P"], convention=2)
        ref = CR.ColourEvaluation(R.Map([(cloud, rgb.reshape(-1, 3), world["P"])], 0.1), cloud, rgb.reshape(-1, 3), world["guess"], 0.1, R.DEFAULT_BOX, 0.1)
        assert ref.n > 1000
        check_eval(device_eval(hip_lib, hip, m, world["guess"], rgb=rgb, depth=depth, point_too=True), ref, "strip")
        padded = np.zeros((24, 1100 + 9, 3), np.uint8)          # a row step longer than a row
        padded[:, :1100] = rgb
        check_eval(device_eval(hip_lib, hip, m, world["guess"], rgb=padded[:, :1100], depth=depth), ref, "strided colour rows")


def test_lambda_limits(hip_lib, hip, frame, world):
    """lambda_geometric = 1: n, H, g, the cost and sum r_G^2 do not depend on the colours passed -- the same bits with random bytes; the
    one word of the row that does is sum r_C^2, which reports them.  lambda_geometric = 0 is accepted: the photometric term alone."""
    m, pose = world["dev"][0.1], world["guess"]
    noise = np.random.default_rng(2).integers(0, 256, frame["colours"].shape, dtype=np.uint8)
    a = device_eval(hip_lib, hip, m, pose, xyz=frame["cloud"], rgb3=frame["colours"], lambda_geometric=1.0)
    b = device_eval(hip_lib, hip, m, pose, xyz=frame["cloud"], rgb3=noise, lambda_geometric=1.0)
    check_eval(a, restated(world, 0.1, frame["cloud"], frame["colours"], pose, lambda_geometric=1.0), "lambda 1")
    assert a["sums"][:30].tobytes() == b["sums"][:30].tobytes() and a["counters"] == b["counters"] and a["cls"].tobytes() == b["cls"].tobytes()
    assert a["residuals"][:, 0].tobytes() == b["residuals"][:, 0].tobytes() and a["sums"][30] != b["sums"][30]
    assert a["sums"][28] == a["sums"][29]          # the cost is sum r_G^2
    zero = device_eval(hip_lib, hip, m, pose, xyz=frame["cloud"], rgb3=frame["colours"], lambda_geometric=0.0)
    check_eval(zero, restated(world, 0.1, frame["cloud"], frame["colours"], pose, lambda_geometric=0.0), "lambda 0")
    assert zero["sums"][28] == zero["sums"][30] and zero["sums"][0] == a["sums"][0]
    pose0, res0 = m.align_cloud_colour(frame["cloud"], frame["colours"], pose, lambda_geometric=0.0, max_iters=0)
    assert res0["status"] == A.OK and res0["n_matched"] == int(a["sums"][0]) and res0["fitness"] == zero["sums"][30] / zero["sums"][0]
    pose1, res1 = m.align_cloud_colour(frame["cloud"], frame["colours"], pose, lambda_geometric=0.0, max_iters=1)
    assert res1["status"] in (A.OK, A.ILL_POSED) and res1["iterations"] <= 1


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------
def check_alignment(m, run, ref, margins=True):
    pose, res = run()
    trace = m.align_trace()
    print("status", res["status"], "iterations", res["iterations"], "converged", res["converged"], "matches", [t[0] for t in trace], "restated",
          [t[0] for t in ref.trace], "margins", ref.margins, "pose difference", A.pose_error(pose, ref.pose))
    if margins:
        assert all(mg > 8.0 for mg in ref.margins)
        assert (res["status"], res["iterations"], res["converged"]) == (ref.status, ref.iterations, ref.converged)
        assert [t[0] for t in trace] == [t[0] for t in ref.trace]
        for (n, ss, u), (rn, rss, ru) in zip(trace, ref.trace):
            assert abs(ss - rss) <= 2e-6 * rss + 1e-12 and np.abs(u - ru).max() <= POSE_TOL
        assert res["n_matched"] == ref.n_matched and abs(res["fitness"] - ref.fitness) <= 2e-6 * ref.fitness + 1e-15
        assert abs(res["rms_geometric"] - ref.rms_geometric) <= 2e-6 * ref.rms_geometric + 1e-15
        assert abs(res["rms_colour"] - ref.rms_colour) <= 2e-6 * ref.rms_colour + 1e-15
        for k in COUNTERS:
            assert res[k] == ref.final.counters[k], k
        if ref.n_matched:
            check_normal_equations(res["hessian"], res["gradient"], ref.hessian, ref.gradient)
    dr, dt = A.pose_error(pose, ref.pose)
    assert res["status"] == ref.status and dr <= POSE_TOL and dt <= POSE_TOL
    # the same bytes from run to run: the pose, the result and the trace
    pose2, res2 = run()
    trace2 = m.align_trace()
    assert pose2.tobytes() == pose.tobytes() and all(np.array_equal(np.asarray(res[k]), np.asarray(res2[k])) for k in res)
    assert len(trace) == len(trace2) and all(a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() for a, b in zip(trace, trace2))
    return pose, res


@pytest.mark.parametrize("route", ["sphere", "cloud"])
@pytest.mark.parametrize("leaf", LEAVES)
def test_the_whole_loop(frame, world, leaf, route):
    m = world["dev"][leaf]
    ref = CR.ColourAlignment(world["ref"][leaf], frame["cloud"], frame["colours"], world["guess"], leaf, R.DEFAULT_BOX, leaf, layers=world["layers"][leaf])
    assert ref.status == A.OK and ref.iterations >= 2 and ref.converged == 1
    run = ((lambda: m.align_sphere_colour(frame["rgb"], frame["depth"], world["guess"], convention=2)) if route == "sphere"
           else (lambda: m.align_cloud_colour(frame["cloud"], frame["colours"], world["guess"])))
    pose, res = check_alignment(m, run, ref)
    r0, t0 = A.pose_error(world["guess"], world["P"])
    r1, t1 = A.pose_error(pose, world["P"])
    assert r1 <= 0.5 * r0 and t1 <= 0.5 * t0


def test_the_iteration_limit(frame, world):
    m = world["dev"][0.1]
    args = (world["ref"][0.1], frame["cloud"], frame["colours"], world["guess"], 0.1, R.DEFAULT_BOX, 0.1)
    ref = CR.ColourAlignment(*args, max_iters=1, layers=world["layers"][0.1])
    assert ref.iterations == 1 and ref.converged == 0 and ref.status == A.OK
    check_alignment(m, lambda: m.align_sphere_colour(frame["rgb"], frame["depth"], world["guess"], convention=2, max_iters=1), ref)
    ref0 = CR.ColourAlignment(*args, max_iters=0, layers=world["layers"][0.1])
    pose, res = check_alignment(m, lambda: m.align_sphere_colour(frame["rgb"], frame["depth"], world["guess"], convention=2, max_iters=0), ref0)
    assert pose.tobytes() == world["guess"].tobytes() and res["iterations"] == 0 and res["n_matched"] > 1000 and m.align_trace() == []


@pytest.mark.parametrize("leaf", LEAVES)
def test_the_sliding_scene_on_the_device(reg, leaf):
    """The textured floor and wall of tests/test_map_colour_cpu.py: the device ends on the restated pose to the device-mode bound, hence
    within the recorded distance of the truth (asserted: twice the recorded distance plus the bound), from a guess 10 cm along the axis
    that the point-to-plane method on the same map cannot see."""
    mx, mc, sx, sc = CR.sliding_scene()
    guess = CR.sliding_guess(0.10)
    ref_map = R.Map([(mx, mc, EYE)], leaf, None)
    ref = CR.ColourAlignment(ref_map, sx, sc, guess, leaf, None, leaf)
    assert ref.status == A.OK and ref.converged == 1
    with new_map(reg, leaf, box=None) as m:
        m.insert_cloud(mx, mc, EYE)
        assert_colours_equal(m.colours(), CR.colours(ref_map), "the scene's layer")
        pose, res = check_alignment(m, lambda: m.align_cloud_colour(sx, sc, guess), ref, margins=all(mg > 8.0 for mg in ref.margins))
        rot, trans = A.pose_error(pose, EYE)
        print("leaf", leaf, "ended", (rot, trans), "restated", A.pose_error(ref.pose, EYE), "iterations", res["iterations"], ref.iterations)
        assert res["converged"] == 1 and rot <= 2 * SLIDING_MEASURED[leaf][0] + POSE_TOL and trans <= 2 * SLIDING_MEASURED[leaf][1] + POSE_TOL
        plane_pose, plane = m.align_cloud_plane(sx, guess)
        print("point-to-plane on the same map: status", plane["status"], "ended", A.pose_error(plane_pose, EYE))
        assert plane["status"] == A.ILL_POSED or A.pose_error(plane_pose, EYE)[1] > 0.05


# ---- non-interference, refusals, the adapter ---------------------------------------------------------------------------------------------
def same_result(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(np.array_equal(np.asarray(a[1][k]), np.asarray(b[1][k])) for k in a[1])


def by_key(got):
    """The records of VoxelMap.normals(), which come in no specified order, ordered by (i_z, i_y, i_x)."""
    key3 = got[5]
    order = np.lexsort((key3[:, 0], key3[:, 1], key3[:, 2]))
    return [np.ascontiguousarray(a[order]) for a in got[:6]]


def test_the_table_is_read_only_and_the_other_methods_are_unchanged(reg, frame, world):
    P, guess = world["P"], world["guess"]
    with new_map(reg, 0.1) as m:
        m.insert_sphere(frame["rgb"], frame["depth"], P, convention=2)
        before, size, records = m.extract(), len(m), m.records()
        point_before = m.align_sphere(frame["depth"], guess, convention=2)
        plane_before = m.align_sphere_plane(frame["depth"], guess, convention=2)
        gicp_before = m.align_sphere_gicp(frame["depth"], guess, convention=2)
        normals_before = m.normals()
        m.align_sphere_colour(frame["rgb"], frame["depth"], guess, convention=2)
        m.align_cloud_colour(frame["cloud"], frame["colours"], guess, min_count=2, min_support=3, min_gradient_support=6)
        after = m.extract()
        assert len(m) == size and all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and m.records().tobytes() == records.tobytes()
        # the other methods behind this one, which left its row and state in the shared buffers and another normal layer behind
        assert same_result(point_before, m.align_sphere(frame["depth"], guess, convention=2))
        assert same_result(plane_before, m.align_sphere_plane(frame["depth"], guess, convention=2))
        assert same_result(gicp_before, m.align_sphere_gicp(frame["depth"], guess, convention=2))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(by_key(normals_before), by_key(m.normals())))
        # a level of the pyramid is a map like any other to a reader: its layers are its own
        lvl = m.level(1)
        assert_colours_equal(lvl.colours(), CR.colours(CR.RecordMap(lvl.records())), "level 1")
        pose, res = lvl.align_cloud_colour(frame["cloud"], frame["colours"], guess)
        assert res["status"] == A.OK and res["n_matched"] > 1000 and same_result((pose, res), lvl.align_cloud_colour(frame["cloud"], frame["colours"], guess))


def test_refusals_and_empties(hip_lib, hip, reg, frame, world):
    from rgbd360_amd import _lib
    from rgbd360_amd.register import pose_to_cm
    m = world["dev"][0.05]
    H = m._handle()
    d, rgb = np.ascontiguousarray(frame["depth"]), frame["rgb"]
    dt = 0 if d.dtype == np.uint16 else 1
    x, c3 = np.ascontiguousarray(frame["cloud"]), np.ascontiguousarray(frame["colours"])
    g, out, res = pose_to_cm(world["guess"]), np.full(16, 7, np.float32), _lib.MapAlignColourResult()
    res.n_matched = -5

    def sphere(colour=rgb, depth=d, dtype=dt, conv=2, guess=g, pose_out=out):
        p = m.align_colour_params()
        return hip_lib.rgbd360_map_align_colour_sphere(H, vp(colour), rgb.strides[0], vp(depth), d.strides[0], dtype, d.shape[0], d.shape[1], conv, vp(guess), 0,
                                                       C.byref(p), vp(pose_out), C.byref(res))

    def raw(**fields):          # (the wrapper refuses these itself: set on the struct)
        p = m.align_colour_params()
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    def cloud(p):
        return hip_lib.rgbd360_map_align_colour_cloud(H, vp(x), vp(c3), len(x), vp(g), 0, C.byref(p), vp(out), C.byref(res))

    nxt = float(np.nextafter(np.float32(0.05), np.float32(1)))
    above_one = float(np.nextafter(np.float32(1), np.float32(2)))
    for bad in (dict(max_dist=0.0), dict(max_dist=nxt), dict(max_dist=float("nan")), dict(max_iters=-1), dict(max_iters=1001), dict(min_count=0),
                dict(eps=-1.0), dict(lambda_geometric=above_one), dict(lambda_geometric=-0.001), dict(lambda_geometric=float("nan")), dict(min_support=0),
                dict(min_support=28), dict(max_flatness=-0.01), dict(min_gradient_support=0), dict(min_gradient_support=27), dict(min_spread=-0.1),
                dict(min_spread=float("nan"))):
        assert cloud(raw(**bad)) == -1, bad
    assert sphere(colour=None) == -1 and b"colours" in hip_lib.rgbd360_map_last_error(H)
    assert sphere(depth=None) == -1 and sphere(guess=None) == -1 and sphere(pose_out=None) == -1
    assert sphere(conv=3) == -1 and sphere(conv=-1) == -1 and sphere(dtype=2) == -1
    p = m.align_colour_params()
    assert hip_lib.rgbd360_map_align_colour_cloud(H, vp(x), None, len(x), vp(g), 0, C.byref(p), vp(out), C.byref(res)) == -1          # no colours
    assert hip_lib.rgbd360_map_align_colour_cloud(H, None, vp(c3), 5, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == -1
    assert hip_lib.rgbd360_map_align_colour_cloud(H, vp(x), vp(c3), -1, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == -1
    assert (out == 7).all() and res.n_matched == -5          # outputs untouched
    # the evaluation entry: a refused cloud leaves its row and counters zeroed, a refused image untouched
    row, cnt = np.full(31, 7.0), np.full(5, 7, np.int64)
    ev = hip_lib.rgbd360_map_align_colour_eval
    assert ev(H, None, 0, None, 0, 0, 0, 0, 0, vp(x), None, 5, vp(g), 0, C.byref(p), vp(row), vp(cnt), None, None, None, None) == -1
    assert not row.any() and not cnt.any()
    row[:], cnt[:] = 7.0, 7
    assert ev(H, None, 0, vp(d), d.strides[0], dt, d.shape[0], d.shape[1], 2, None, None, 0, vp(g), 0, C.byref(p), vp(row), vp(cnt), None, None, None, None) == -1
    assert (row == 7).all() and (cnt == 7).all()
    assert ev(H, None, 0, None, 0, 0, 0, 0, 0, vp(x), vp(c3), 5, None, 0, C.byref(p), vp(row), vp(cnt), None, None, None, None) == -1
    # the layer's read-out
    cp = m.colour_params()
    cp.min_gradient_support = 0
    st = _lib.MapColourStats()
    st.n_voxels = -5
    assert hip_lib.rgbd360_map_colours(H, C.byref(cp), 10, None, None, None, None, None, None, C.byref(st)) == -1 and st.n_voxels == -5
    assert hip_lib.rgbd360_map_colours(H, None, -1, None, None, None, None, None, None, C.byref(st)) == -1 and st.n_voxels == -5
    assert hip_lib.rgbd360_map_colours(H, None, 0, None, None, None, None, None, None, C.byref(st)) == len(m) and st.n_voxels == len(m)
    # empty inputs: NO_VALID_PIXELS, pose_out = guess
    assert hip_lib.rgbd360_map_align_colour_cloud(H, None, None, 0, vp(g), 0, C.byref(p), vp(out), C.byref(res)) == A.NO_VALID_PIXELS
    assert out.tobytes() == g.tobytes() and res.status == A.NO_VALID_PIXELS and res.n_matched == 0
    out[:] = 7
    assert hip_lib.rgbd360_map_align_colour_sphere(H, vp(rgb), rgb.strides[0], vp(d), d.strides[0], dt, 0, d.shape[1], 2, vp(g), 0, None, vp(out),
                                                   None) == A.NO_VALID_PIXELS
    assert out.tobytes() == g.tobytes()
    # an empty map: every point is searched, none matches; no layer is built
    with new_map(reg) as empty:
        ref = CR.ColourEvaluation(R.Map([], 0.05), frame["cloud"], frame["colours"], world["guess"], 0.05, R.DEFAULT_BOX, 0.05)
        assert ref.n == 0 and ref.counters["n_valid"] > 0
        check_eval(device_eval(hip_lib, hip, empty, world["guess"], rgb=rgb, depth=frame["depth"]), ref, "empty map")
        got = empty.colours()
        assert len(got[0]) == 0 and got[6]["n_voxels"] == 0 and empty.colour_bytes == 0
        for run in (lambda: empty.align_sphere_colour(rgb, frame["depth"], world["guess"], convention=2),
                    lambda: empty.align_cloud_colour(frame["cloud"], frame["colours"], world["guess"])):
            pose, r = run()
            assert r["status"] == A.NO_VALID_PIXELS and r["iterations"] == 0 and r["n_matched"] == 0 and r["fitness"] == 0.0 and r["rms_colour"] == 0.0
            assert pose.tobytes() == world["guess"].tobytes() and r["n_valid"] == ref.counters["n_valid"] and len(empty) == 0
    # and the map aligns afterwards (params NULL: the defaults)
    assert hip_lib.rgbd360_map_align_colour_sphere(H, vp(rgb), rgb.strides[0], vp(d), d.strides[0], dt, d.shape[0], d.shape[1], 2, vp(g), 0, None, vp(out),
                                                   C.byref(res)) == 0
    assert res.n_matched > 1000 and res.n_no_normal > 0 and res.rms_colour > 0


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
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    const std::vector<float> a = read(f), ac = read(f), pose_a = read(f), guess_v = read(f);
    fclose(f);
    std::vector<uint8_t> rgb3(ac.begin(), ac.end());
    rgbd360::RegisterPhotoICP align;
    rgbd360::GlobalMap target(align, rgbd360::FilterPointCloud(0.1f), 1 << 16);
    rgbd360::Mat4f P, guess, pose;
    for (int k = 0; k < 16; ++k) P.m[k] = pose_a[k], guess.m[k] = guess_v[k];
    if (!target.insert(a.data(), rgb3.data(), (long long)(a.size() / 3), P)) return 4;
    const int rc = target.alignCloudColour(a.data(), rgb3.data(), (long long)(a.size() / 3), guess, pose);
    const rgbd360_map_align_colour_result& r = target.alignColourResult();
    printf("cloud %d %d %d %lld %lld %lld %a %a %a", rc, r.iterations, r.converged, r.n_matched, r.n_no_normal, r.n_no_gradient, r.fitness, r.rms_geometric,
           r.rms_colour);
    for (int k = 0; k < 16; ++k) printf(" %a", (double)pose.m[k]);
    printf("\n");
    std::vector<float> xyz, intensity, gradient;
    std::vector<int32_t> status;
    const long long n = target.colours(xyz, intensity, gradient, &status);
    double si = 0.0, sg = 0.0;
    long long ok = 0;
    for (long long k = 0; k < n; ++k) si += intensity[k], sg += ((double)gradient[3 * k] + (double)gradient[3 * k + 1]) + (double)gradient[3 * k + 2], ok += status[k] == RGBD360_COLOUR_OK;
    printf("colours %lld %lld %lld %a %a %zu\n", n, ok, target.colourStats().n_gradients, si, sg, target.colourBytes());
    return 0;
}
"""


def test_cpp_adapter_gives_the_python_wrappers_result(tmp_path, frame, world):
    """GlobalMap::alignCloudColour and GlobalMap::colours against VoxelMap.align_cloud_colour / colours on the same map: the same bytes."""
    from rgbd360_amd import build
    from rgbd360_amd.register import pose_to_cm
    lib = build.build()
    data = tmp_path / "cloud.bin"
    with open(data, "wb") as f:
        for a in (frame["cloud"], frame["colours"].astype(np.float32), pose_to_cm(world["P"]), pose_to_cm(world["guess"])):
            f.write(np.int64(a.size).tobytes())
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    src = tmp_path / "colour_adapter.cpp"
    src.write_text(ADAPTER_PROGRAM)
    exe = str(tmp_path / "colour_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.dirname(lib),
                           "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = [l.split() for l in subprocess.check_output([exe, str(data)], text=True).strip().splitlines()]
    assert [l[0] for l in out] == ["cloud", "colours"]
    m = world["dev"][0.1]          # (the frame inserted as a sphere image there, as a cloud in the adapter: the same points, the same map)
    pose, res = m.align_cloud_colour(frame["cloud"], frame["colours"], world["guess"])
    line = out[0]
    assert [int(v) for v in line[1:7]] == [res["status"], res["iterations"], res["converged"], res["n_matched"], res["n_no_normal"], res["n_no_gradient"]], line
    assert [float.fromhex(v) for v in line[7:10]] == [res["fitness"], res["rms_geometric"], res["rms_colour"]]
    assert np.array([float.fromhex(v) for v in line[10:]], np.float32).tobytes() == pose_to_cm(pose).tobytes()
    assert res["status"] == A.OK and res["n_matched"] > 1000
    _, intensity, gradient, status, _, _, stats = m.colours()
    line = out[1]
    assert [int(v) for v in line[1:4]] == [len(m), int((status == CR.OK).sum()), stats["n_gradients"]] and int(line[6]) == m.colour_bytes
    assert float.fromhex(line[4]) == float(np.cumsum(intensity.astype(np.float64))[-1])
    assert float.fromhex(line[5]) == float(np.cumsum((gradient.astype(np.float64)[:, 0] + gradient.astype(np.float64)[:, 1]) + gradient.astype(np.float64)[:, 2])[-1])
