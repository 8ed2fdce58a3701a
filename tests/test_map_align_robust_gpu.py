"""The robust kernels of the alignments against the voxel map (rgbd360_map_set_align_robust; csrc/map_align.h: RobustWeight, vmap::Robust;
csrc/map_align_robust.h) on the device against the numpy restatement (tests/map_align_robust_reference.py).

Row bits: the row of rgbd360_map_align_robust_eval equals the restatement summed in the kernels' order (order="device") word for word --
except the probe word, which counts table slots and is no part of the definition, and Cauchy's sum rho, held to 2e-12 relative: its terms
are positive, log1p is within 2 ulp on the device and 1 ulp on the host per term, and at most 7500 additions of half an ulp each follow
(the frame has more points; the bound is kept).  w per point bit for bit.
The loops are compared as tests/test_map_align_plane_gpu.py compares the quadratic loop; the trial's six end errors are asserted on the
device by the assertions of tests/test_map_align_robust_cpu.py.  Shapes: clouds of 1, 1024, 1025, 2085 and 7500 points (one lane, a
full tile, a second workgroup with one point, a ragged third, eight workgroups) and one 256 x 128 frame as uint16 from host memory and as
float32 from device memory with padded rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import map_align_plane_reference as PL
import map_align_reference as A
import map_align_robust_reference as RB
import map_colour_reference as CO
import map_align_gicp_reference as GI
import voxel_map_reference as R
from test_map_align_robust_cpu import assert_trial

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
F = np.float32
POSE_TOL = 5e-6
LEAF = 0.1
DELTA = {RB.POINT: 0.03, RB.PLANE: 0.01, RB.GICP: 0.3, RB.COLOUR: 0.01}      # near the median sqrt(s) of each method's cost term
METHOD_NAMES = {RB.POINT: "point", RB.PLANE: "plane", RB.GICP: "gicp", RB.COLOUR: "colour"}
CLOUD_SIZES = (1, 1024, 1025, 2085, 7500)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


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


def new_map(reg, leaf=LEAF, capacity=1 << 16, box="default"):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, leaf, capacity)
    if box is None:
        m.set_box(None, None)
    return m


def to_device(hip, a):
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), max(a.nbytes, 8)) == 0 and hip.hipMemcpy(d, vp(a), a.nbytes, 1) == 0
    return d


@pytest.fixture(scope="module")
def corner(reg):
    """The trial (tests/map_align_robust_reference.trial) at both lifts: one device map of the corner scene at leaf 0.1 m, the restated
    map, the two sources, the pose and the guess; the cloud inputs cut from the 0.04 m source."""
    lifts = {lift: RB.trial(lift) for lift in (0.04, 0.06)}
    target, cloud, P, guess, _ = lifts[0.04]
    m = new_map(reg, box=None)
    m.insert_cloud(PL.corner_scene(101, step=0.02), None, EYE)
    assert len(m) == len(target) and not m.full
    clouds = {n: np.ascontiguousarray(cloud[np.linspace(0, len(cloud) - 1, n).astype(np.int64)]) for n in CLOUD_SIZES}
    yield dict(m=m, ref=target, P=P, guess=guess, clouds=clouds, lifts=lifts)
    m.close()


@pytest.fixture(scope="module")
def room(reg, hip):
    """One 256 x 128 frame of the synthetic room against a map of three others (as tests/test_map_render_gpu.py builds it), with colours;
    the frame as uint16 in host memory and as float32 in device memory with padded rows (and its colours beside it)."""
    from rgbd360_amd import synth
    frames = [tuple(np.ascontiguousarray(a) for a in synth.render(synth.trajectory_pose(k), 256, 128)[:2]) for k in range(4)]
    poses = [synth.trajectory_pose(k).astype(F) for k in range(4)]
    clouds = [reg.sphere_cloud(d, 2) for _, d in frames]
    m = new_map(reg)
    for k in range(3):
        m.insert_sphere(frames[k][0], frames[k][1], poses[k], convention=2)
    assert not m.full
    ref = R.Map([(clouds[k], frames[k][0].reshape(-1, 3), poses[k]) for k in range(3)], LEAF)
    rgb, depth = frames[3]
    assert depth.dtype == np.uint16 and depth.shape == (128, 256)
    metres = depth.astype(F) * F(0.001)
    wide_d, wide_c = np.zeros((128, 256 + 16), F), np.zeros((128, 256 + 8, 3), np.uint8)
    wide_d[:, :256], wide_c[:, :256] = metres, rgb
    assert reg.sphere_cloud(metres, 2).tobytes() == clouds[3].tobytes()
    dev_d, dev_c = to_device(hip, wide_d), to_device(hip, wide_c)
    rng = np.random.default_rng(5)
    v = rng.standard_normal((depth.size, 3))
    yield dict(m=m, ref=ref, rgb=rgb, depth=depth, cloud=clouds[3], colours=rgb.reshape(-1, 3), guess=A.perturbed(poses[3], 0.01, 0.003, 8), P=poses[3],
               dev=dict(depth=dev_d, depth_step=wide_d.strides[0], rgb=dev_c, rgb_step=wide_c.strides[0]),
               normals=np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True), F), gicp_layers=GI.Layers(ref), colour_layers=CO.Layers(ref))
    hip.hipFree(dev_d)
    hip.hipFree(dev_c)
    m.close()


def method_params(m, method, **kw):
    return {RB.POINT: m.align_params, RB.PLANE: m.align_plane_params, RB.GICP: m.align_gicp_params, RB.COLOUR: m.align_colour_params}[method](**kw)


def device_row(hip_lib, hip, m, method, pose, n, depth=None, depth_step=0, depth_type=0, shape=(0, 0), rgb=None, rgb_step=0, xyz=None, normals=None, rgb3=None,
               on_device=0, expect=0, **params):
    """rgbd360_map_align_robust_eval: (row[40], w per input point).  The pointers are host arrays or device addresses as on_device says."""
    from rgbd360_amd.register import pose_to_cm
    row = np.full(40, 7.0)
    w_host = np.full(max(n, 1), 9.0)
    w_dev = to_device(hip, w_host)
    p = method_params(m, method, **params)
    ptr = lambda a: a if isinstance(a, (C.c_void_p, type(None))) else vp(a)
    rc = hip_lib.rgbd360_map_align_robust_eval(m._handle(), method, ptr(rgb), rgb_step, ptr(depth), depth_step, depth_type, shape[0], shape[1], 2, ptr(xyz),
                                               ptr(normals), ptr(rgb3), 0 if xyz is None else n, vp(pose_to_cm(pose)), on_device, C.byref(p), vp(row), w_dev)
    assert rc == expect, (rc, hip_lib.rgbd360_map_last_error(m._handle()))
    assert hip.hipMemcpy(vp(w_host), w_dev, w_host.nbytes, 2) == 0
    hip.hipFree(w_dev)
    return row, w_host[:n]


def check_row(got_row, got_w, ref, what):
    method, words = ref.method, RB.WORDS[ref.method]
    probes, sum_sq = words - 2, RB.SUM_SQ[method]
    assert got_w.tobytes() == ref.w.tobytes(), (what, np.nonzero(got_w != ref.w)[0][:5])
    assert np.all(got_row[words + 2:] == 0.0), what
    exact = [k for k in range(words + 2) if k != probes and not (ref.kind == RB.CAUCHY and k == sum_sq)]
    differ = [k for k in exact if np.float64(got_row[k]).tobytes() != np.float64(ref.row[k]).tobytes()]
    assert not differ, (what, differ, got_row[differ], ref.row[differ])
    assert got_row[probes] >= got_row[words - 1], what         # (a searched point reads at least one slot)
    if ref.kind == RB.CAUCHY:
        err = abs(got_row[sum_sq] - ref.row[sum_sq]) / max(ref.row[sum_sq], 1e-300)
        print(what, "Cauchy's sum rho: relative difference", err)
        assert err <= 2e-12, (what, got_row[sum_sq], ref.row[sum_sq])
    print(what, "contributing", ref.n, "down-weighted", ref.n_downweighted, "sum w", ref.sum_w)


@pytest.mark.parametrize("kind", RB.KINDS, ids=[RB.KIND_NAMES[k] for k in RB.KINDS])
@pytest.mark.parametrize("method", [RB.POINT, RB.PLANE], ids=["point", "plane"])
def test_row_bits_on_the_clouds(hip_lib, hip, corner, method, kind):
    m = corner["m"]
    m.set_align_robust(method, kind, DELTA[method])
    try:
        for n, xyz in corner["clouds"].items():
            ref = RB.RobustEvaluation(method, kind, DELTA[method], corner["ref"], xyz, corner["guess"], LEAF, None, LEAF, order="device")
            assert n == 1 or (0 < ref.n_downweighted <= ref.n and ref.n > 0.5 * n)
            row, w = device_row(hip_lib, hip, m, method, corner["guess"], n, xyz=xyz)
            check_row(row, w, ref, "%s %s cloud of %d" % (METHOD_NAMES[method], RB.KIND_NAMES[kind], n))
    finally:
        m.set_align_robust(method, "none")


def frame_reference(room, method, kind):
    kw = {RB.GICP: dict(layers=room["gicp_layers"]), RB.COLOUR: dict(rgb=room["colours"], layers=room["colour_layers"])}.get(method, {})
    return RB.RobustEvaluation(method, kind, DELTA[method], room["ref"], room["cloud"], room["guess"], LEAF, R.DEFAULT_BOX, LEAF, order="device",
                               shape=room["depth"].shape, **kw)


@pytest.mark.parametrize("kind", RB.KINDS, ids=[RB.KIND_NAMES[k] for k in RB.KINDS])
@pytest.mark.parametrize("method", [RB.POINT, RB.PLANE, RB.GICP, RB.COLOUR], ids=["point", "plane", "gicp", "colour"])
def test_row_bits_on_the_frame_from_host_uint16_and_device_float32(hip_lib, hip, room, method, kind):
    m, d = room["m"], room["depth"]
    m.set_align_robust(method, kind, DELTA[method])
    try:
        ref = frame_reference(room, method, kind)
        assert ref.n > 2000 and 0 < ref.n_downweighted <= ref.n
        colour = method == RB.COLOUR
        row, w = device_row(hip_lib, hip, m, method, room["guess"], d.size, depth=d, depth_step=d.strides[0], depth_type=0, shape=d.shape,
                            rgb=room["rgb"] if colour else None, rgb_step=room["rgb"].strides[0] if colour else 0)
        check_row(row, w, ref, "%s %s uint16 host frame" % (METHOD_NAMES[method], RB.KIND_NAMES[kind]))
        dv = room["dev"]
        row2, w2 = device_row(hip_lib, hip, m, method, room["guess"], d.size, depth=dv["depth"], depth_step=dv["depth_step"], depth_type=1, shape=d.shape,
                              rgb=dv["rgb"] if colour else None, rgb_step=dv["rgb_step"] if colour else 0, on_device=1)
        assert row2.tobytes() == row.tobytes() and w2.tobytes() == w.tobytes()
    finally:
        m.set_align_robust(method, "none")


@pytest.mark.parametrize("kind", RB.KINDS, ids=[RB.KIND_NAMES[k] for k in RB.KINDS])
@pytest.mark.parametrize("method", [RB.GICP, RB.COLOUR], ids=["gicp", "colour"])
def test_row_bits_on_the_cloud_route_with_normals_and_colours(hip_lib, hip, room, method, kind):
    """Generalized ICP with a normal per source point and the colour method with a colour per point, on a ragged cut of the frame's cloud."""
    m = room["m"]
    valid = np.nonzero(np.isfinite(room["cloud"]).all(axis=1))[0]
    pick = valid[np.linspace(0, len(valid) - 1, 2085).astype(np.int64)]
    xyz, normals, rgb3 = (np.ascontiguousarray(room[k][pick]) for k in ("cloud", "normals", "colours"))
    delta = 0.03 if method == RB.GICP else DELTA[method]       # (seeded source normals make the weight nearly isotropic: the cost is near e.e)
    m.set_align_robust(method, kind, delta)
    try:
        if method == RB.GICP:
            ref = RB.RobustEvaluation(method, kind, delta, room["ref"], xyz, room["guess"], LEAF, R.DEFAULT_BOX, LEAF, order="device", normals=normals,
                                      layers=room["gicp_layers"])
            row, w = device_row(hip_lib, hip, m, method, room["guess"], len(xyz), xyz=xyz, normals=normals)
        else:
            ref = RB.RobustEvaluation(method, kind, delta, room["ref"], xyz, room["guess"], LEAF, R.DEFAULT_BOX, LEAF, order="device", rgb=rgb3,
                                      layers=room["colour_layers"])
            row, w = device_row(hip_lib, hip, m, method, room["guess"], len(xyz), xyz=xyz, rgb3=rgb3)
        assert ref.n > 300 and 0 < ref.n_downweighted <= ref.n
        check_row(row, w, ref, "%s %s cloud of 2085" % (METHOD_NAMES[method], RB.KIND_NAMES[kind]))
    finally:
        m.set_align_robust(method, "none")


ALIGN = {RB.POINT: "align_cloud", RB.PLANE: "align_cloud_plane"}


def check_alignment(m, run, ref):
    """The comparison of tests/test_map_align_plane_gpu.py's check_alignment, on the robust loop, and robust_info."""
    pose, res = run()
    trace, info = m.align_trace(), m.robust_info()
    print("status", res["status"], "iterations", res["iterations"], "converged", res["converged"], "contributing", [t[0] for t in trace], "restated",
          [t[0] for t in ref.trace], "margins", ref.margins, "pose difference", A.pose_error(pose, ref.pose), "info", info, "restated", ref.info)
    assert (res["status"], res["iterations"], res["converged"]) == (ref.status, ref.iterations, ref.converged)
    assert [t[0] for t in trace] == [t[0] for t in ref.trace]
    for (n, ss, u), (rn, rss, ru) in zip(trace, ref.trace):
        assert abs(ss - rss) <= 2e-6 * rss + 1e-12 and np.abs(u - ru).max() <= POSE_TOL
    dr, dt = A.pose_error(pose, ref.pose)
    assert dr <= POSE_TOL and dt <= POSE_TOL
    assert res["n_matched"] == ref.n_matched and abs(res["fitness"] - ref.fitness) <= 2e-6 * ref.fitness + 1e-15
    if "fitness_point" in res:
        assert abs(res["fitness_point"] - ref.fitness_point) <= 2e-6 * ref.fitness_point + 1e-15
    for k, v in ref.final.counters.items():
        assert res[k] == v, k
    assert np.abs(res["hessian"] - ref.hessian).max() <= 2e-5 * np.abs(ref.hessian).max()
    assert np.abs(res["gradient"] - ref.gradient).max() <= 2e-5 * max(np.abs(ref.gradient).max(), 1e-30) + 2e-6 * np.abs(ref.hessian).max() * 1e-3
    assert (info["method"], info["kind"], info["delta_eff"], info["n"], info["n_downweighted"]) == tuple(ref.info[k] for k in ("method", "kind", "delta_eff", "n", "n_downweighted"))
    assert abs(info["sum_w"] - ref.info["sum_w"]) <= 2e-6 * ref.info["sum_w"]
    pose2, res2 = run()       # the same bytes from run to run
    assert pose2.tobytes() == pose.tobytes() and all(np.array_equal(np.asarray(res[k]), np.asarray(res2[k])) for k in res) and m.robust_info() == info
    return pose, res


@pytest.mark.parametrize("kind", RB.KINDS, ids=[RB.KIND_NAMES[k] for k in RB.KINDS])
@pytest.mark.parametrize("method", [RB.POINT, RB.PLANE], ids=["point", "plane"])
def test_the_robust_loop_equals_the_restated_loop(corner, method, kind):
    """Two (point) and four (plane) steps from the trial's guess on its 7500 points: every restated stop decision is a factor of more than
    3 from eps (with more steps the point method's come within a factor 2)."""
    m, xyz = corner["m"], corner["clouds"][7500]
    iters = 2 if method == RB.POINT else 4
    ref = RB.RobustAlignment(method, kind, DELTA[method], corner["ref"], xyz, corner["guess"], LEAF, None, LEAF, max_iters=iters, order="device")
    assert ref.status == A.OK and ref.iterations == iters and all(mg >= 3.0 for mg in ref.margins)
    m.set_align_robust(method, kind, DELTA[method])
    try:
        check_alignment(m, lambda: getattr(m, ALIGN[method])(xyz, corner["guess"], max_iters=iters), ref)
    finally:
        m.set_align_robust(method, "none")


def test_the_trial_on_the_device(corner):
    """The six end errors per lift, asserted as on the CPU: every robust kind ends closer than quadratic in angle and distance,
    Geman-McClure <= Cauchy <= Huber in distance, Geman-McClure at most half the quadratic distance."""
    m = corner["m"]
    try:
        for lift, (target, cloud, P, guess, n_raised) in corner["lifts"].items():
            err = {}
            for kind in (RB.NONE,) + RB.KINDS:
                m.set_align_robust("plane", kind, 0.01)
                pose, res = m.align_cloud_plane(cloud, guess, max_iters=10)
                assert res["status"] == A.OK and m.robust_info()["kind"] == kind
                err[kind] = A.pose_error(pose, P)
            assert_trial(err, lift)
    finally:
        m.set_align_robust("plane", "none")


class _Settable:
    """tools/map_align_bits.py's VoxelMap with a robust setting applied to every map it makes."""

    def __init__(self, setter):
        from rgbd360_amd.voxel_map import VoxelMap
        self.setter, self.VoxelMap = setter, VoxelMap

    def __call__(self, *a, **kw):
        m = self.VoxelMap(*a, **kw)
        self.setter(m)
        return m


def test_none_is_the_quadratic_call_byte_for_byte(reg, hip_lib, monkeypatch):
    """After set(kind = NONE), and after a robust setting was set and reset, every case of tests/golden/map_align_bits.json still matches."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_align_bits as recorder
    with open(recorder.OUT) as f:
        want = json.load(f)["cases"]

    def none(m):
        for method in range(4):
            m.set_align_robust(method, "none", 123.0, True)

    def set_then_reset(m):
        for method in range(4):
            m.set_align_robust(method, "cauchy", 0.01)
        m.align_cloud_plane(np.zeros((3, 3), F) + 0.5, EYE)        # (a robust call in between)
        for method in range(4):
            m.set_align_robust(method, "none")

    for setter in (none, set_then_reset):
        monkeypatch.setattr(recorder, "VoxelMap", _Settable(setter))
        got = recorder.compute(reg)
        assert sorted(got) == sorted(want) and len(want) == 54
        differ = [(case, part, field) for case in want for part in ("eval", "align") for field in set(want[case][part]) | set(got[case][part])
                  if want[case][part].get(field) != got[case][part].get(field)]
        assert not differ, differ[:10]


def quadratic_sums(hip_lib, hip, room, method):
    """The quadratic evaluation entry of `method` on the room's frame: its sums."""
    from rgbd360_amd.register import pose_to_cm
    m, d = room["m"], room["depth"]
    n_sums, n_counters = RB.N_SUMS[method], 3 + len(RB.COUNTERS[method])
    sums, counters = np.zeros(n_sums), np.zeros(n_counters, np.int64)
    p = method_params(m, method)
    image = (vp(d), d.strides[0], 0, d.shape[0], d.shape[1], 2)
    cm = vp(pose_to_cm(room["guess"]))
    if method == RB.POINT:
        rc = hip_lib.rgbd360_map_align_eval(m._handle(), *image, None, 0, cm, 0, C.byref(p), vp(sums), vp(counters), None, None, 0, None, None)
    elif method == RB.PLANE:
        rc = hip_lib.rgbd360_map_align_plane_eval(m._handle(), *image, None, 0, cm, 0, C.byref(p), vp(sums), vp(counters), None, None, None, None)
    elif method == RB.GICP:
        rc = hip_lib.rgbd360_map_align_gicp_eval(m._handle(), *image, None, None, 0, cm, 0, C.byref(p), vp(sums), vp(counters), None, None, None, None)
    else:
        rc = hip_lib.rgbd360_map_align_colour_eval(m._handle(), vp(room["rgb"]), room["rgb"].strides[0], *image, None, None, 0, cm, 0, C.byref(p), vp(sums),
                                                   vp(counters), None, None, None, None)
    assert rc == 0
    return sums, counters


SPHERE = {RB.POINT: "align_sphere", RB.PLANE: "align_sphere_plane", RB.GICP: "align_sphere_gicp", RB.COLOUR: "align_sphere_colour"}


@pytest.mark.parametrize("method", [RB.POINT, RB.PLANE, RB.GICP, RB.COLOUR], ids=["point", "plane", "gicp", "colour"])
def test_huber_with_a_large_delta_is_the_quadratic_call_on_the_device(hip_lib, hip, room, method):
    """delta above the square root of every cost term (max_dist^2 / epsilon bounds generalized ICP's, max_dist^2 + 1 the colour method's):
    w = 1.0, so the weighted words, sum rho, the counters, the pose, the result and the trace are the quadratic call's bytes."""
    m, d = room["m"], room["depth"]
    big = {RB.POINT: 0.11, RB.PLANE: 0.11, RB.GICP: 4.0, RB.COLOUR: 2.0}[method]
    head = (room["rgb"], d) if method == RB.COLOUR else (d,)
    sums, counters = quadratic_sums(hip_lib, hip, room, method)
    pose_q, res_q = getattr(m, SPHERE[method])(*head, room["guess"], convention=2)
    trace_q, info_q = m.align_trace(), m.robust_info()
    assert info_q == dict(method=method, kind=0, delta_eff=0.0, sum_w=float(res_q["n_matched"]), n=res_q["n_matched"], n_downweighted=0)
    m.set_align_robust(method, "huber", big)
    try:
        colour = method == RB.COLOUR
        row, w = device_row(hip_lib, hip, m, method, room["guess"], d.size, depth=d, depth_step=d.strides[0], shape=d.shape,
                            rgb=room["rgb"] if colour else None, rgb_step=room["rgb"].strides[0] if colour else 0)
        assert row[:len(sums)].tobytes() == sums.tobytes() and row[len(sums):len(sums) + len(counters)].tolist() == counters.tolist()
        words = RB.WORDS[method]
        assert row[words] == sums[0] and row[words + 1] == 0 and set(np.unique(w)) <= {0.0, 1.0} and w.sum() == sums[0]
        pose_r, res_r = getattr(m, SPHERE[method])(*head, room["guess"], convention=2)
        trace_r, info_r = m.align_trace(), m.robust_info()
    finally:
        m.set_align_robust(method, "none")
    assert res_q["iterations"] >= 2 and pose_r.tobytes() == pose_q.tobytes()
    assert all(np.asarray(res_q[k]).tobytes() == np.asarray(res_r[k]).tobytes() for k in res_q)
    assert len(trace_q) == len(trace_r) and all(a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() for a, b in zip(trace_q, trace_r))
    assert info_r == dict(info_q, kind=RB.HUBER, delta_eff=big)


@pytest.mark.parametrize("method", ["point", "plane"])
def test_a_batch_is_the_single_robust_calls(corner, method):
    """Nine jobs over the five clouds under Cauchy: pose, result, trace and robust info of every job are the single robust call's bytes,
    also permuted and with a job repeated."""
    m, clouds = corner["m"], [corner["clouds"][n] for n in CLOUD_SIZES]
    code = RB.POINT if method == "point" else RB.PLANE
    guesses = [corner["guess"], A.perturbed(corner["P"], 0.01, 0.002, 3)]
    jobs = [(i, guesses[j % 2]) for j, i in enumerate((0, 1, 2, 3, 4, 4, 3, 2, 1))]
    m.set_align_robust(code, "cauchy", DELTA[code])
    try:
        single = {}
        for j, (i, g) in enumerate(jobs):
            pose, res = getattr(m, ALIGN[code])(clouds[i], g, max_iters=3)
            single[j] = (pose, res, m.align_trace(), m.robust_info())
        assert sum(s[1]["status"] == A.OK for s in single.values()) >= 7 and single[4][3]["n_downweighted"] > 0
        for order in (list(range(9)), [8, 3, 5, 0, 7, 1, 6, 2, 4], [4, 4, 0, 7]):
            poses, results = m.align_batch_cloud(clouds, [jobs[j] for j in order], method=method, max_iters=3)
            for k, j in enumerate(order):
                pose, res, trace, info = single[j]
                assert poses[k].tobytes() == pose.tobytes(), (order, k)
                assert all(np.asarray(res[f]).tobytes() == np.asarray(results[k][f]).tobytes() for f in res), (order, k)
                bt = m.align_batch_trace(k)
                assert len(bt) == len(trace) and all(a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() for a, b in zip(bt, trace))
                assert m.robust_info(k) == info, (order, k, m.robust_info(k), info)
        with pytest.raises(Exception):
            m.robust_info(4)        # (the last batch had four jobs)
    finally:
        m.set_align_robust(code, "none")


@pytest.mark.parametrize("scale", [True, False], ids=["scaled", "unscaled"])
@pytest.mark.parametrize("kind", ["point", "plane"])
def test_coarse_to_fine_levels_are_the_single_level_robust_calls(corner, kind, scale):
    """top_shift 2: level s of the chain is the single-level robust call on the level's handle from the pose handed on, with delta 2^s
    (scale_with_level) or delta set on the root; the root reports the finest level."""
    m, xyz = corner["m"], corner["clouds"][7500]
    code = RB.POINT if kind == "point" else RB.PLANE
    delta = DELTA[code]
    try:
        m.set_align_robust(code, "cauchy", delta, scale_with_level=scale)
        assert m.align_robust(code) == dict(kind=RB.CAUCHY, scale_with_level=int(scale), delta=delta)
        pose, res = m.align_cloud_c2f(xyz, corner["guess"], top_shift=2, kind=kind, max_iters=3)
        info = m.robust_info()
        assert res["n_levels"] == 3 and [lv["shift"] for lv in res["levels"]] == [2, 1, 0]
        handed = corner["guess"]
        for lv in res["levels"]:
            s = lv["shift"]
            eff = delta * 2.0 ** s if scale else delta
            m.set_align_robust(code, "cauchy", eff)
            view = m if s == 0 else m.level(s)
            if s:
                assert view.align_robust(code)["delta"] == eff
                with pytest.raises(Exception):
                    view.set_align_robust(code, "huber", 1.0)
            lp, lr = getattr(view, ALIGN[code])(xyz, handed, max_iters=3)
            assert lp.tobytes() == lv["pose"].tobytes(), s
            assert all(np.asarray(lr[f]).tobytes() == np.asarray(lv[f]).tobytes() for f in ("status", "iterations", "converged", "n_valid", "n_matched", "fitness")), s
            assert view.robust_info()["delta_eff"] == eff and view.robust_info()["n"] == lv["n_matched"]
            if s == 0:
                assert m.robust_info() == info and lp.tobytes() == pose.tobytes()
                assert lr["hessian"].tobytes() == res["hessian"].tobytes()
            if lv["status"] == A.OK:
                handed = lv["pose"]
        assert res["levels"][-1]["n_matched"] > 1000 and info["delta_eff"] == delta and info["n_downweighted"] > 0
    finally:
        m.set_align_robust(code, "none")


def test_the_setting_writes_nothing(reg, corner):
    """The map's records and its census are unchanged by set / get and by robust alignments."""
    xyz = corner["clouds"][2085]
    with new_map(reg, box=None) as m:
        m.insert_cloud(PL.corner_scene(101, step=0.02), None, EYE)
        before, census = m.extract(), m.census()
        for method, kind in ((0, "huber"), (1, "cauchy"), (2, "geman_mcclure"), (3, "huber")):
            m.set_align_robust(method, kind, 0.02)
            assert m.align_robust(method)["kind"] == RB.HUBER + ("huber", "cauchy", "geman_mcclure").index(kind)
        m.align_cloud(xyz, corner["guess"])
        m.align_cloud_plane(xyz, corner["guess"])
        m.align_cloud_gicp(xyz, corner["guess"])
        assert m.robust_info()["method"] == RB.GICP and m.robust_info()["kind"] == RB.GEMAN_MCCLURE
        after = m.extract()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and m.census() == census


def test_refusals_leave_outputs_and_the_setting_untouched(hip_lib, hip, corner):
    from rgbd360_amd import _lib
    m = corner["m"]
    H = m._handle()
    m.set_align_robust("plane", "cauchy", 0.02, scale_with_level=True)
    try:
        keep = m.align_robust("plane")

        def refused(method, kind, delta):
            r = _lib.MapRobust(kind, 0, delta)
            rc = hip_lib.rgbd360_map_set_align_robust(H, method, C.byref(r))
            return rc == -1 and hip_lib.rgbd360_map_last_error(H) != b"" and m.align_robust("plane") == keep

        assert refused(1, -1, 0.01) and refused(1, 4, 0.01) and refused(-1, 1, 0.01) and refused(4, 1, 0.01)
        for bad in (0.0, -0.01, float("nan"), float("inf")):
            assert refused(1, 1, bad) and refused(1, 3, bad)
        assert hip_lib.rgbd360_map_set_align_robust(H, 1, None) == -1 and m.align_robust("plane") == keep
        r = _lib.MapRobust(7, 7, 7.0)
        assert hip_lib.rgbd360_map_get_align_robust(H, 4, C.byref(r)) == -1 and hip_lib.rgbd360_map_get_align_robust(H, 1, None) == -1
        assert (r.kind, r.scale_with_level, r.delta) == (7, 7, 7.0)
        # NONE takes any delta
        r = _lib.MapRobust(0, 0, float("nan"))
        assert hip_lib.rgbd360_map_set_align_robust(H, 0, C.byref(r)) == 0 and m.align_robust("point")["kind"] == 0
        # a level follows its root and refuses a setting of its own
        lv = m.level(1)
        assert lv.align_robust("plane") == keep
        r = _lib.MapRobust(1, 0, 0.5)
        assert hip_lib.rgbd360_map_set_align_robust(lv._handle(), 1, C.byref(r)) == -1 and lv.align_robust("plane") == keep and m.align_robust("plane") == keep
        # the evaluation entry: an unknown method, a method without a robust kernel, a NULL pose, a bad parameter
        xyz = corner["clouds"][1025]
        for method, kw, pose in ((7, {}, corner["guess"]), (0, {}, corner["guess"]), (1, dict(max_dist=0.0), corner["guess"])):
            code = method if method < 4 else 1
            from rgbd360_amd.register import pose_to_cm
            row, wd = np.full(40, 7.0), to_device(hip, np.full(len(xyz), 9.0))
            p = method_params(m, code, **kw)
            rc = hip_lib.rgbd360_map_align_robust_eval(H, method, None, 0, None, 0, 0, 0, 0, 2, vp(xyz), None, None, len(xyz), vp(pose_to_cm(pose)), 0, C.byref(p),
                                                       vp(row), wd)
            back = np.zeros(len(xyz))
            assert hip.hipMemcpy(vp(back), wd, back.nbytes, 2) == 0
            hip.hipFree(wd)
            assert rc == -1 and (row == 7.0).all() and (back == 9.0).all() and hip_lib.rgbd360_map_last_error(H) != b"", method
        info = _lib.MapRobustInfo(7, 7, 7.0, 7.0, 7, 7)
        assert hip_lib.rgbd360_map_align_batch_robust_info(H, 10 ** 6, C.byref(info)) == -1 and hip_lib.rgbd360_map_align_robust_info(H, None) == -1
        assert (info.method, info.n) == (7, 7)
    finally:
        m.set_align_robust("plane", "none")


def test_the_rig_calibration_does_not_see_the_setting(corner):
    """rgbd360_map_calibrate_rig_clouds keeps the quadratic kernels: the same bytes with and without a robust setting on the plane method."""
    m, xyz = corner["m"], corner["clouds"][7500]
    clouds = [[xyz[0::2], xyz[1::2]], [xyz[0::3], xyz[1::3]]]
    poses, ext = [corner["guess"], corner["P"]], [EYE, A.perturbed(EYE, 0.005, 0.002, 2)]

    def run():
        T, E, res = m.calibrate_rig_clouds(clouds, poses, ext, max_iters=3)
        sensors = res.pop("sensors")
        return T.tobytes() + E.tobytes() + repr(sorted(res.items())).encode() + b"".join(s["hessian"].tobytes() + s["gradient"].tobytes() for s in sensors)

    plain = run()
    m.set_align_robust("plane", "geman_mcclure", 0.01)
    try:
        assert run() == plain
    finally:
        m.set_align_robust("plane", "none")
    assert run() == plain

