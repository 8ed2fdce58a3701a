"""The rig calibration against the voxel map (rgbd360_map_calibrate_rig_*, csrc/rig_calib.h) on the device: the kernels' solve against
the host build of the same text byte for byte on the cases of tests/test_rig_calib_cpu.py; the whole call on that file's scenario against
the restatement (tests/rig_calib_reference.py) within the point-to-plane device / restatement pose bound, statuses and step counts equal;
reruns, host and device inputs, sensors that do not depend on each other, tile edges, max_iters 0, a level map, the map untouched, the
pinhole depth entry against the cloud entry on numpy-formed points byte for byte, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import map_align_plane_reference as PL
import map_align_reference as A
import map_input_forms as MF
import rig_calib_reference as RC
import test_rig_calib_cpu as CPU

pytestmark = pytest.mark.gpu

F = np.float32
EYE = np.eye(4, dtype=F)
POSE_TOL = CPU.POSE_TOL
OK, ILL_POSED, NO_VALID_PIXELS = A.OK, A.ILL_POSED, A.NO_VALID_PIXELS


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip():
    return MF.hip_runtime()


@pytest.fixture(scope="module")
def cube_map(reg):
    """The scene's cube in a map of leaf 0.1 (no box), and in one of leaf 0.05 for its level 1; a calibration never changes a map."""
    from rgbd360_amd.voxel_map import VoxelMap
    sc = RC.scene()
    maps = {}
    for leaf in (0.1, 0.05):
        m = VoxelMap(reg, leaf, 1 << 16)
        m.set_box(None, None)
        m.insert_cloud(np.ascontiguousarray(sc["map_cloud"]), None, EYE)
        maps[leaf] = m
    yield maps
    for m in maps.values():
        m.close()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pose_max(a, b):
    errs = [A.pose_error(x, y) for x, y in zip(a, b)]
    return max(e[0] for e in errs), max(e[1] for e in errs)


class Call:
    """One rgbd360_map_calibrate_rig_clouds call: rc, T, E, the result and sensor structs and everything as bytes."""

    def __init__(self, L, m, clouds, T, E, on_device=0, addresses=None, depth=None, **kw):
        from rgbd360_amd import _lib
        K, S = len(T), len(E)
        self.p = m.rig_calib_params(**kw)
        Tc, Ec = CPU.cm(T), CPU.cm(E)
        self.res = _lib.RigCalibResult()
        self.res.status = -77
        self.sen = (_lib.RigCalibSensor * S)()
        if depth is None:
            xs = [np.ascontiguousarray(x, F).reshape(-1, 3) for x in clouds]
            I = (_lib.MapBatchCloud * len(xs))()
            for k, x in enumerate(xs):
                I[k].xyz, I[k].n = (addresses[k] if addresses else x.ctypes.data), len(x)
            self.rc = L.rgbd360_map_calibrate_rig_clouds(m._handle(), I, K, S, on_device, vp(Tc), vp(Ec), C.byref(self.p), C.byref(self.res), self.sen)
        else:
            frames, depth_type, rows, cols, pin = depth
            I = (_lib.MapBatchFrame * len(frames))()
            for k, (addr, step) in enumerate(frames):
                I[k].depth, I[k].depth_step = addr, step
            self.rc = L.rgbd360_map_calibrate_rig_depth(m._handle(), I, depth_type, rows, cols, *[C.c_float(v) for v in pin], K, S, on_device, vp(Tc), vp(Ec),
                                                        C.byref(self.p), C.byref(self.res), self.sen)
        self.err = L.rgbd360_map_last_error(m._handle())
        self.T, self.E = np.transpose(Tc, (0, 2, 1)), np.transpose(Ec, (0, 2, 1))
        self.bytes = (self.rc, Tc.tobytes(), Ec.tobytes(), bytes(self.res), bytes(self.sen))


def scene_call(L, m, joint, **kw):
    sc = RC.scene()
    T0, E0, refine, fixed = RC.start(joint)
    kw = dict(dict(max_iters=10, eps=0.0, refine_poses=refine, fixed_sensor=fixed, max_flatness=RC.MAX_FLATNESS), **kw)
    return Call(L, m, sc["clouds"], T0, E0, **kw)


# ---- the solve alone
SOLVE_CASES = CPU.CASES + ("wall", "singular", "too_few")


@pytest.mark.parametrize("name", SOLVE_CASES)
def test_device_solve_equals_host_solve_byte_for_byte(hip_lib, cube_map, name):
    L, m = hip_lib, cube_map[0.1]
    if name == "wall":
        rows, T, E, kw = RC.wall_case()
    elif name == "singular":
        rows, T, E, kw = RC.singular_rows()
    elif name == "too_few":
        rows, T, E, kw = RC.solve_cases()["extrinsics"]
        kw = dict(kw, min_matches=int(rows[:, 0].sum()) + 1)
    else:
        rows, T, E, kw = RC.solve_cases()[name]
    host = CPU.run_solve(L.rgbd360_rig_calib_solve_host, (), rows, T, E, kw)
    dev = CPU.run_solve(L.rgbd360_rig_calib_solve_dev, (m._handle(),), rows, T, E, kw)
    assert host[0] == dev[0] == 0 and host[1] == dev[1]
    assert host[1] == {"wall": ILL_POSED, "singular": ILL_POSED, "too_few": NO_VALID_PIXELS}.get(name, OK)
    for h, d in zip(host[2:], dev[2:]):
        assert h.tobytes() == d.tobytes()
    # again: nothing is left behind by the call before
    again = CPU.run_solve(L.rgbd360_rig_calib_solve_dev, (m._handle(),), rows, T, E, kw)
    assert all(a.tobytes() == d.tobytes() for a, d in zip(again[2:], dev[2:]))


# ---- the whole call
@pytest.mark.parametrize("joint", (0, 1))
def test_the_scenario_against_the_restatement(hip_lib, cube_map, joint):
    L, m = hip_lib, cube_map[0.1]
    sc = RC.scene()
    ref = CPU.scenario(joint)
    before = m.records()
    got = scene_call(L, m, joint)
    assert np.array_equal(m.records(), before) and len(before) > 1000          # the map is untouched
    dr_e, dt_e = pose_max(got.E, ref.E)
    dr_t, dt_t = pose_max(got.T, ref.T)
    print("joint", joint, "device against restatement: extrinsics", dr_e, dt_e, "poses", dr_t, dt_t, "| status", got.rc, "steps", got.res.iterations,
          "| to the truth: extrinsics", RC.largest_translation_error(got.E, sc["E"]), "poses", RC.largest_translation_error(got.T, sc["T"]))
    assert got.rc == got.res.status == ref.status == OK
    assert (got.res.iterations, got.res.converged) == (ref.iterations, ref.converged)
    assert max(dr_e, dt_e, dr_t, dt_t) <= POSE_TOL
    assert (got.res.n_matched, got.res.n_inputs_used, got.res.n_frames_skipped) == (ref.n_matched, ref.n_inputs_used, ref.n_frames_skipped)
    assert abs(got.res.cost - ref.cost) <= 1e-5 * ref.cost and abs(got.res.fitness - ref.fitness) <= 1e-5 * ref.fitness
    assert sum(s.n_matched for s in got.sen) == got.res.n_matched
    tr = m.rig_calib_trace()
    assert len(tr) == ref.iterations and tr[0][0] == ref.trace[0][0]
    if not joint:
        assert got.T.tobytes() == RC.start(0)[0].tobytes()
    # the rerun is identical
    assert scene_call(L, m, joint).bytes == got.bytes


def test_host_and_device_inputs_give_identical_results(hip_lib, hip, cube_map):
    L, m = hip_lib, cube_map[0.1]
    sc = RC.scene()
    host = scene_call(L, m, 1, max_iters=3)
    T0, E0, refine, fixed = RC.start(1)
    dev = []
    try:
        addrs = []
        for x in sc["clouds"]:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), x.nbytes) == 0 and hip.hipMemcpy(p, vp(x), x.nbytes, 1) == 0
            dev.append(p)
            addrs.append(p.value)
        got = Call(L, m, sc["clouds"], T0, E0, on_device=1, addresses=addrs, max_iters=3, eps=0.0, refine_poses=refine, fixed_sensor=fixed,
                   max_flatness=RC.MAX_FLATNESS)
    finally:
        for p in dev:
            hip.hipFree(p)
    assert host.rc == OK and got.bytes == host.bytes


def test_a_sensor_does_not_depend_on_the_others(hip_lib, cube_map):
    """Extrinsics only: M is block diagonal, a sensor's bytes are those of any call it takes part in (eps 0: the stop test is the call's)."""
    L, m = hip_lib, cube_map[0.1]
    sc = RC.scene()
    T0, E0, _, _ = RC.start(0)
    S, K = RC.N_SENSORS, RC.N_FRAMES
    kw = dict(max_iters=3, eps=0.0, max_flatness=RC.MAX_FLATNESS)
    full = Call(L, m, sc["clouds"], T0, E0, **kw)
    assert full.rc == OK
    for pick in ((2,), (0, 2), (3, 1, 0, 2)):
        clouds = [sc["clouds"][k * S + s] for k in range(K) for s in pick]
        part = Call(L, m, clouds, T0, E0[list(pick)], **kw)
        assert part.rc == OK
        for i, s in enumerate(pick):
            assert part.E[i].tobytes() == full.E[s].tobytes(), (pick, s)
            assert bytes(part.sen[i]) == bytes(full.sen[s]), (pick, s)


def test_tile_edges_and_small_inputs(hip_lib, cube_map):
    """Clouds of 1, 1023 and 1025 points (the tile has 1024) next to whole ones; the one-point input is below min_input_matches."""
    L, m = hip_lib, cube_map[0.1]
    sc = RC.scene()
    S = RC.N_SENSORS
    T0, E0, _, _ = RC.start(0)
    clouds = [np.ascontiguousarray(x) for x in sc["clouds"]]
    thin = lambda x, n: np.ascontiguousarray(x[np.linspace(0, len(x) - 1, n).astype(int)])      # (evenly: every wall the sensor sees stays)
    clouds[0], clouds[1], clouds[2] = clouds[0][:1], thin(clouds[1], 1023), thin(clouds[2], 1025)
    assert [len(c) for c in clouds[:3]] == [1, 1023, 1025]
    ref = RC.RigCalibration(sc["target"], clouds, T0, E0, RC.LEAF, RC.LEAF, max_iters=2, eps=0.0, **RC.plane_kw())
    got = Call(L, m, clouds, T0, E0, max_iters=2, eps=0.0, max_flatness=RC.MAX_FLATNESS)
    assert got.rc == ref.status == OK and got.res.iterations == ref.iterations == 2
    assert (got.res.n_matched, got.res.n_inputs_used) == (ref.n_matched, ref.n_inputs_used) and ref.n_inputs_used == RC.N_FRAMES * S - 1
    assert max(pose_max(got.E, ref.E)) <= POSE_TOL


def test_max_iters_zero_is_the_final_evaluation(hip_lib, cube_map):
    L, m = hip_lib, cube_map[0.1]
    sc = RC.scene()
    T0, E0, refine, fixed = RC.start(1)
    got = scene_call(L, m, 1, max_iters=0)
    rows = RC.solve_cases()["joint"][0]
    assert got.rc == OK and got.res.iterations == 0 and got.res.converged == 0
    assert got.T.tobytes() == T0.tobytes() and got.E.tobytes() == E0.tobytes()
    assert got.res.n_matched == int(rows[:, 0].sum()) and abs(got.res.cost - rows[:, 28].sum()) <= 1e-6 * rows[:, 28].sum()
    assert m.rig_calib_trace() == []
    # the per-sensor records are G_s and its gradient of that evaluation
    ref = RC.Solve(rows, T0, E0, refine=0, fixed=-1)
    for s in range(RC.N_SENSORS):
        G = np.zeros((6, 6))
        for k in range(RC.N_FRAMES):
            G += np.array(ref.inputs[k][s].G)
        H = np.array(got.sen[s].hessian, F).reshape(6, 6).T
        assert np.abs(H - G).max() <= 1e-5 * np.abs(G).max()


def test_a_level_map_is_accepted(hip_lib, cube_map):
    L = hip_lib
    sc = RC.scene()
    lv = cube_map[0.05].level(1)
    T0, E0, _, _ = RC.start(0)
    got = scene_call(L, lv, 0)
    e0, e1 = RC.largest_translation_error(E0, sc["E"]), RC.largest_translation_error(got.E, sc["E"])
    print("level 1 of the 0.05 map:", e0, "->", e1)
    assert got.rc == OK and got.res.iterations == 10 and e1 <= 0.25 * e0


def test_one_frame_one_sensor_is_the_single_alignment(hip_lib, cube_map):
    L, m = hip_lib, cube_map[0.1]
    x, g, pa, rc = CPU.single()
    got = Call(L, m, [x], EYE[None], g[None], max_iters=10, eps=0.0, max_flatness=RC.MAX_FLATNESS)
    dr, dt = A.pose_error(got.E[0], pa.pose)
    print("K = S = 1 on the device against PlaneAlignment:", dr, dt)
    assert got.rc == OK
    assert dr <= POSE_TOL + 1.5 * CPU.MEASURED_SINGLE_GAP[0] and dt <= POSE_TOL + 1.5 * CPU.MEASURED_SINGLE_GAP[1]


# ---- the pinhole depth entry
def cast_depth(P, rows, cols, pin):
    """The z of every pixel's ray f = ((u - cx) / fx, (v - cy) / fy, 1) from pose P (inside the cube [0, 2]^3) to the cube's walls, float64."""
    fx, fy, cx, cy = pin
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    f = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, float)], axis=-1)
    d = f @ P[:3, :3].astype(float).T
    o = P[:3, 3].astype(float)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (2.0 - o) / d, np.where(d < 0, (0.0 - o) / d, np.inf))
    return t.min(axis=-1)


def numpy_cloud(z, pin):
    """The points rgbd360_map_calibrate_rig_depth forms, in float32 with every operation rounded on its own; NaN triples without a measurement."""
    fx, fy, cx, cy = (F(v) for v in pin)
    rows, cols = z.shape
    v, u = np.meshgrid(np.arange(rows, dtype=F), np.arange(cols, dtype=F), indexing="ij")
    f0, f1 = (u - cx) / fx, (v - cy) / fy
    ok = np.isfinite(z) & (z > 0)
    with np.errstate(invalid="ignore"):
        pts = np.stack([z * f0, z * f1, z], axis=-1).astype(F)
    pts[~ok] = np.nan
    return np.ascontiguousarray(pts.reshape(-1, 3))


@pytest.mark.parametrize("dtype", ("uint16", "float32"))
@pytest.mark.parametrize("size", ((6, 8), (45, 66), (48, 64)))
def test_depth_images_against_numpy_formed_clouds(hip_lib, hip, cube_map, size, dtype):
    L, m = hip_lib, cube_map[0.1]
    sc = RC.scene()
    rows, cols = size
    K, S = 2, 2
    pin = (0.7 * cols, 0.7 * cols, (cols - 1) / 2.0 + 0.25, (rows - 1) / 2.0)
    T, E = sc["T"][:K], sc["E"][:S]
    E0 = np.stack([A.perturbed(E[s], 0.01, 0.005, 40 + s) for s in range(S)])
    images = []
    for k in range(K):
        for s in range(S):
            z = cast_depth(T[k].astype(float) @ E[s].astype(float), rows, cols, pin)
            if dtype == "uint16":
                img = np.round(z * 1000.0).astype(np.uint16)
                img[0, 0] = img[rows // 2, cols // 3] = 0
            else:
                img = z.astype(F)
                img[0, 0], img[rows // 2, cols // 3], img[rows - 1, cols - 1], img[1, 2] = 0.0, np.nan, -1.5, np.inf
            images.append(img)
    metres = [(F(0.001) * img.astype(F)).astype(F) if dtype == "uint16" else img for img in images]
    kw = dict(max_iters=3, eps=0.0, max_flatness=RC.MAX_FLATNESS, min_input_matches=1)
    want = Call(L, m, [numpy_cloud(z, pin) for z in metres], T, E0, **kw)
    assert want.rc == OK and want.res.n_matched > 0.5 * K * S * rows * cols and want.res.iterations == 3
    depth_type = 0 if dtype == "uint16" else 1
    padded = [MF.padded_rows(img, 12) for img in images]
    dev = []

    def device(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, vp(a), a.nbytes, 1) == 0
        dev.append(p)
        return p.value

    try:
        forms = {"host": (0, [(img.ctypes.data, img.strides[0]) for img in images]),
                 "host, padded rows": (0, [(b.ctypes.data, b.shape[1]) for b in padded]),
                 "device": (1, [(device(img), img.strides[0]) for img in images]),
                 "device, padded rows": (1, [(device(b), b.shape[1]) for b in padded])}
        for name, (on_device, frames) in forms.items():
            got = Call(L, m, None, T, E0, on_device=on_device, depth=(frames, depth_type, rows, cols, pin), **kw)
            assert got.bytes == want.bytes, (name, got.rc, got.err)
    finally:
        for p in dev:
            hip.hipFree(p)


# ---- refusals
def test_refusals(hip_lib, cube_map):
    from rgbd360_amd import _lib
    L, m = hip_lib, cube_map[0.1]
    H = m._handle()
    sc = RC.scene()
    S = RC.N_SENSORS
    T0, E0, _, _ = RC.start(0)
    clouds = [np.ascontiguousarray(x) for x in sc["clouds"][:2 * S]]
    T0 = T0[:2]
    assert Call(L, m, clouds, T0, E0, max_iters=1, max_flatness=RC.MAX_FLATNESS).rc == OK

    def refused(call, why):
        assert call.rc == -1 and call.err, why
        assert call.res.status == -77 and not any(s.n_matched or s.cost for s in call.sen), why          # the outputs are untouched
        return call

    for kw in (dict(refine_poses=1), dict(refine_poses=1, fixed_sensor=-1), dict(fixed_sensor=S), dict(fixed_sensor=-2), dict(refine_poses=2, fixed_sensor=0),
               dict(lambda_=-0.5), dict(lambda_=float("nan")), dict(lambda_=float("inf")), dict(min_input_matches=0),
               dict(max_dist=0.2), dict(max_dist=0.0), dict(max_iters=-1), dict(max_iters=1001), dict(min_count=0), dict(eps=-1.0), dict(min_support=0),
               dict(min_support=28), dict(max_flatness=-1.0)):
        c = refused(Call(L, m, clouds, T0, E0, **kw), kw)
        assert c.T.tobytes() == T0.tobytes() and c.E.tobytes() == E0.tobytes()
    for bad in (np.nan, np.inf):
        Tb, Eb = T0.copy(), E0.copy()
        Tb[1, 2, 3] = bad
        Eb[3, 0, 0] = bad
        refused(Call(L, m, clouds, Tb, E0), "a pose that is not finite")
        refused(Call(L, m, clouds, T0, Eb), "an extrinsic that is not finite")
    # the counts
    big_E = np.stack([EYE] * 17)
    refused(Call(L, m, clouds[:2] * 17, T0, big_E), "17 sensors")
    many_T = np.stack([EYE] * 513)
    refused(Call(L, m, [clouds[0][:0]] * 1026, many_T, E0[:2]), "K S above RGBD360_MAP_BATCH_MAX")
    p = m.rig_calib_params()
    res = _lib.RigCalibResult()
    I = (_lib.MapBatchCloud * (2 * S))()
    for k, x in enumerate(clouds):
        I[k].xyz, I[k].n = x.ctypes.data, len(x)
    Tc, Ec = CPU.cm(T0), CPU.cm(E0)
    entry = L.rgbd360_map_calibrate_rig_clouds
    for args in ((None, 2, S, 0, vp(Tc), vp(Ec)), (I, 2, S, 0, None, vp(Ec)), (I, 2, S, 0, vp(Tc), None), (I, 0, S, 0, vp(Tc), vp(Ec)), (I, 2, 0, 0, vp(Tc), vp(Ec)),
                 (I, -1, S, 0, vp(Tc), vp(Ec))):
        assert entry(H, *args, C.byref(p), C.byref(res), None) == -1 and L.rgbd360_map_last_error(H), args
    # what the batch refuses of an input: a bad count, NULL points, too many workgroups, too many bytes to upload (nothing is read or launched)
    fake = clouds[0].ctypes.data
    for n, on_device, addr in ((-1, 0, fake), (5, 0, None), (1 << 40, 0, fake), (1024 * (1 << 20) + 1, 1, fake), (90_000_000, 0, fake)):
        J = (_lib.MapBatchCloud * (2 * S))()
        for k, x in enumerate(clouds):
            J[k].xyz, J[k].n = x.ctypes.data, len(x)
        J[5].xyz, J[5].n = addr, n
        assert entry(H, J, 2, S, on_device, vp(Tc), vp(Ec), C.byref(p), C.byref(res), None) == -1 and L.rgbd360_map_last_error(H), n
    assert Tc.tobytes() == CPU.cm(T0).tobytes() and Ec.tobytes() == CPU.cm(E0).tobytes()
    # the depth entry's own
    img = np.full((6, 8), 1000, np.uint16)
    frames = [(img.ctypes.data, img.strides[0])] * (2 * S)
    good = (4.0, 4.0, 3.5, 2.5)
    assert Call(L, m, None, T0, E0, depth=(frames, 0, 6, 8, good), max_iters=0).rc >= 0
    for depth in ((frames, 0, 6, 8, (0.0, 4.0, 3.5, 2.5)), (frames, 0, 6, 8, (4.0, 0.0, 3.5, 2.5)), (frames, 0, 6, 8, (4.0, 4.0, np.nan, 2.5)),
                  (frames, 0, 6, 8, (4.0, 4.0, 3.5, np.inf)), (frames, 2, 6, 8, good), (frames, 0, -1, 8, good),
                  ([(img.ctypes.data, 15)] * (2 * S), 0, 6, 8, good), ([(None, 16)] * (2 * S), 0, 6, 8, good)):
        refused(Call(L, m, None, T0, E0, depth=depth), depth[1:])
    refused(Call(L, m, None, T0, E0, depth=(frames, 0, 6, 8, good), refine_poses=1), "the gauge, through the depth entry")
