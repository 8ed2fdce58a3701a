"""Many alignments against the voxel map in lock step (rgbd360_map_align_batch_* / rgbd360_map_align_plane_batch_*,
csrc/map_align_batch.h) on the device.  The definition is the single call: per job the pose, the whole result struct and the trace are
compared BYTE FOR BYTE with rgbd360_map_align_cloud / _sphere (their _plane forms) of the job's input from the job's guess -- over inputs
of 1 to 5 tiles, ragged tiles, jobs that end at different steps or not at all, inputs in host memory, device memory and with padded
rows, permuted, single and repeated jobs, a level of the pyramid -- then the refusals and the multi-start scenario of
tests/test_map_align_batch_cpu.py end to end.  The helpers repeat those of tests/test_map_align_plane_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import map_align_plane_reference as PL
import map_align_reference as A
import map_input_forms as F
import voxel_map_reference as R

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)
SEED = 8
LEAVES = (0.05, 0.1)
METHODS = ("point", "plane")
OK, ILL_POSED, NO_VALID_PIXELS = A.OK, A.ILL_POSED, A.NO_VALID_PIXELS
TILE = 1024                                   # points per workgroup (vmap::kTile)
SIZES = (1, TILE, TILE + 1, 2 * TILE + 37, 5000)
# tests/test_map_align_batch_cpu.py: the scenario, the restatement's winners and their distances from the truth
MS_LEAF, MS_OFFSET, MS_SPACING, MS_MIN_MATCHED = 0.1, (0.21, -0.17, 0.19), 0.2, 6
MEASURED_WINNER = {"point": 6, "plane": 3}
MEASURED_WINNER_ERR = {"point": 4.862e-3, "plane": 8.482e-3}


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip():
    return F.hip_runtime()


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
    """The frame in maps of 0.05 m and 0.1 m at the general pose; an alignment never changes a map."""
    P = R.general_pose()
    maps = {leaf: new_map(reg, leaf) for leaf in LEAVES}
    for m in maps.values():
        m.insert_sphere(None, frame["depth"], P, convention=2)
    yield dict(P=P, guess=A.perturbed(P, 0.01, 0.003, SEED), dev=maps)
    for m in maps.values():
        m.close()


@pytest.fixture(scope="module")
def wall_map(reg):
    """One wall alone in a map of its own: the ill-posed case of point-to-plane."""
    wall = np.ascontiguousarray(PL.corner_scene(5)[:40000:4])
    m = new_map(reg, 0.05, box=None)
    m.insert_cloud(wall, None, EYE)
    yield m, wall
    m.close()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def cm(pose):
    return np.ascontiguousarray(np.asarray(pose, np.float32).T.reshape(16))


def moved(T, d):
    T = np.array(T, np.float32).copy()
    T[:3, 3] += np.asarray(d, np.float32)
    return T


def types(method):
    from rgbd360_amd import _lib
    return (_lib.MapAlignPlaneParams, _lib.MapAlignPlaneResult) if method == "plane" else (_lib.MapAlignParams, _lib.MapAlignResult)


def params_of(m, method, **kw):
    return (m.align_plane_params if method == "plane" else m.align_params)(**kw)


def entry(L, method, name):
    return getattr(L, ("rgbd360_map_align_plane_" if method == "plane" else "rgbd360_map_align_") + name)


def single_trace(L, H):
    from rgbd360_amd import _lib
    n = C.c_int()
    assert L.rgbd360_map_align_eval(H, None, 0, 0, 0, 0, 0, None, 0, None, 0, None, None, None, None, None, 0, C.byref(n), None) == 0
    tr = (_lib.MapAlignTrace * max(n.value, 1))()
    assert L.rgbd360_map_align_eval(H, None, 0, 0, 0, 0, 0, None, 0, None, 0, None, None, None, None, None, n.value, None, tr) == 0
    return n.value, bytes(tr)[:n.value * C.sizeof(_lib.MapAlignTrace)]


def batch_trace(L, H, job):
    from rgbd360_amd import _lib
    n = C.c_int()
    assert L.rgbd360_map_align_batch_trace(H, job, 0, C.byref(n), None) == 0
    tr = (_lib.MapAlignTrace * max(n.value, 1))()
    assert L.rgbd360_map_align_batch_trace(H, job, n.value, None, tr) == 0
    return n.value, bytes(tr)[:n.value * C.sizeof(_lib.MapAlignTrace)]


def single(L, m, method, p, guess, xyz=None, sphere=None, on_device=0):
    """One single call: (status, pose bytes, result struct, its bytes, trace bytes).  sphere: (depth pointer, step, type, rows, cols,
    convention); xyz: a float32 [n, 3] array (host)."""
    rt = types(method)[1]
    pose, res, g = np.zeros(16, np.float32), rt(), cm(guess)
    if sphere is not None:
        rc = entry(L, method, "sphere")(m._handle(), *sphere, vp(g), on_device, C.byref(p), vp(pose), C.byref(res))
    else:
        rc = entry(L, method, "cloud")(m._handle(), vp(xyz), len(xyz), vp(g), on_device, C.byref(p), vp(pose), C.byref(res))
    assert rc >= 0, (rc, L.rgbd360_map_last_error(m._handle()))
    assert rc == res.status
    return rc, pose.tobytes(), res, bytes(res), single_trace(L, m._handle())[1]


def job_array(jobs):
    from rgbd360_amd import _lib
    J = (_lib.MapBatchJob * max(len(jobs), 1))()
    for k, (i, guess) in enumerate(jobs):
        J[k].input = i
        J[k].guess[:] = cm(guess).tolist()
    return J


def batch(L, m, method, p, jobs, clouds=None, frames=None, geometry=None, on_device=0):
    """One batch call: per job (status, pose bytes, result struct, its bytes, trace bytes).  clouds: [(pointer, n)]; frames: [(pointer,
    step)] with geometry = (depth type, rows, cols, convention)."""
    from rgbd360_amd import _lib
    rt = types(method)[1]
    J = job_array(jobs)
    poses, res = np.zeros((len(jobs), 16), np.float32), (rt * len(jobs))()
    if clouds is not None:
        I = (_lib.MapBatchCloud * len(clouds))()
        for k, (ptr, n) in enumerate(clouds):
            I[k].xyz, I[k].n = ptr, n
        rc = entry(L, method, "batch_cloud")(m._handle(), I, len(clouds), on_device, J, len(jobs), C.byref(p), vp(poses), res)
    else:
        I = (_lib.MapBatchFrame * len(frames))()
        for k, (ptr, step) in enumerate(frames):
            I[k].depth, I[k].depth_step = ptr, step
        rc = entry(L, method, "batch_sphere")(m._handle(), I, len(frames), *geometry, on_device, J, len(jobs), C.byref(p), vp(poses), res)
    assert rc == 0, (rc, L.rgbd360_map_last_error(m._handle()))
    assert single_trace(L, m._handle())[0] == 0          # after a batch the single-call trace is empty
    out = []
    for j in range(len(jobs)):
        n, tr = batch_trace(L, m._handle(), j)
        assert n == res[j].iterations
        out.append((res[j].status, poses[j].tobytes(), res[j], bytes(res[j]), tr))
    return out


def addr(a):
    return C.c_void_p(a.ctypes.data)


def same(got, want, what=""):
    assert got[0] == want[0], (what, got[0], want[0])
    assert got[1] == want[1], (what, "pose", np.frombuffer(got[1], np.float32), np.frombuffer(want[1], np.float32))
    assert got[3] == want[3], (what, "result struct")
    assert got[4] == want[4], (what, "trace", len(got[4]), len(want[4]))


@pytest.fixture(scope="module")
def cloud_case(frame, world, wall_map):
    """Test 1's batch: six inputs, 17 jobs.  Inputs 0-4 are cut from the frame's valid points (1 point; one full tile; a tile and one
    point; two tiles and a ragged third; five tiles, the last ragged), input 5 is the wall.  Per input of the frame the guesses are the
    map pose, a guess 1 cm and 3 mrad off and one 0.5 m off; the wall, which lies elsewhere, gets the first two."""
    c = frame["cloud"].reshape(-1, 3)
    valid = c[np.isfinite(c).all(axis=1) & (np.abs(c).sum(axis=1) > 0)]
    assert len(valid) >= 4 * SIZES[-1]
    # every cut spans the whole image (the top rows alone lie outside the map's box): n points evenly spaced among the valid ones
    inputs = [np.ascontiguousarray(valid[np.linspace(len(valid) // 2 if n == 1 else 0, len(valid) - 1, n).astype(np.int64)]) for n in SIZES] + [wall_map[1]]
    P = world["P"]
    guesses = (P, world["guess"], moved(P, (0.5, 0.0, 0.0)))
    jobs = [(i, g) for i in range(5) for g in guesses] + [(5, guesses[0]), (5, guesses[1])]
    assert len(jobs) == 17 and len(inputs) == 6
    return dict(inputs=inputs, jobs=jobs)


_singles = {}


def singles_of(L, world, cloud_case, method, leaf, **kw):
    """The single calls of test 1's jobs, made once per (method, leaf, params) and shared."""
    key = (method, leaf, tuple(sorted(kw.items())))
    if key not in _singles:
        m = world["dev"][leaf]
        p = params_of(m, method, **kw)
        _singles[key] = [single(L, m, method, p, g, xyz=cloud_case["inputs"][i]) for i, g in cloud_case["jobs"]]
    return _singles[key]


def cloud_batch(L, world, cloud_case, method, leaf, jobs=None, **kw):
    m = world["dev"][leaf]
    return batch(L, m, method, params_of(m, method, **kw), cloud_case["jobs"] if jobs is None else jobs,
                 clouds=[(addr(x), len(x)) for x in cloud_case["inputs"]])


@pytest.mark.parametrize("method", METHODS)
def test_clouds_equal_the_single_calls(hip_lib, world, wall_map, cloud_case, method):
    seen = []
    for leaf in LEAVES:
        want = singles_of(hip_lib, world, cloud_case, method, leaf)
        got = cloud_batch(hip_lib, world, cloud_case, method, leaf)
        for j, (g, w) in enumerate(zip(got, want)):
            same(g, w, (method, leaf, "job", j))
        seen += [(r[2].status, r[2].iterations, r[2].converged) for r in got]
    # the wall in its own map, its own batch: three guesses
    m, wall = wall_map
    p = params_of(m, method)
    wall_jobs = [(0, EYE), (0, A.perturbed(EYE, 0.01, 0.003, SEED)), (0, moved(EYE, (0.5, 0.0, 0.0)))]
    got = batch(hip_lib, m, method, p, wall_jobs, clouds=[(addr(wall), len(wall))])
    for j, (i, g) in enumerate(wall_jobs):
        same(got[j], single(hip_lib, m, method, p, g, xyz=wall), (method, "wall", j))
    seen += [(r[2].status, r[2].iterations, r[2].converged) for r in got]
    # max_iters = 2: a job stopped by the limit
    limited = []
    for leaf in LEAVES:
        want = singles_of(hip_lib, world, cloud_case, method, leaf, max_iters=2)
        got = cloud_batch(hip_lib, world, cloud_case, method, leaf, max_iters=2)
        for j, (g, w) in enumerate(zip(got, want)):
            same(g, w, (method, leaf, "max_iters 2, job", j))
        limited += [(r[2].status, r[2].iterations, r[2].converged) for r in got]
    print(method, "max_iters 2:", limited)
    assert any(st == OK and it == 2 and not cv for st, it, cv in limited), limited
    # not trivial: jobs that converge after different numbers of steps, one without matches, and (point-to-plane: a single wall leaves
    # three directions free; the point-to-point normal matrix of points not on one line has full rank) an ill-posed one
    print(method, sorted(set(seen)))
    assert len({it for st, it, cv in seen if st == OK and cv}) >= 2, seen
    assert sum(st == OK for st, it, cv in seen) >= 8, seen
    assert any(st == NO_VALID_PIXELS for st, it, cv in seen), seen
    if method == "plane":
        assert any(st == ILL_POSED for st, it, cv in seen), seen


@pytest.mark.parametrize("method", METHODS)
def test_an_empty_input(hip_lib, world, method):
    from rgbd360_amd import _lib
    m = world["dev"][0.05]
    p = params_of(m, method)
    jobs = [(0, world["P"]), (0, world["guess"]), (0, EYE)]
    for ptr in (None, addr(np.zeros((1, 3), np.float32))):
        got = batch(hip_lib, m, method, p, jobs, clouds=[(ptr, 0)])
        for (st, pose, res, raw, tr), (i, g) in zip(got, jobs):
            zero = types(method)[1]()
            zero.status = NO_VALID_PIXELS
            assert st == NO_VALID_PIXELS and pose == cm(g).tobytes() and raw == bytes(zero) and tr == b""
    # next to a live input: the empty one's jobs as above, the live one's as the single call
    x = np.ascontiguousarray(np.zeros((5, 3), np.float32) + 0.5)
    got = batch(hip_lib, m, method, p, [(0, EYE), (1, world["P"]), (0, world["guess"])], clouds=[(None, 0), (addr(x), len(x))])
    assert got[0][0] == got[2][0] == NO_VALID_PIXELS and got[2][1] == cm(world["guess"]).tobytes()
    same(got[1], single(hip_lib, m, method, p, world["P"], xyz=x))


def device_copy(hip, keep, a):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, vp(a), a.nbytes, 1) == 0
    keep.append(p)
    return p


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", ("uint16", "float32"))
def test_sphere_frames_in_every_form(hip_lib, hip, world, small_pair, method, dtype):
    """Both frames of the pair as two inputs, six jobs; from host memory, from device memory and with padded rows."""
    depths = [np.ascontiguousarray(small_pair[k][1]) for k in (0, 1)]
    assert depths[0].dtype == np.uint16
    if dtype == "float32":
        depths = [(d.astype(np.float32) * np.float32(0.001)).astype(np.float32) for d in depths]
    rows, cols = depths[0].shape
    geometry = (0 if dtype == "uint16" else 1, rows, cols, 2)
    m = world["dev"][0.05]
    p = params_of(m, method)
    P = world["P"]
    jobs = [(0, world["guess"]), (1, P), (0, P), (1, world["guess"]), (1, moved(P, (0.5, 0.0, 0.0))), (0, A.perturbed(P, 0.02, 0.005, 3))]
    want = [single(hip_lib, m, method, p, g, sphere=(vp(depths[i]), depths[i].strides[0]) + geometry) for i, g in jobs]
    assert any(w[2].status == OK and w[2].iterations >= 2 for w in want)
    dev = []
    try:
        padded = [F.padded_rows(d, 64) for d in depths]
        forms = {"host": (0, [(addr(d), d.strides[0]) for d in depths]),
                 "host, padded rows": (0, [(addr(b), b.shape[1]) for b in padded]),
                 "device": (1, [(device_copy(hip, dev, d), d.strides[0]) for d in depths]),
                 "device, padded rows": (1, [(device_copy(hip, dev, b), b.shape[1]) for b in padded])}
        for name, (on_device, frames) in forms.items():
            got = batch(hip_lib, m, method, p, jobs, frames=frames, geometry=geometry, on_device=on_device)
            for j, (g, w) in enumerate(zip(got, want)):
                same(g, w, (method, dtype, name, "job", j))
    finally:
        for d in dev:
            hip.hipFree(d)


@pytest.mark.parametrize("method", METHODS)
def test_the_strip_in_every_form(hip_lib, reg, method):
    """The 1100 x 24 strip (a full tile and a ragged second tile per row) in a map of its own, three jobs."""
    from rgbd360_amd import _lib
    forms = F.Forms(reg)
    try:
        with new_map(reg, F.LEAF, 1 << 14) as m:
            st = _lib.MapStats()
            assert hip_lib.rgbd360_map_insert_sphere(m._handle(), *forms.forms["u16"][1], vp(cm(F.POSE_A)), 0, C.byref(st)) == 0
            p = params_of(m, method)
            guesses = [A.perturbed(F.POSE_A, 0.01, 0.003, 7), F.POSE_A, F.pose_b()]
            jobs = [(0, g) for g in guesses]
            for name in ("u16", "f32_padded"):
                kind, host, dev = forms.forms[name]
                want = [single(hip_lib, m, method, p, g, sphere=host[2:]) for g in guesses]
                assert want[0][2].status == OK and want[0][2].iterations >= 1 and want[0][2].n_matched > 1000
                for on_device, args in ((0, host), (1, dev)):
                    got = batch(hip_lib, m, method, p, jobs, frames=[(args[2], args[3])], geometry=args[4:], on_device=on_device)
                    for j, (g, w) in enumerate(zip(got, want)):
                        same(g, w, (method, name, on_device, "job", j))
    finally:
        forms.close()


@pytest.mark.parametrize("method", METHODS)
def test_jobs_do_not_depend_on_each_other(hip_lib, world, cloud_case, method):
    leaf = 0.05
    want = singles_of(hip_lib, world, cloud_case, method, leaf)
    jobs = cloud_case["jobs"]
    order = np.random.default_rng(17).permutation(len(jobs)).tolist()
    assert order != sorted(order)
    got = cloud_batch(hip_lib, world, cloud_case, method, leaf, jobs=[jobs[k] for k in order])
    for at, k in enumerate(order):
        same(got[at], want[k], (method, "permuted", at, k))
    for k in range(len(jobs)):               # each job alone
        same(cloud_batch(hip_lib, world, cloud_case, method, leaf, jobs=[jobs[k]])[0], want[k], (method, "alone", k))
    twice = [jobs[4], jobs[13], jobs[4], jobs[0], jobs[4]]
    got = cloud_batch(hip_lib, world, cloud_case, method, leaf, jobs=twice)
    for at, k in enumerate((4, 13, 4, 0, 4)):
        same(got[at], want[k], (method, "repeated", at, k))


@pytest.mark.parametrize("method", METHODS)
def test_no_iterations_is_the_final_evaluation(hip_lib, world, cloud_case, method):
    want = singles_of(hip_lib, world, cloud_case, method, 0.05, max_iters=0)
    got = cloud_batch(hip_lib, world, cloud_case, method, 0.05, max_iters=0)
    for j, (g, w) in enumerate(zip(got, want)):
        same(g, w, (method, "job", j))
        assert g[2].iterations == 0 and g[4] == b"" and g[1] == cm(cloud_case["jobs"][j][1]).tobytes()
    assert any(g[2].n_matched > 1000 for g in got)


@pytest.mark.parametrize("method", METHODS)
def test_a_level_map(hip_lib, world, cloud_case, method):
    lv = world["dev"][0.05].level(1)
    p = params_of(lv, method)
    assert abs(p.max_dist - 0.1) < 1e-6
    jobs = cloud_case["jobs"]
    got = batch(hip_lib, lv, method, p, jobs, clouds=[(addr(x), len(x)) for x in cloud_case["inputs"]])
    for j, (i, g) in enumerate(jobs):
        same(got[j], single(hip_lib, lv, method, p, g, xyz=cloud_case["inputs"][i]), (method, "level 1, job", j))
    assert any(r[2].status == OK and r[2].converged for r in got)


def test_the_map_is_untouched(hip_lib, world, cloud_case):
    m = world["dev"][0.05]
    before = m.records()
    x = cloud_case["inputs"][4]
    pose0, res0 = m.align_cloud_plane(x, world["guess"])
    for method in METHODS:
        cloud_batch(hip_lib, world, cloud_case, method, 0.05)
    assert np.array_equal(m.records(), before) and len(before) > 1000
    pose1, res1 = m.align_cloud_plane(x, world["guess"])
    assert pose0.tobytes() == pose1.tobytes()
    assert all(np.array_equal(res0[k], res1[k]) for k in res0)
    assert len(m.align_trace()) == res1["iterations"]


@pytest.mark.parametrize("method", METHODS)
def test_refusals(hip_lib, world, method):
    from rgbd360_amd import _lib
    L, m = hip_lib, world["dev"][0.05]
    H = m._handle()
    pt, rt = types(method)
    x = np.ascontiguousarray(np.zeros((8, 3), np.float32) + 0.25)
    d = np.zeros((4, 8), np.uint16)
    good_p = params_of(m, method)
    cloud_entry, sphere_entry = entry(L, method, "batch_cloud"), entry(L, method, "batch_sphere")

    def clouds(items):
        I = (_lib.MapBatchCloud * max(len(items), 1))()
        for k, (ptr, n) in enumerate(items):
            I[k].xyz, I[k].n = ptr, n
        return I

    def refused(call, what):
        poses = np.full((4, 16), 7.0, np.float32)
        res = (rt * 4)()
        C.memset(res, 0x5A, C.sizeof(res))
        rc = call(vp(poses), res)
        err = L.rgbd360_map_last_error(H)
        assert rc == -1 and err, (what, rc, err)
        assert np.all(poses == 7.0) and bytes(res) == b"\x5a" * C.sizeof(res), what

    one, jobs2 = clouds([(addr(x), 8)]), job_array([(0, EYE), (0, EYE)])
    many_inputs = clouds([(addr(x), 8)] * 1025)
    many_jobs = job_array([(0, EYE)] * 1025)
    call = lambda I, n_in, J, n_jobs, p=good_p: (lambda poses, res: cloud_entry(H, I, n_in, 0, J, n_jobs, C.byref(p), poses, res))
    # what the single calls refuse: of the parameters, of an input
    refused(call(one, 1, jobs2, 2, params_of(m, method, max_dist=0.051)), "max_dist above the leaf")
    refused(call(one, 1, jobs2, 2, params_of(m, method, max_iters=1001)), "max_iters above 1000")
    refused(call(one, 1, jobs2, 2, params_of(m, method, min_count=0)), "min_count 0")
    if method == "plane":
        refused(call(one, 1, jobs2, 2, params_of(m, method, min_support=28)), "min_support 28")
    refused(call(clouds([(addr(x), 8), (None, 3)]), 2, jobs2, 2), "a cloud of 3 points without xyz")
    refused(call(clouds([(addr(x), -1)]), 1, jobs2, 2), "a negative point count")
    frames = (_lib.MapBatchFrame * 2)()
    frames[0].depth, frames[0].depth_step, frames[1].depth, frames[1].depth_step = d.ctypes.data, 16, d.ctypes.data, 16
    sphere = lambda I, geometry: (lambda poses, res: sphere_entry(H, I, 2, *geometry, 0, jobs2, 2, C.byref(good_p), poses, res))
    refused(sphere(frames, (0, 4, 8, 3)), "a bad convention")
    refused(sphere(frames, (2, 4, 8, 2)), "a bad depth type")
    frames[1].depth_step = 15
    refused(sphere(frames, (0, 4, 8, 2)), "a row step shorter than a row")
    frames[1].depth, frames[1].depth_step = None, 16
    refused(sphere(frames, (0, 4, 8, 2)), "a frame without depth")
    # the counts, the indices, the arrays
    for n in (0, -1, 1025):
        refused(call(one, 1, many_jobs, n), ("n_jobs", n))
        refused(call(many_inputs, n, jobs2, 2), ("n_inputs", n))
    refused(call(one, 1, job_array([(0, EYE), (1, EYE)]), 2), "an input index past the end")
    refused(call(one, 1, job_array([(-1, EYE), (0, EYE)]), 2), "a negative input index")
    refused(call(None, 1, jobs2, 2), "inputs NULL")
    refused(call(one, 1, None, 2), "jobs NULL")
    res = (rt * 2)()
    C.memset(res, 0x5A, C.sizeof(res))
    assert cloud_entry(H, one, 1, 0, jobs2, 2, C.byref(good_p), None, res) == -1 and L.rgbd360_map_last_error(H)       # poses_out NULL
    assert bytes(res) == b"\x5a" * C.sizeof(res)
    # the stated bounds (the points are never read: the call is refused first)
    refused(call(clouds([(addr(x), 1 << 31)]), 1, jobs2, 2), "more than RGBD360_MAP_BATCH_MAX_ROWS workgroups in one job")
    refused(call(clouds([(addr(x), 1 << 21)]), 1, job_array([(0, EYE)] * 1024), 1024), "more than RGBD360_MAP_BATCH_MAX_ROWS workgroups in all")
    refused(call(clouds([(addr(x), 1 << 27)]), 1, jobs2, 2), "more than RGBD360_MAP_BATCH_MAX_UPLOAD bytes of host input")
    # and the trace of a job the last batch did not have
    assert L.rgbd360_map_align_batch_trace(H, 1 << 20, 0, None, None) == -1 and L.rgbd360_map_align_batch_trace(H, -1, 0, None, None) == -1
    # the arguments of the refused calls, put right, run
    poses, res = np.zeros((2, 16), np.float32), (rt * 2)()
    assert cloud_entry(H, one, 1, 0, jobs2, 2, None, vp(poses), res) == 0 and cloud_entry(H, one, 1, 0, jobs2, 2, C.byref(good_p), vp(poses), None) == 0


@pytest.mark.parametrize("method", METHODS)
def test_multi_start_end_to_end(reg, method):
    """tests/test_map_align_batch_cpu.py's scenario through the Python mirror: the centre guess alone fails, the lattice in one batch call
    has the restatement's winner, within the recorded bound of the truth."""
    P = R.general_pose()
    centre = moved(P, MS_OFFSET)
    guesses = [moved(centre, (MS_SPACING * i, MS_SPACING * j, MS_SPACING * k)) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    src = PL.corner_scene(201, P, step=0.04)
    with new_map(reg, MS_LEAF, box=None) as m:
        m.insert_cloud(PL.corner_scene(101, step=0.02), None, EYE)
        pose, res = (m.align_cloud_plane if method == "plane" else m.align_cloud)(src, centre)
        assert not (res["status"] == OK and A.pose_error(pose, P)[1] <= 0.1)
        poses, results = m.align_batch_cloud([src], [(0, g) for g in guesses], method=method)
        assert poses.shape == (27, 4, 4) and len(results) == 27
        assert poses[13].tobytes() == pose.tobytes() and results[13]["n_matched"] == res["n_matched"]
        winner = m.best_job(results, MS_MIN_MATCHED)
        err = A.pose_error(poses[winner], P)[1]
        print(method, "winner", winner, "matched", results[winner]["n_matched"], "error", err, "centre", res["status"], A.pose_error(pose, P)[1])
        assert winner == MEASURED_WINNER[method]
        assert err <= 1.5 * MEASURED_WINNER_ERR[method]
        assert len(m.align_trace()) == 0 and len(m.align_batch_trace(winner)) == results[winner]["iterations"]
