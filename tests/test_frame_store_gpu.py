"""The resident frame store (rgbd360_store_*, rgbd360_amd/store.py) on the device.

The definition of correct: for every pair of an align call, pose (16 floats), status, iters[] and hessian[36] are BIT-equal to
rgbd360_align360 on a fresh context that got the same two frames through rgbd360_set_target / rgbd360_set_source and the same guess.
No tolerance anywhere in this file.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from rgbd360_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mk(n_pyr=3, libm=0):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP()
    r.setNumPyr(n_pyr)
    if libm:
        r.set_index_arithmetic(libm)
    return r


def _one_pair(frames, t, s, guess, method, n_pyr=3, libm=0):
    """The reference result: a FRESH context, set_target / set_source, rgbd360_align360."""
    reg = _mk(n_pyr, libm)
    reg.setTargetFrame(*frames[t])
    reg.setSourceFrame(*frames[s])
    rc = reg.alignFrames360(np.eye(4) if guess is None else guess, method)
    out = (reg.getOptimalPose(), rc, list(reg.num_iterations), np.array(list(reg._res.hessian), np.float32))
    reg.close()
    return out


def _assert_bits(got, k, want, what=""):
    poses, status, iters, results = got
    pose, rc, its, hess = want
    assert status[k] == rc, (what, k, status[k], rc)
    assert list(iters[k]) == its, (what, k, list(iters[k]), its)
    assert poses[k].tobytes() == pose.tobytes(), (what, k, poses[k], pose)
    assert np.array(list(results[k].hessian), np.float32).tobytes() == hess.tobytes(), (what, k)


def _same(a, b, ka, kb):
    return (a[0][ka].tobytes() == b[0][kb].tobytes() and a[1][ka] == b[1][kb] and list(a[2][ka]) == list(b[2][kb]) and
            bytes(a[3][ka]) == bytes(b[3][kb]))


@pytest.fixture(scope="module")
def frames6():
    return [synth.render(synth.trajectory_pose(k, 7), 256, 128, 7) for k in range(6)]


# consecutive pairs, a skipped pair and its reverse, a self pair, entry 4 as target of five pairs, one repeated pair
PAIRS = [(0, 1), (1, 2), (2, 3), (0, 3), (3, 0), (2, 2), (4, 0), (4, 1), (4, 2), (4, 3), (4, 5), (0, 3)]


def _true_rel(t, s):
    """The pose of source frame s in target frame t (what alignFrames360 converges to), from the generator's trajectory."""
    return np.linalg.inv(synth.trajectory_pose(t, 7)) @ synth.trajectory_pose(s, 7)


def _guesses(pairs):
    out = []
    for k, (t, s) in enumerate(pairs):
        if k % 3 == 0:
            out.append(np.eye(4))
        elif k % 3 == 1:
            out.append(_true_rel(t, s))
        else:
            d = synth.make_pose(synth.rodrigues(np.array([0.0, 1.0, 0.0]), 0.02), np.array([0.03, 0.0, 0.0]))
            out.append(_true_rel(t, s) @ d)
    return np.stack(out).astype(np.float32)


@pytest.fixture()
def store6(hip_lib, frames6):
    from rgbd360_amd.store import FrameStore
    reg = _mk(3)
    st = FrameStore(reg, 8, 128, 256)
    st.put(list(range(6)), frames6)
    yield st
    st.close()
    reg.close()


@pytest.mark.parametrize("method", [0, 1, 2])
def test_arbitrary_pairs_equal_the_one_pair_path(hip_lib, frames6, store6, method):
    got = store6.align(PAIRS, method=method)
    for k, (t, s) in enumerate(PAIRS):
        _assert_bits(got, k, _one_pair(frames6, t, s, None, method), "method %d" % method)
    assert _same(got, got, 3, 11)            # the repeated pair


def test_per_pair_guesses(hip_lib, frames6, store6):
    """Pair k starts from guess k and from nothing else: bit-equal to the one-pair path with that guess, and a permuted list gives the
    permuted results."""
    G = _guesses(PAIRS)
    got = store6.align(PAIRS, guesses=G, method=2)
    for k, (t, s) in enumerate(PAIRS):
        _assert_bits(got, k, _one_pair(frames6, t, s, G[k], 2), "guess")
    assert not _same(got, got, 3, 11)        # the repeated pair, now from two different guesses
    perm = np.random.default_rng(5).permutation(len(PAIRS))
    got2 = store6.align([PAIRS[i] for i in perm], guesses=G[perm], method=2, n_inflight=5)
    for j, i in enumerate(perm):
        assert _same(got2, got, j, i), (j, i)


def test_slot_count_invariance(hip_lib, frames6, store6):
    pairs = PAIRS[:11]
    G = _guesses(pairs)
    want = [_one_pair(frames6, t, s, G[k], 2) for k, (t, s) in enumerate(pairs)]
    for n_inflight in (1, 2, 3, 5, 32, 64):
        got = store6.align(pairs, guesses=G, method=2, n_inflight=n_inflight)
        for k in range(len(pairs)):
            _assert_bits(got, k, want[k], "n_inflight %d" % n_inflight)


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def _to_device(hip, a):
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
    assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0      # hipMemcpyHostToDevice
    return p.value


def test_consecutive_pairs_equal_the_sequence_entry(hip_lib, frames6, store6):
    """Pairs (j, j + 1) with one guess: the output of rgbd360_align360_batch_dev, every field of rgbd360_result included."""
    from rgbd360_amd._lib import Result
    reg = _mk(3)
    hip = _hip()
    rgb_d = [_to_device(hip, f[0]) for f in frames6]
    dep_d = [_to_device(hip, f[1]) for f in frames6]
    g = synth.make_pose(synth.rodrigues(np.array([0.0, 0.0, 1.0]), 0.01), np.array([0.0, 0.01, 0.0]))
    n = 5
    out = np.zeros(n * 16, np.float32)
    res = (Result * n)()
    from rgbd360_amd.register import pose_to_cm, pose_from_cm
    gcm = pose_to_cm(g)
    rp = (C.c_void_p * 6)(*rgb_d)
    dp = (C.c_void_p * 6)(*dep_d)
    rc = reg._L.rgbd360_align360_batch_dev(reg._ctx(), 6, rp, 256 * 3, dp, 256 * 2, 0, 128, 256, gcm.ctypes.data_as(C.c_void_p), 2, 0, 4,
                                           out.ctypes.data_as(C.c_void_p), res)
    assert rc == 0
    for q in rgb_d + dep_d:
        hip.hipFree(C.c_void_p(q))
    pairs = [(j, j + 1) for j in range(n)]
    got = store6.align(pairs, guesses=np.stack([g] * n), method=2, n_inflight=3)
    for k in range(n):
        assert got[0][k].tobytes() == pose_from_cm(out[16 * k:16 * k + 16]).tobytes(), k
        assert bytes(got[3][k]) == bytes(res[k]), k          # the whole record: status, iters, sso, errors, hessian, gradient
    reg.close()


def test_overwrite_an_entry(hip_lib, frames6):
    from rgbd360_amd.store import FrameStore
    reg = _mk(3)
    st = FrameStore(reg, 4, 128, 256)
    assert [st.occupied(e) for e in range(4)] == [False] * 4
    st.put([0, 1, 2], [frames6[0], frames6[1], frames6[2]])          # A = frame 2 in entry 2
    assert [st.occupied(e) for e in range(4)] == [True, True, True, False]
    pairs = [(0, 1), (2, 0), (1, 2), (1, 0), (2, 2)]
    first = st.align(pairs, method=2)
    st.put([2], [frames6[5]])                                        # B = frame 5 in entry 2
    assert [st.occupied(e) for e in range(4)] == [True, True, True, False]
    second = st.align(pairs, method=2)
    fr = {0: 0, 1: 1, 2: 5}
    src = [frames6[k] for k in range(6)]
    for k, (t, s) in enumerate(pairs):
        _assert_bits(second, k, _one_pair(src, fr[t], fr[s], None, 2), "after overwrite")
        if 2 in (t, s):
            assert not _same(first, second, k, k), k
        else:
            assert _same(first, second, k, k), k
    st.close()
    reg.close()


def test_bad_frames_do_not_leak(hip_lib):
    """An entry without any valid depth: the pair that has it as source ends NO_VALID_PIXELS, the other pairs of the same round carry
    the bits of the one-pair path (compare test_native_batch_threads_blank_frame_and_odd_spans).  Then float32 depth with NaN / Inf /
    negative / out-of-range patches and ramps in every frame."""
    from rgbd360_amd.store import FrameStore
    frames = [synth.render(synth.trajectory_pose(k, 11), 256, 128, 11) for k in range(5)]
    frames[2] = (frames[2][0], np.zeros_like(frames[2][1]))
    reg = _mk(3)
    st = FrameStore(reg, 5, 128, 256)
    st.put(range(5), frames)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 2), (0, 4)]
    got = st.align(pairs, method=2, n_inflight=32)                   # one round
    assert got[1][1] == 2 and got[1][4] == 2                         # RGBD360_NO_VALID_PIXELS
    assert all(got[1][k] == 0 for k in (0, 2, 3, 5))                 # a blank TARGET still aligns photometrically
    for k, (t, s) in enumerate(pairs):
        _assert_bits(got, k, _one_pair(frames, t, s, None, 2), "blank frame")
    f32 = [(f[0], synth.spoil_depth(f[1].astype(np.float32) * np.float32(0.001), k + 1, ramps=True)) for k, f in enumerate(frames)]
    st.put(range(5), f32)
    for method in (1, 2):
        got = st.align(pairs, method=method, n_inflight=4)
        for k, (t, s) in enumerate(pairs):
            _assert_bits(got, k, _one_pair(f32, t, s, None, method), "spoiled float depth")
    st.close()
    reg.close()


@pytest.mark.parametrize("W,H,n_pyr", [(250, 101, 3), (480, 80, 3), (1000, 37, 2), (66, 18, 1), (130, 34, 2)])
def test_ragged_sizes_padded_rows_and_device_pointers(hip_lib, W, H, n_pyr):
    from rgbd360_amd.store import FrameStore
    frames = [synth.render(synth.trajectory_pose(k, 7), W, H, 7) for k in range(4)]
    pairs = [(0, 1), (1, 2), (3, 1), (2, 0), (0, 3)]
    want = {m: [_one_pair(frames, t, s, None, m, n_pyr) for t, s in pairs] for m in (0, 1, 2)}
    reg = _mk(n_pyr)
    st = FrameStore(reg, 4, H, W)
    st.put(range(4), frames)
    for m in (0, 1, 2):
        got = st.align(pairs, method=m, n_inflight=3)
        for k in range(len(pairs)):
            _assert_bits(got, k, want[m][k], "packed host")
    # row-padded host images (cv::Mat ROI style), float32 metres
    f32 = [(f[0], f[1].astype(np.float32) * np.float32(0.001)) for f in frames]
    want32 = [_one_pair(f32, t, s, None, 2, n_pyr) for t, s in pairs]
    pads = []
    for rgb, d in f32:
        R = np.zeros((H, W + 41, 3), np.uint8); R[:, :W] = rgb
        D = np.zeros((H, W + 33), np.float32); D[:, :W] = d
        pads.append((R[:, :W], D[:, :W]))
    assert pads[0][0].strides[0] == (W + 41) * 3
    st.put([3, 2, 1, 0], pads[::-1])
    got = st.align(pairs, method=2)
    for k in range(len(pairs)):
        _assert_bits(got, k, want32[k], "padded host f32")
    # device pointers, padded rows
    hip = _hip()
    ptrs = []
    for rgb, d in frames:
        R = np.zeros((H, W * 3 + 7), np.uint8); R[:, :W * 3] = rgb.reshape(H, W * 3)
        D = np.zeros((H, W + 5), np.uint16); D[:, :W] = d
        ptrs.append((_to_device(hip, R), _to_device(hip, D)))
    st.put_dev([0, 1, 2, 3], [p[0] for p in ptrs], [p[1] for p in ptrs], 0, rgb_step=W * 3 + 7, depth_step=(W + 5) * 2)
    for p in ptrs:
        hip.hipFree(C.c_void_p(p[0])); hip.hipFree(C.c_void_p(p[1]))
    got = st.align(pairs, method=2, n_inflight=2)
    for k in range(len(pairs)):
        _assert_bits(got, k, want[2][k], "device pointers")
    st.close()
    reg.close()


def test_full_size_compact_source_records(hip_lib):
    """2048 x 1024, 4 levels, PHOTO_DEPTH: level 0 and 1 carry the 8-byte source record here."""
    from rgbd360_amd.store import FrameStore
    frames = [synth.render(synth.trajectory_pose(k, 7), 2048, 1024, 7) for k in range(4)]
    pairs = [(0, 1), (1, 0), (0, 3), (2, 1), (3, 3), (2, 3)]
    reg = _mk(4)
    st = FrameStore(reg, 4, 1024, 2048)
    st.put(range(4), frames)
    n = [2048 * 1024 >> (2 * l) for l in range(4)]
    assert st.entry_bytes == sum(x * ((8 if x >= 256 * 1024 else 16) + 24) for x in n)
    got = st.align(pairs, method=2, n_inflight=4)
    for k, (t, s) in enumerate(pairs):
        _assert_bits(got, k, _one_pair(frames, t, s, None, 2, 4), "2048x1024")
    st.close()
    reg.close()


@pytest.mark.parametrize("method", [0, 1, 2])
def test_reference_index_arithmetic(hip_lib, frames6, method):
    """rgbd360_set_index_arithmetic(1) on the context: the store's passes warp in the reference's libm arithmetic too."""
    from rgbd360_amd.store import FrameStore
    reg = _mk(3, libm=1)
    st = FrameStore(reg, 6, 128, 256)
    st.put(range(6), frames6)
    got = st.align(PAIRS, method=method)
    for k, (t, s) in enumerate(PAIRS):
        _assert_bits(got, k, _one_pair(frames6, t, s, None, method, 3, libm=1), "libm")
    # and the mode is read at every align call
    reg.set_index_arithmetic(0)
    got0 = st.align(PAIRS[:4], method=method)
    for k, (t, s) in enumerate(PAIRS[:4]):
        _assert_bits(got0, k, _one_pair(frames6, t, s, None, method, 3, libm=0), "back to the device arithmetic")
    st.close()
    reg.close()


def test_the_real_sample_pair(hip_lib):
    """The stitched panoramas of tests/golden/sample_pair (built as tests/test_samples_gpu.py builds them), both directions, all three
    methods; target = frame 1, source = frame 10 is the direction of the committed record."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import config1_samples as c1
    from rgbd360_amd.register import RegisterPhotoICP, stitch_sphere
    from rgbd360_amd.store import FrameStore
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "config1_samples.json")))
    Rt_inv = np.stack(c1.load_extrinsics("fixture"))
    sreg = RegisterPhotoICP()
    panos = []
    for idx in (1, 10):
        fr = c1.frames(idx, "fixture")
        panos.append(stitch_sphere(sreg, np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), Rt_inv))
    sreg.close()
    reg = _mk(4)
    st = FrameStore(reg, 2, *panos[0][1].shape)
    st.put([0, 1], panos)
    for method in (0, 1, 2):
        got = st.align([(0, 1), (1, 0)], method=method)
        for k, (t, s) in enumerate([(0, 1), (1, 0)]):
            _assert_bits(got, k, _one_pair(panos, t, s, None, method, 4), "sample pair")
        assert list(got[2][0]) == gold["alignments"]["m%d_o0" % method]["device"]["iters"]
        if method != 1:
            assert list(got[2][0]) == [10, 10, 10, 7]
    st.close()
    reg.close()


def test_errors_leave_no_state_behind(hip_lib, frames6, store6):
    from rgbd360_amd._lib import Result
    from rgbd360_amd.register import Rgbd360Error
    L, h = store6._L, store6._handle()
    good = store6.align(PAIRS[:3], method=2)

    def call(trg, src, method=2, occlusion=0, n_inflight=4, n=None):
        t = np.array(trg, np.int32); s = np.array(src, np.int32)
        n = len(trg) if n is None else n
        out = np.full(max(n, 1) * 16, 7.0, np.float32)
        res = (Result * max(n, 1))()
        rc = L.rgbd360_store_align(h, n, t.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), None, method, occlusion, n_inflight,
                                   out.ctypes.data_as(C.c_void_p), res)
        return rc, out, L.rgbd360_store_last_error(h).decode()

    rc, out, msg = call([0, 1, 8], [1, 2, 0])                        # capacity is 8
    assert rc == -1 and "pair 2" in msg and (out == 7.0).all()
    rc, out, msg = call([0, -1], [1, 2])
    assert rc == -1 and "pair 1" in msg and (out == 7.0).all()
    rc, out, msg = call([0, 1], [7, 2])                              # entry 7 is empty
    assert rc == -1 and "pair 0" in msg and "empty" in msg and (out == 7.0).all()
    rc, out, msg = call([0], [1], occlusion=1)
    assert rc == -1 and msg and (out == 7.0).all()
    rc, out, msg = call([0], [1], n_inflight=0)
    assert rc == -1 and msg
    rc, out, msg = call([0], [1], n_inflight=65)
    assert rc == -1 and msg
    rc, out, msg = call([0], [1], method=3)
    assert rc == -4 and msg
    rc, out, msg = call([0], [1], n=0)
    assert rc == 0 and (out == 7.0).all()
    assert L.rgbd360_store_occupied(h, 8) == -1 and L.rgbd360_store_occupied(h, -1) == -1 and L.rgbd360_store_occupied(h, 7) == 0
    # create: capacity 0, the size limits of the sequence entry
    hh = C.c_void_p()
    ctx = store6._reg._ctx()
    assert L.rgbd360_store_create(ctx, 0, 128, 256, C.byref(hh)) == -1 and not hh.value
    assert L.rgbd360_last_error(ctx)
    assert L.rgbd360_store_create(ctx, 2, 4, 16, C.byref(hh)) == -1 and not hh.value          # too small for 3 levels
    # put: entry out of range / twice, through the C ABI
    f = frames6[0]
    e = np.array([1, 1], np.int32)
    rp = (C.c_void_p * 2)(f[0].ctypes.data, f[0].ctypes.data)
    dp = (C.c_void_p * 2)(f[1].ctypes.data, f[1].ctypes.data)
    assert L.rgbd360_store_put(h, 2, e.ctypes.data_as(C.c_void_p), rp, 256 * 3, dp, 256 * 2, 0, 0) == -1
    assert "twice" in L.rgbd360_store_last_error(h).decode()
    e[1] = 8
    assert L.rgbd360_store_put(h, 2, e.ctypes.data_as(C.c_void_p), rp, 256 * 3, dp, 256 * 2, 0, 0) == -1
    assert L.rgbd360_store_put(h, 2, e.ctypes.data_as(C.c_void_p), rp, 256 * 3 - 1, dp, 256 * 2, 0, 0) == -1
    # the mirror raises
    with pytest.raises(Rgbd360Error):
        store6.align([(0, 7)])
    with pytest.raises(Rgbd360Error):
        store6.align([(0, 1)], occlusion=1)
    # nothing of all that stayed: the same call gives the same bits, entry 1 still holds frame 1
    again = store6.align(PAIRS[:3], method=2)
    for k in range(3):
        assert _same(good, again, k, k)


def test_keyframe_odometry_example(hip_lib, tmp_path):
    """examples/keyframe_odometry.cpp on 8 synthetic frames: the printed poses are the Python mirror's (same windows, same store calls),
    with the reference's residual threshold (the keyframe stays) and with a threshold no frame meets (every frame becomes one)."""
    from rgbd360_amd import build
    from rgbd360_amd.store import FrameStore
    lib = build.build()
    exe = os.path.join(str(tmp_path), "keyframe_odometry")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "keyframe_odometry.cpp"), "-L" + os.path.dirname(lib), "-lrgbd360_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-pthread", "-o", exe])
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "8", "256", "128"])
    frames = [synth.render(synth.trajectory_pose(k, 7), 256, 128, 7) for k in range(8)]

    def mirror(window, max_residual):
        """The example's loop on the Python mirror: keyframe = target, a window per align call, guess = the last result against the
        keyframe; a frame that fails the residual test becomes the keyframe and the resident frames behind it are aligned again."""
        reg = _mk(4)
        st = FrameStore(reg, window + 1, 128, 256)
        free = list(range(window, 0, -1))
        st.put([0], [frames[0]])
        kf, kf_entry, guess, nxt, pending, rows = 0, 0, np.eye(4, dtype=np.float32), 1, [], []
        while nxt < 8 or pending:
            ents = []
            while len(pending) < window and nxt < 8:
                ents.append(free.pop())
                pending.append((nxt, ents[-1]))
                nxt += 1
            st.put(ents, [frames[f] for f, _ in pending[len(pending) - len(ents):]])
            poses, status, iters, res = st.align([(kf_entry, e) for _, e in pending], guesses=np.stack([guess] * len(pending)), method=2)
            j = 0
            while j < len(pending):
                f, e = pending[j]
                rows.append((f, kf, int(status[j]), poses[j]))
                j += 1
                if status[j - 1] == 0 and res[j - 1].rms_depth < max_residual:
                    guess = poses[j - 1]
                    free.append(e)
                    continue
                free.append(kf_entry)
                kf, kf_entry, guess = f, e, np.eye(4, dtype=np.float32)
                break
            pending = pending[j:]
        st.close()
        reg.close()
        return rows

    for window, max_residual, n_keyframes in ((3, 0.9, 1), (3, 0.0, 8)):
        out = subprocess.check_output([exe, str(seq), "8", "256", "128", str(window), repr(max_residual)], text=True)
        rows = [l.split() for l in out.splitlines() if l.startswith("frame ")]
        want = mirror(window, max_residual)
        assert len(rows) == len(want) == 7
        assert [w[0] for w in want] == list(range(1, 8))
        assert [w[1] for w in want] == ([0] * 7 if n_keyframes == 1 else list(range(7)))
        for r, (i, kfi, stt, pose) in zip(rows, want):
            assert int(r[1]) == i and int(r[3]) == kfi and int(r[5]) == stt, (r, i, kfi, stt)
            got = np.array([float(x) for x in r[7:23]], np.float32).reshape(4, 4).T
            assert got.tobytes() == pose.tobytes(), (i, got, pose)
