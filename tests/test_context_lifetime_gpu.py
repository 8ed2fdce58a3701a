"""The lifetime of what the alignment side owns -- the one-pair context, the lock-step sequence engines, the frame store and the 8-sensor
rig -- when frame sizes grow and shrink, other paths run in between, engines are rebuilt and objects are destroyed unused: every output
of a call on the long-lived object equals, byte for byte, that of the same call on an object created for that call alone (modelled on
test_context_regrows_and_is_reused, tests/test_frame360_host_gpu.py).  No tolerance anywhere in this file, and no free-memory reading:
the device is shared, a leak is found by reading the destructors."""
import ctypes as C

import numpy as np
import pytest

from rgbd360_amd import synth

pytestmark = pytest.mark.gpu


def _res(r):
    """every field of an rgbd360_result, floats as bytes"""
    return (int(r.status), [int(x) for x in r.iters], bytes(C.c_float(r.sso)), bytes(C.c_double(r.err_final)), bytes(C.c_double(r.rms_photo)),
            bytes(C.c_double(r.rms_depth)), bytes(r.hessian), bytes(r.gradient))


def _same(a, b):
    """nested tuples / lists / dicts of arrays, bytes and numbers, compared bit for bit"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def _reg(n_pyr, K=None):
    from rgbd360_amd.register import RegisterPhotoICP
    reg = RegisterPhotoICP()
    reg.setNumPyr(n_pyr)
    reg.setMaskSeams(False)                 # the pinhole path refuses a context with the panorama's seam mask
    if K is not None:
        reg.setCameraMatrix(K)
    return reg


def _accepted(res):
    return res[0] == 0 and max(res[1]) >= 1


# ---- one context across frame sizes, with the pinhole path in between -----------------------------------------------------------------
def _sphere_block(reg, pair):
    """alignFrames360 (methods 0, 1, 2; occlusion 1 and 2 for method 2), warpImages and warp_indices of one pair"""
    (rgbA, dA), (rgbB, dB), T = pair
    reg.setTargetFrame(rgbA, dA)
    reg.setSourceFrame(rgbB, dB)
    out = []
    for method, occ in ((0, 0), (1, 0), (2, 0), (2, 1), (2, 2)):
        rc = reg.alignFrames360(np.eye(4), method, occ)
        res = _res(reg._res)
        assert rc == 0 and _accepted(res), (method, occ, res[:2])
        out.append((rc, res, reg.getOptimalPose()))
    wi = reg.warpImages(T, 2)
    assert (wi["winner"] >= 0).any()
    out.append(wi)
    idx = reg.warp_indices(0, T)
    assert (idx[:, 0] >= 0).any()
    out.append(idx)
    return out


def _pinhole_block(reg, pair):
    """alignFrames with occlusion 1 and 2 (the pinhole occlusion set and the pinhole source records are allocated, and freed by the next
    size change) and eval_pinhole"""
    (rgbA, dA), (rgbB, dB), T, _ = pair
    reg.setTargetFrame(rgbA, dA)
    reg.setSourceFrame(rgbB, dB)
    out = []
    for occ in (1, 2):
        rc = reg.alignFrames(np.eye(4), 2, occ)
        res = _res(reg._res)
        assert rc == 0 and _accepted(res), (occ, res[:2])
        out.append((rc, res, reg.getOptimalPose()))
    out.append(reg.eval_pinhole(0, T, 2))
    out.append(reg.eval_pinhole(1, T, 2, 1))
    return out


def test_context_through_sizes_and_pinhole(hip_lib):
    small, large = synth.make_pair(256, 128, seed=31), synth.make_pair(512, 256, seed=31)
    # (seeds and motion chosen on the CPU oracle so that every alignment below accepts a step: at 130 x 34 seed 31 leaves methods 0 and 2
    # at the guess, and the pinhole pair's occlusion-2 alignment finds no valid pixel at the generator's default motion)
    ragged = synth.make_pair(130, 34, seed=5)
    pin = synth.make_pinhole_pair(128, 96, seed=77, trans=0.05, rot_deg=2.0)
    K = pin[3]
    steps = [lambda r: _sphere_block(r, small), lambda r: _pinhole_block(r, pin), lambda r: _sphere_block(r, large),
             lambda r: _pinhole_block(r, pin), lambda r: _sphere_block(r, small)]
    one = _reg(3, K)
    got = [step(one) for step in steps]
    for k, step in enumerate(steps):
        alone = _reg(3, K)
        assert _same(got[k], step(alone)), k
        alone.close()
    assert _same(got[0], got[4]) and _same(got[1], got[3])
    assert not _same(got[0][2], got[2][2])                     # (the two sizes do not give the same pose by accident)
    one.setNumPyr(2)                                           # the object goes on with two levels and the ragged size
    steps2 = [lambda r: _pinhole_block(r, pin), lambda r: _sphere_block(r, ragged), lambda r: _sphere_block(r, small)]
    got2 = [step(one) for step in steps2]
    for k, step in enumerate(steps2):
        alone = _reg(2, K)
        assert _same(got2[k], step(alone)), k
        alone.close()
    one.close()


# ---- alignSequence: the engines and the staging of one context ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seq_frames():
    f256 = [synth.render(synth.trajectory_pose(k, 7), 256, 128, 7) for k in range(6)]
    f130 = [synth.render(synth.trajectory_pose(k, 7), 130, 34, 7) for k in range(4)]
    f32 = [(rgb, d.astype(np.float32) * np.float32(0.001)) for rgb, d in f256[:4]]
    return f256, f130, f32


@pytest.mark.parametrize("contexts", [False, True])
def test_sequence_engines_and_staging_are_rebuilt(hip_lib, seq_frames, contexts):
    """contexts: the per-context route (the siblings and the context's own upload ring) instead of the lock-step engines."""
    f256, f130, f32 = seq_frames
    calls = []
    for n_inflight in (3, 5):
        # four frames of one size, four of the ragged one (the engines are rebuilt), then uint16 / float32 / uint16 depth of one size
        # (the staging slots grow), then six frames (five slots: a second engine)
        calls += [(f256[:4], n_inflight), (f130, n_inflight), (f256[:4], n_inflight), (f32, n_inflight), (f256[:4], n_inflight),
                  (f256, n_inflight)]

    def run(reg, frames, n_inflight):
        if contexts:
            reg.debug_set_sequence_route(True)
        poses, status, iters = reg.alignSequence(frames, method=2, n_inflight=n_inflight)
        assert (status == 0).all() and (iters.max(axis=1) >= 1).all(), (status, iters)
        return poses, status, iters

    one = _reg(3)
    got = [run(one, *c) for c in calls]
    for k, c in enumerate(calls):
        alone = _reg(3)
        assert _same(got[k], run(alone, *c)), k
        alone.close()
    one.close()
    assert _same(got[0], got[2]) and _same(got[0], got[4]) and _same(got[0], got[6])
    assert _same(got[5][0][:3], got[0][0])                     # the first three pairs of the six-frame call


# ---- the frame store's alignment engines ----------------------------------------------------------------------------------------------
def test_store_engines_are_recreated(hip_lib, seq_frames):
    from rgbd360_amd.store import FrameStore
    from tests.test_frame_store_gpu import _assert_bits, _mk, _one_pair
    frames = seq_frames[0][:4]
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]
    want = [_one_pair(frames, t, s, None, 2) for t, s in pairs]
    assert all(w[1] == 0 and max(w[2]) >= 1 for w in want)
    reg = _mk(3)
    st = FrameStore(reg, 4, 128, 256)
    st.put(range(4), frames)
    for n_inflight in (2, 4, 2):                               # one engine of 2 slots, two engines of 2, one of 2 again
        got = st.align(pairs, method=2, n_inflight=n_inflight)
        for k in range(len(pairs)):
            _assert_bits(got, k, want[k], "n_inflight %d" % n_inflight)
    st.close()
    reg.close()


# ---- the rig: a second frame size re-creates its engine -------------------------------------------------------------------------------
def test_rig_second_size_recreates_the_engine(hip_lib):
    from rgbd360_amd.register import Rgbd360Error
    from rgbd360_amd.rig import RegisterDensePhotoICP
    first = synth.make_rig_pair(160, 120, seed=3, trans=0.04, rot_deg=1.5)
    M, Rt, K = first[2:]
    # the intrinsics belong to the rig object: the second size is the same room through the same K on 128 x 96 pixel sensors
    T_w1 = synth.make_pose(np.eye(3), np.asarray(synth.CAM_A, float))
    second = tuple([synth.render_pinhole(T @ Rt[s], 128, 96, 3, False, K) for s in range(len(Rt))] for T in (T_w1, T_w1 @ M)) + (M, Rt, K)
    pairs = [first, second]

    def block(rig, pair):
        f1, f2, M = pair[:3]
        rig.setTargetFrame(f1)
        rig.setSourceFrame(f2)
        ok = rig.align(np.eye(4), 2)
        res = _res(rig._res)
        assert ok and max(res[1]) >= 1, res[:2]
        return ok, res, rig.getPose(), rig.warp_indices(0, M), rig.eval(1, M, 2)

    def fresh(pair):
        return RegisterDensePhotoICP(pair[3], pair[4], n_pyr=3)

    one = fresh(pairs[0])
    got = [block(one, pairs[0])]
    # a target of another size re-creates the engine and forgets both frames: aligning before the source is set again is refused
    one.setTargetFrame(pairs[1][0])
    with pytest.raises(Rgbd360Error, match=r"must be called first \(-2\)"):
        one.align(np.eye(4), 2)
    got.append(block(one, pairs[1]))
    got.append(block(one, pairs[0]))
    for k, pair in enumerate((pairs[0], pairs[1], pairs[0])):
        alone = fresh(pairs[0])
        assert _same(got[k], block(alone, pair)), k
        alone.close()
    one.close()
    assert _same(got[0], got[2])


# ---- destruction without use and after a refusal --------------------------------------------------------------------------------------
def test_destroyed_unused_and_after_refusal(hip_lib, seq_frames):
    from rgbd360_amd._lib import Result
    from rgbd360_amd.register import Rgbd360Error
    from rgbd360_amd.rig import RegisterDensePhotoICP
    reg = _reg(3)                                              # created and closed
    reg._ctx()
    reg.close()
    reg = _reg(3)                                              # its only call was refused
    with pytest.raises(Rgbd360Error, match=r"\(-1\): image too small"):
        reg.setTargetFrame(np.zeros((1, 4, 3), np.uint8), np.zeros((1, 4), np.uint16))
    reg.close()
    # an engine-backed call refused for its slot count
    f256 = seq_frames[0]
    reg = _reg(3)
    rp = (C.c_void_p * 4)(*[f[0].ctypes.data for f in f256[:4]])
    dp = (C.c_void_p * 4)(*[f[1].ctypes.data for f in f256[:4]])
    out = np.zeros(3 * 16, np.float32)
    res = (Result * 3)()
    for n_inflight in (0, 65):
        rc = reg._L.rgbd360_align360_batch(reg._ctx(), 4, rp, 256 * 3, dp, 256 * 2, 0, 128, 256, None, 2, 0, n_inflight, out.ctypes.data_as(C.c_void_p), res)
        assert rc == -1 and reg._L.rgbd360_last_error(reg._ctx()) == b"n_inflight must be in 1..64"
    with pytest.raises(Rgbd360Error, match=r"\(-1\): bad arguments"):
        reg.forced_iters_batch(33, f256[0], f256[1], 1, np.eye(4), 2, 2)          # more pairs than an engine has slots
    reg.close()
    # the lock-step forced schedule: an engine and its frame scratch live for one call
    reg = _reg(3)
    r = reg.forced_iters_batch(2, f256[0], f256[1], 1, np.eye(4), 2, 4)
    alone = _reg(3)
    r2 = alone.forced_iters_batch(2, f256[0], f256[1], 1, np.eye(4), 2, 4)
    assert r["status"] == 0 and _same(r["poses"], r2["poses"]) and _same(r["poses"][0], r["poses"][1])
    assert not np.array_equal(r["poses"][0], np.eye(4, dtype=np.float32))
    reg.close()
    alone.close()
    # a rig without frames
    pair = synth.make_rig_pair(64, 48, seed=3, n_sensors=2)
    rig = RegisterDensePhotoICP(pair[3], pair[4], n_pyr=2)
    rig.close()
