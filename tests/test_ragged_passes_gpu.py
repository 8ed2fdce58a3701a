"""The occlusion-aware spherical passes (k_occ_build, k_occ_build_fs, k_eval_occ), the pinhole passes (k_src_rec_pinhole,
k_eval_pinhole, k_pin_occ_keys, k_pin_occ_walk, k_warp_indices_pinhole) and the rig pass at sizes where NO pyramid level fills its
last wave, against the CPU oracle: the wave-wide run detection and segmented scan with lanes that hold no pixel, the clamped loads
at n - 1, the tail step of a 1024-thread block, the idle lanes of the walk's block reduction, the box scan at odd `cols`, level_K
and the pyramids at odd sizes.  And the 7-bit generation of the occlusion list heads across two wraps on one context.

The inputs and what makes them binding (level sizes, list lengths, conflicts, one accept / reject sequence in the oracle's four
arithmetic settings) are pinned without a GPU in tests/test_ragged_cases_cpu.py; both files take them from tests/ragged_cases.py.

Pose rule: the pose constants of the suite were set at 256x128, 320x240 and 160x120.  For every alignment here the bound is
max(constant, 4 x d), d = the oracle's own pose distance between float32 and float64 accumulation (reduce_mode 0 / 1 at math_mode 1)
on this input -- the device adds float32 partial sums in a third order, hence the factor.  Both numbers and the measured distance
are printed.  A pose beyond the bound is a defect to find, not a number to widen."""
import numpy as np
import pytest

from rgbd360_amd import synth
from tests import ragged_cases as RC
from tests.test_gpu_parity import (ERR2_RTOL, HG_RTOL, PINHOLE_ROT_TOL_DEV, PINHOLE_TRANS_TOL_DEV, POSE_TOL_DEV, _assert_libm_oracle_agrees,
                                   _mk, _pair_ctx, _pinhole_probe_pose, _poses)
from tests.test_rig_dense import POSE_TOL_DEV as RIG_POSE_TOL_DEV

pytestmark = pytest.mark.gpu


def _assert_pose(what, pose, runs, constants):
    """The pose rule of this file's docstring against the oracle's device-arithmetic run (math_mode 1, float64 sums)."""
    spread = RC.reduce_spread(runs)
    bound = RC.pose_bound(constants, spread)
    rot, trans = synth.pose_error(pose, runs[(1, 1)][2])
    print(f"{what}: device vs oracle {rot:.3e} rad {trans:.3e} m; constants {constants[0]:.1e} / {constants[1]:.1e}; "
          f"4 x oracle float32-vs-float64 sums {4 * spread[0]:.3e} / {4 * spread[1]:.3e}")
    assert rot <= bound[0] and trans <= bound[1], (what, rot, trans, bound)


def _assert_sums(e, sp, sd, Hd, gd):
    assert abs(e["err2_split"][0] - sp) <= ERR2_RTOL * max(1.0, abs(sp)), (e["err2_split"], sp)
    assert abs(e["err2_split"][1] - sd) <= ERR2_RTOL * max(1.0, abs(sd)), (e["err2_split"], sd)
    scale_h = max(np.abs(Hd).max(), 1e-30)
    assert np.abs(e["H64"] - Hd).max() <= HG_RTOL * scale_h
    assert np.abs(e["g64"] - gd).max() <= HG_RTOL * max(np.abs(gd).max(), 1e-3 * np.sqrt(scale_h))


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("err2_split", "n_split", "H", "g", "H64", "g64")) \
        and a["n_visible"] == b["n_visible"] and a["err2"] == b["err2"] and a["n_valid"] == b["n_valid"]


# ---- occlusion-aware spherical passes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", sorted(RC.SPHERICAL))
def test_occlusion_eval_parity_at_ragged_sizes(hip_lib, oracle_mod, W, H):
    """test_eval_occlusion_parity's body at 250x101 (n % 64 = 34, 42, 14) and 1000x37 (8, 40): occlusion 1 and 2, the three methods,
    every level, every pose of occlusion_test_poses on one context -- counts exact, sums within the float tolerances."""
    n_pyr = RC.SPHERICAL[(W, H)]
    reg, ora, T = _pair_ctx(hip_lib, oracle_mod, RC.spherical_pair(W, H), n_pyr=n_pyr)
    conflicts = 0
    for level in range(n_pyr):
        assert reg.level_dims(level) == ora.level_dims(level)
        for pose in synth.occlusion_test_poses(T):
            for method in (0, 1, 2):
                plain = reg.eval(level, pose, method, 0)
                for occlusion in (1, 2):
                    e = reg.eval(level, pose, method, occlusion)
                    _, sp, sd, n_p, n_d = ora.error_occ(level, pose, method, occlusion)
                    _, _, Hd, gd, nvis = ora.hessgrad_occ(level, pose, method, occlusion)
                    assert list(e["n_split"]) == [n_p, n_d], (level, method, occlusion, list(e["n_split"]), n_p, n_d)     # integer work: exact
                    assert e["n_visible"] == nvis, (level, method, occlusion, e["n_visible"], nvis)
                    _assert_sums(e, sp, sd, Hd, gd)
                    conflicts += int(plain["n_visible"] != e["n_visible"]) + int(list(plain["n_split"]) != list(e["n_split"]))
    assert conflicts > 0
    reg.close()


def test_both_occlusion_schedules_at_250x101(hip_lib, oracle_mod):
    """The fused {k_occ_build_fs, k_eval_occ} schedule (blocks of 1024 threads whose last span ends at n = 25250, 674 pixels into a
    step) and the three-launch one ({k_occ_build, k_eval_occ, k_solve}: blocks of 256) give bit-identical results from the identity
    and from a guess; each equals the oracle's status and iteration counts, its pose by the pose rule, and the libm oracle agrees."""
    pair = RC.spherical_pair(250, 101)
    (rgbA, dA), (rgbB, dB), T = pair
    ora = RC.spherical_oracle(oracle_mod, pair, 3)
    out = {}
    for fused in (True, False):
        reg = _mk(hip_lib, 3)
        reg.debug_set_schedule(fused_solve=True, fused_occ=fused)
        reg.setTargetFrame(rgbA, dA)
        reg.setSourceFrame(rgbB, dB)
        rows = []
        for occlusion, method in RC.OCC_ALIGNMENTS:
            for from_guess in (False, True):
                rc = reg.alignFrames360(RC.schedule_guess() if from_guess else np.eye(4), method, occlusion)
                rows.append((rc, list(reg.num_iterations), reg.getOptimalPose().copy(), reg.avResidual, reg.SSO))
                runs = RC.spherical_alignments(oracle_mod, 250, 101, occlusion, method, from_guess)
                assert rc == runs[(1, 1)][0] == 0 and rows[-1][1] == runs[(1, 1)][1], (fused, occlusion, method, from_guess, rows[-1][:2], runs[(1, 1)][:2])
                _assert_pose(f"250x101 fused_occ={fused} occ {occlusion} method {method} guess {from_guess}", rows[-1][2], runs,
                             (POSE_TOL_DEV, POSE_TOL_DEV))
                if not from_guess:
                    _assert_libm_oracle_agrees(reg, ora, method, 3, occlusion)
        out[fused] = rows
        reg.close()
    assert len(out[True]) == len(out[False]) == 8
    for a, b in zip(out[True], out[False]):
        assert a[0] == b[0] and a[1] == b[1], (a, b)
        assert np.array_equal(a[2], b[2]), (a, b)
        assert a[3] == b[3] and a[4] == b[4], (a, b)


def test_occlusion_generation_wraps_twice_on_one_context(hip_lib, oracle_mod):
    """The list heads carry a 7-bit generation, cleared once per 127 passes.  2 * 127 + 5 level-0 evaluations on one context cycle the
    four poses and alternate occlusion 1 / 2: every result is, bit for bit, the first one of its (pose, occlusion), and the counts are
    the oracle's; then level 2 and level 0 again.  This holds the passes to be deterministic across the wraps and the generation
    arithmetic (the tag stays within its 7 bits, a pass reads its own generation).  It does NOT bind the memset of the wrap: the four
    (pose, mode) pairs repeat with period 4, so every head a pass exchanges was written four passes earlier, never 127 --
    test_occlusion_generation_wrap_meets_stale_heads runs the schedule that does."""
    reg, ora, T = _pair_ctx(hip_lib, oracle_mod, RC.spherical_pair(250, 101), n_pyr=3)
    poses = synth.occlusion_test_poses(T)
    first = {}
    for i in range(2 * 127 + 5):
        k, occlusion = i % 4, 1 + i % 2
        e = reg.eval(0, poses[k], 2, occlusion)
        if (k, occlusion) not in first:
            first[(k, occlusion)] = e
            _, _, _, n_p, n_d = ora.error_occ(0, poses[k], 2, occlusion)
            assert list(e["n_split"]) == [n_p, n_d] and e["n_visible"] == ora.hessgrad_occ(0, poses[k], 2, occlusion)[4], (i, k, occlusion)
        else:
            assert _same_bits(e, first[(k, occlusion)]), (i, k, occlusion, list(e["n_split"]), list(first[(k, occlusion)]["n_split"]))
    assert len(first) == 4
    for level, k, occlusion in ((2, 2, 2), (0, 3, 2), (2, 3, 1), (0, 2, 1)):
        e = reg.eval(level, poses[k], 2, occlusion)
        _, sp, sd, n_p, n_d = ora.error_occ(level, poses[k], 2, occlusion)
        _, _, Hd, gd, nvis = ora.hessgrad_occ(level, poses[k], 2, occlusion)
        assert list(e["n_split"]) == [n_p, n_d] and e["n_visible"] == nvis, (level, k, occlusion)
        _assert_sums(e, sp, sd, Hd, gd)
        if (k, occlusion) in first and level == 0:
            assert _same_bits(e, first[(k, occlusion)])
    reg.close()


def test_occlusion_generation_wrap_meets_stale_heads(hip_lib, oracle_mod):
    """RC.generation_wrap_schedule() on one fresh context: level 0 at the identity (generation 1 in every head up to 25250), 126 level-2
    passes that exchange only heads below 1550, then -- generation 1 again -- level 0 at the compressing pose with occlusion 2, the first
    pass to exchange the heads from 1550 up since pass 1; the same once more into occlusion 1 at the sideways pose.  If the head array
    were not cleared at the wrap, at least 16053 and 20968 of those heads (test_generation_wrap_schedule_meets_stale_heads, on the
    oracle alone) would decode as earlier runs of the current pass and be linked into its lists.  Every pass: counts exact and sums
    within tolerance against the oracle; a repeated (level, pose, mode) reproduces its first result bit for bit."""
    reg, ora, T = _pair_ctx(hip_lib, oracle_mod, RC.spherical_pair(250, 101), n_pyr=3)
    poses = synth.occlusion_test_poses(T)
    first = {}
    for j, (level, k, occlusion) in enumerate(RC.generation_wrap_schedule()):
        e = reg.eval(level, poses[k], 2, occlusion)
        if (level, k, occlusion) in first:
            assert _same_bits(e, first[(level, k, occlusion)]), (j, level, k, occlusion, list(e["n_split"]))
            continue
        first[(level, k, occlusion)] = e
        _, sp, sd, n_p, n_d = ora.error_occ(level, poses[k], 2, occlusion)
        _, _, Hd, gd, nvis = ora.hessgrad_occ(level, poses[k], 2, occlusion)
        assert list(e["n_split"]) == [n_p, n_d] and e["n_visible"] == nvis, (j, level, k, occlusion, list(e["n_split"]), n_p, n_d, e["n_visible"], nvis)
        _assert_sums(e, sp, sd, Hd, gd)
    assert len(first) == 4 + 4          # four level-2 (pose, mode) pairs, four level-0 passes
    reg.close()


def test_occlusion_sequence_route_at_250x101(hip_lib):
    """alignSequence with occlusion 2 / PHOTO_DEPTH on three 250x101 frames (the per-context route): pair by pair bit-equal to single
    alignments, as test_occlusion_sequence_with_the_default_inflight_equals_pairwise at 256x128."""
    frames = list(RC.spherical_frames())
    reg = _mk(hip_lib, 3)
    p, s, i = reg.alignSequence(frames, method=2, occlusion=2)
    one = _mk(hip_lib, 3)
    for j in range(len(frames) - 1):
        one.setTargetFrame(*frames[j]); one.setSourceFrame(*frames[j + 1])
        assert one.alignFrames360(np.eye(4), 2, 2) == s[j]
        assert np.array_equal(one.getOptimalPose(), p[j]) and list(one.num_iterations) == list(i[j]), j
    assert sum(int(x) for x in i.sum(axis=1)) > 0
    one.close()
    reg.close()


def test_reference_arithmetic_warp_at_250x101(hip_lib, oracle_mod):
    """rgbd360_set_index_arithmetic(ctx, 1) at 250x101: every target index equals the oracle's math_mode 0 on every level and pose."""
    reg, ora, T = _pair_ctx(hip_lib, oracle_mod, RC.spherical_pair(250, 101), n_pyr=3, math_mode=0)
    reg.set_index_arithmetic(1)
    for level in range(3):
        for pose in _poses(T):
            got, want = reg.warp_indices(level, pose), ora.warp_indices(level, pose)
            assert (want[:, 0] >= 0).mean() > 0.5
            assert np.array_equal(got, want), (level, int((got != want).any(axis=1).sum()))
    reg.close()


# ---- pinhole passes at 250x187 (n = 46750, 11625, 2852; 250, 125 and 62 columns) ---------------------------------------------------
def _pinhole_ctx(hip_lib, oracle_mod, modes=(1, 1)):
    pair = RC.pinhole_pair()
    (rgbA, dA), (rgbB, dB), T, K = pair
    reg = _mk(hip_lib, 3, setMaskSeams=False)
    reg.setCameraMatrix(K)
    reg.setTargetFrame(rgbA, dA)
    reg.setSourceFrame(rgbB, dB)
    return reg, RC.pinhole_oracle(oracle_mod, pair, modes), T


def test_pinhole_levels_and_warp_indices_in_both_arithmetics(hip_lib, oracle_mod):
    reg, ora, T = _pinhole_ctx(hip_lib, oracle_mod)
    ora0 = RC.pinhole_oracle(oracle_mod, RC.pinhole_pair(), (0, 1))
    for level in range(3):
        assert reg.level_dims(level) == ora.level_dims(level)
    for mode, o in ((0, ora), (1, ora0)):
        reg.set_index_arithmetic(mode)
        for level in range(3):
            for pose in _poses(T):
                a, b = reg.warp_indices_pinhole(level, pose), o.warp_indices_pinhole(level, pose)
                assert (b[:, 0] >= 0).mean() > 0.5
                assert np.array_equal(a, b), (mode, level, int((a != b).any(axis=1).sum()))
    reg.close()


@pytest.mark.parametrize("occ", [0, 1, 2])
def test_pinhole_eval_parity_at_250x187(hip_lib, oracle_mod, occ):
    """The plain pass (occlusion 0) and the keys + walk passes (1, 2) for the three methods at the poses of _poses, the 0.6 m probe
    (lists of up to 4) and the 20 m push (lists of 249 / 218 / 197: the box scan at 250, 125 and 62 columns): counts and rows exact,
    sums as in test_pinhole_occlusion_eval_parity."""
    reg, ora, T = _pinhole_ctx(hip_lib, oracle_mod)
    longest = 0
    for level in range(3):
        for pose in list(_poses(T)) + [_pinhole_probe_pose(T), RC.pinhole_push_pose(T)]:
            longest = max(longest, RC.longest_list(ora.warp_indices_pinhole(level, pose)))
            for method in (0, 1, 2):
                e = reg.eval_pinhole(level, pose, method, occ)
                if occ == 0:
                    _, sp, sd, n_p, n_d = ora.error_pinhole(level, pose, method)
                    _, _, Hd, gd, nrows = ora.hessgrad_pinhole(level, pose, method)
                else:
                    _, sp, sd, n_p, n_d = ora.error_pinhole_occ(level, pose, method, occ)
                    _, _, Hd, gd, nrows = ora.hessgrad_pinhole_occ(level, pose, method, occ)
                assert list(e["n_split"]) == [n_p, n_d] and e["n_rows"] == nrows, (level, method, occ, list(e["n_split"]), n_p, n_d, e["n_rows"], nrows)
                _assert_sums(e, sp, sd, Hd, gd)
                if occ != 0 and method == 1:
                    assert not e["H64"].any()          # as written: both row sums test the photometric residual
    assert longest == 249
    reg.close()


def test_pinhole_alignments_at_250x187(hip_lib, oracle_mod):
    """alignFrames, PHOTO_DEPTH, occlusion 0, 1 and 2: the oracle's status (2 for occlusion 2, after [0, 4, 0] iterations: its error
    gate leaves no depth residual on the fine levels) and iteration counts; the pose by the pose rule.  And DEPTH_CONSISTENCY without
    occlusion, the alignment on which the oracle's two accumulations lie farthest apart (2.6e-4 m)."""
    reg, ora, T = _pinhole_ctx(hip_lib, oracle_mod)
    for occ, method, status in RC.PINHOLE_ALIGNMENTS:
        rc = reg.alignFrames(np.eye(4), method, occ)
        runs = RC.pinhole_alignments(oracle_mod, occ, method)
        st, iters = runs[(1, 1)][0], runs[(1, 1)][1]
        assert rc == st == status, (occ, method, rc, st)
        assert reg.num_iterations == iters, (occ, method, reg.num_iterations, iters)
        _assert_pose(f"pinhole 250x187 occ {occ} method {method}", reg.getOptimalPose(), runs, (PINHOLE_ROT_TOL_DEV, PINHOLE_TRANS_TOL_DEV))
    reg.close()


def test_pinhole_saliency_list_mode_at_250x187(hip_lib, oracle_mod):
    """test_pinhole_saliency_list_mode's body: the error sums over vSalientPixels, the normal equations over every pixel."""
    reg, ora, T = _pinhole_ctx(hip_lib, oracle_mod)
    plain = reg.eval_pinhole(1, T, 2)
    reg.useSaliency(True)
    ora.use_saliency(True, 0.01)
    for level in range(3):
        for pose in _poses(T):
            for method in (0, 1, 2):
                e = reg.eval_pinhole(level, pose, method)
                _, sp, sd, n_p, n_d = ora.error_pinhole_salient(level, pose, method)
                _, _, Hd, gd, nrows = ora.hessgrad_pinhole(level, pose, method)
                assert list(e["n_split"]) == [n_p, n_d] and e["n_rows"] == nrows, (level, method)
                assert abs(e["err2_split"][0] - sp) <= ERR2_RTOL * max(1.0, abs(sp)) and abs(e["err2_split"][1] - sd) <= ERR2_RTOL * max(1.0, abs(sd))
                assert np.abs(e["H64"] - Hd).max() <= HG_RTOL * np.abs(Hd).max()
    sal = reg.eval_pinhole(1, T, 2)
    assert sal["n_split"][0] < plain["n_split"][0] and np.array_equal(sal["H64"], plain["H64"])
    rc = reg.alignFrames(np.eye(4), 2)
    runs = RC.pinhole_alignments(oracle_mod, 0, 2, True)
    assert rc == runs[(1, 1)][0] == 0 and reg.num_iterations == runs[(1, 1)][1]
    _assert_pose("pinhole 250x187 salient list, method 2", reg.getOptimalPose(), runs, (PINHOLE_ROT_TOL_DEV, PINHOLE_TRANS_TOL_DEV))
    reg.useSaliency(False)
    assert list(reg.eval_pinhole(1, T, 2)["n_split"]) == list(plain["n_split"])
    reg.close()


# ---- the 8-sensor rig at 150x113 (n = 16950, 4200, 1036 per sensor) ----------------------------------------------------------------
def _gpu_rig():
    from rgbd360_amd.rig import RegisterDensePhotoICP
    f1, f2, M, Rt, K = RC.rig_pair()
    reg = RegisterDensePhotoICP(Rt, K, n_pyr=3)
    reg.setTargetFrame(f1)
    reg.setSourceFrame(f2)
    return reg, M


def _assert_rig_eval(reg, ora, level, T, method):
    e = reg.eval(level, T, method)
    err, sums = ora.error(level, T, method)
    _, _, Hd, gd, n = ora.hessgrad(level, T, method)
    assert list(e["n_split"]) == [int(sums[2]), int(sums[3])] and e["n_rows"] == n, (level, method, e["n_split"], sums, e["n_rows"], n)
    assert abs(e["err2"] - err) <= ERR2_RTOL * max(err, 1.0)
    assert np.abs(e["H64"] - Hd).max() <= HG_RTOL * np.abs(Hd).max()
    assert np.abs(e["g64"] - gd).max() <= HG_RTOL * max(np.abs(gd).max(), 1e-3 * np.abs(Hd).max())
    return e


def test_rig_eval_parity_at_150x113(hip_lib, oracle_mod):
    """test_rig_eval_parity's body (three methods, every level, the identity, the true motion and a perturbed pose), then the salient
    pixel list mode once at level 1."""
    reg, M = _gpu_rig()
    ora = RC.rig_oracle(oracle_mod, RC.rig_pair())
    rng = np.random.default_rng(4)
    poses = [np.eye(4), M, synth.make_pose(synth.rodrigues(rng.normal(size=3), 0.03), rng.normal(size=3) * 0.03)]
    for level in range(3):
        for T in poses:
            for method in (0, 1, 2):
                _assert_rig_eval(reg, ora, level, T, method)
    full = reg.eval(1, M, 2)
    reg.useSaliency(True)
    ora.use_saliency(True, 0.01)
    sal = _assert_rig_eval(reg, ora, 1, M, 2)
    assert 0 < sal["n_split"][0] < full["n_split"][0] and sal["n_rows"] < full["n_rows"]
    reg.useSaliency(False)
    assert list(reg.eval(1, M, 2)["n_split"]) == list(full["n_split"])
    reg.close()


@pytest.mark.parametrize("method", [0, 1, 2])
def test_rig_align_at_150x113(hip_lib, oracle_mod, method):
    """test_rig_align_matches_oracle's body; the pose against the device-arithmetic oracle by the pose rule.  Against the true motion the
    160x120 test asks 5e-4 rad / 2e-3 m, kept here for the single modalities; with PHOTO_DEPTH the ORACLE itself ends 2.1 mm from it at
    150x113 (a property of the coarser problem), so that case asks 2.5e-3 m, the bound test_ragged_cases_cpu.py holds the oracle to."""
    reg, M = _gpu_rig()
    assert reg.align(np.eye(4), method)
    runs = RC.rig_alignments(oracle_mod, method)
    st, iters, _, hessian = runs[(1, 1)]
    assert st == 0 and reg.num_iterations == iters          # same accept / reject / LM-retry sequence
    _assert_pose(f"rig 150x113 method {method}", reg.getPose(), runs, RIG_POSE_TOL_DEV)
    assert np.allclose(reg.getInfoMat(), hessian, rtol=1e-3, atol=1e-4 * np.abs(hessian).max())
    # the reference-faithful arithmetic (libm rounding, double projection, float accumulators): the north-star tolerance
    st0, _, pose0, _ = runs[(0, 0)]
    rot, trans = synth.pose_error(reg.getPose(), pose0)
    assert st0 == 0 and rot <= 1e-4 and trans <= 1e-3, (rot, trans)
    rot, trans = synth.pose_error(reg.getPose(), M)
    assert rot < 5e-4 and trans < RC.RIG_TRUTH_TRANS[method], (rot, trans)
    # bitwise reproducible (fixed-order reductions, no atomics)
    p1 = reg.getPose()
    assert reg.align(np.eye(4), method) and np.array_equal(p1, reg.getPose())
    reg.close()
