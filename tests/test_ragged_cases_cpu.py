"""What tests/test_ragged_passes_gpu.py assumes about its inputs, pinned on the CPU oracle alone (no GPU): the level sizes leave every
last wave partly filled, the occluder produces real z-buffer conflicts at these sizes, the pinhole push pose overflows the slot rows so
that the box scans run with odd `cols`, and every alignment the device tests compare walks ONE accept / reject sequence in the
oracle's four arithmetic settings -- otherwise an equal-iterations assertion against the device would hinge on rounding, not on the
code under test.  A case whose sequence differs between the settings is not a valid input: choose another seed and re-check it here."""
import os
import re

import numpy as np
import pytest

from rgbd360_amd import synth
from tests import ragged_cases as RC


def _level_sizes(ora, n_pyr):
    dims = [ora.level_dims(level) for level in range(n_pyr)]
    return dims, [r * c for r, c in dims]


@pytest.fixture(scope="module")
def sph_250(oracle_mod):
    pair = RC.spherical_pair(250, 101)
    return pair, RC.spherical_oracle(oracle_mod, pair, 3)


@pytest.fixture(scope="module")
def sph_1000(oracle_mod):
    pair = RC.spherical_pair(1000, 37)
    return pair, RC.spherical_oracle(oracle_mod, pair, 2)


@pytest.fixture(scope="module")
def pin_250(oracle_mod):
    pair = RC.pinhole_pair()
    return pair, RC.pinhole_oracle(oracle_mod, pair)


def test_spherical_250x101_levels_leave_partly_filled_waves(sph_250):
    dims, n = _level_sizes(sph_250[1], 3)
    assert dims == [(101, 250), (50, 125), (25, 62)]
    assert n == [25250, 6250, 1550]
    assert [v % 64 for v in n] == [34, 42, 14]
    assert n[0] % 1024 == 674          # the last step of the last 1024-thread block of the pass ends inside a wave


def test_spherical_1000x37_levels_leave_partly_filled_waves(sph_1000):
    dims, n = _level_sizes(sph_1000[1], 2)
    assert dims == [(37, 1000), (18, 500)]
    assert n == [37000, 9000]
    assert [v % 64 for v in n] == [8, 40]


def _occlusion_counts(ora, level, pose, occlusion):
    _, _, _, n_p, n_d = ora.error_occ(level, pose, 2, occlusion)
    return (n_p, n_d), ora.hessgrad_occ(level, pose, 2, occlusion)[4]


def test_spherical_250x101_occluder_makes_conflicts_on_every_level(sph_250):
    """The lists reach four source pixels per target pixel, and at every level both occlusion modes count differently from the plain
    pass at every pose that moves the pixels: a device pass that ignored its lists could not produce the oracle's counts.  At the
    identity every source pixel lands on its own target pixel (longest list 1), so occlusion 1 counts what the plain pass counts
    (15833 + 14622 = 30455 at level 0) and only occlusion 2, through its depth gate, differs there."""
    (_, _, T), ora = sph_250
    longest = 0
    for level in range(3):
        ora.prepare_level(level)
        for k, pose in enumerate(synth.occlusion_test_poses(T)):
            longest = max(longest, RC.longest_list(ora.warp_indices(level, pose)))
            _, _, n_valid = ora.error(level, pose, 2)
            n_visible = ora.hessgrad(level, pose, 2)[4]
            for occlusion in (1, 2):
                n_split, n_vis_occ = _occlusion_counts(ora, level, pose, occlusion)
                if k == 0 and occlusion == 1:
                    assert sum(n_split) == n_valid and n_vis_occ == n_visible
                    continue
                assert sum(n_split) != n_valid, (level, k, occlusion, n_split, n_valid)
                if occlusion == 2:                    # (occlusion 1's H, g pass never rejects: its numVisible is the plain one)
                    assert n_vis_occ != n_visible, (level, k, n_vis_occ, n_visible)
    assert longest == 4
    # the figures of level 0 at the identity, occlusion 1 / PHOTO_DEPTH
    ora.prepare_level(0)
    n_split, n_vis = _occlusion_counts(ora, 0, np.eye(4), 1)
    assert n_split == (15833, 14622) and n_vis == 25149
    assert ora.error(0, np.eye(4), 2)[2] == 30455


def test_spherical_1000x37_occluder_makes_conflicts_on_every_level(sph_1000):
    (_, _, T), ora = sph_1000
    longest = 0
    for level in range(2):
        ora.prepare_level(level)
        for k, pose in enumerate(synth.occlusion_test_poses(T)):
            longest = max(longest, RC.longest_list(ora.warp_indices(level, pose)))
            _, _, n_valid = ora.error(level, pose, 2)
            for occlusion in (1, 2):
                n_split, _ = _occlusion_counts(ora, level, pose, occlusion)
                assert (sum(n_split) != n_valid) == (k > 0 or occlusion == 2), (level, k, occlusion, n_split, n_valid)
    assert longest == 4


def test_pinhole_250x187_levels_and_list_lengths(pin_250):
    (_, _, T, _), ora = pin_250
    dims, n = _level_sizes(ora, 3)
    assert dims == [(187, 250), (93, 125), (46, 62)]
    assert n == [46750, 11625, 2852]
    assert [v % 64 for v in n] == [30, 41, 36]
    push = RC.pinhole_push_pose(T)
    # beyond the 8 slots of a target pixel: the walk scans the box of the arrivals, at 250, 125 and 62 columns
    assert [RC.longest_list(ora.warp_indices_pinhole(level, push)) for level in range(3)] == [249, 218, 197]
    probe = RC.pinhole_push_pose(T, RC.PINHOLE_PROBE)
    assert max(RC.longest_list(ora.warp_indices_pinhole(level, probe)) for level in range(3)) == 4


def test_generation_wrap_schedule_meets_stale_heads(sph_250):
    """What makes RC.generation_wrap_schedule() binding, from the oracle's target indices: a pass that exchanges the heads of ANOTHER
    pass of its own generation for the first time since.  (The plain schedule of 259 level-0 evaluations cycling four (pose, mode)
    pairs cannot: every head it exchanges was written four passes earlier.)  A head `meets its generation` when the last pass that wrote
    it carried the generation of the pass that now exchanges it -- without the memset of the wrap, occ_store_node would decode it as an
    earlier run of the current pass and link a phantom node.  With the memset every head is 0 (generation 0) at passes 128 and 255."""
    (_, _, T), ora = sph_250
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rgbd360_amd", "csrc", "occlusion_kernels.h")) as f:
        assert int(re.search(r"constexpr int kOccGenMax = (\d+);", f.read()).group(1)) == RC.OCC_GENERATIONS == 127
    sched = RC.generation_wrap_schedule()
    gen = [j % RC.OCC_GENERATIONS + 1 for j in range(len(sched))]          # of pass j + 1
    level0 = [j for j, (level, _, _) in enumerate(sched) if level == 0]
    assert level0 == [0, 127, 254, 256] and [gen[j] for j in level0[:3]] == [1, 1, 1] and len(sched) == 2 * 127 + 3
    assert all(level == 2 for level, _, _ in sched[1:127] + sched[128:254])
    assert sched[0] == (0, 0, 1) and sched[127] == (0, 3, 2) and sched[254] == (0, 2, 1)
    (rows, cols), (r2, c2) = ora.level_dims(0), ora.level_dims(2)
    n0, n2 = rows * cols, r2 * c2
    assert (n0, n2) == (25250, 1550)                     # a level-2 pass exchanges heads below 1550 only
    poses = synth.occlusion_test_poses(T)
    ora.prepare_level(0)
    # occlusion 1: the candidates are the visible pixels of warp_indices (its H, g pass counts every candidate)
    idx1 = ora.warp_indices(0, poses[0])
    assert int((idx1[:, 0] >= 0).sum()) == ora.hessgrad_occ(0, poses[0], 2, 1)[4]
    S1 = RC.distinct_targets(idx1, cols)                  # heads that carry generation 1 behind pass 1
    S1_high = S1[S1 >= n2]                                # ... and that no pass before 128 exchanges
    assert len(S1) == 25149 and len(S1_high) > 20000
    # pass 128, occlusion 2: it exchanges one head per target pixel with a gated candidate = numVisible of its H, g pass
    exchanged_128 = ora.hessgrad_occ(0, poses[3], 2, 2)[4]
    met_128 = exchanged_128 - n2 - (n0 - len(S1))        # at least: not below 1550, not among the heads pass 1 left alone
    assert exchanged_128 == 17704 and met_128 >= 16053
    # pass 255, occlusion 1: heads from 1550 up were last written by pass 1 or pass 128, both generation 1
    idx255 = ora.warp_indices(0, poses[2])
    assert int((idx255[:, 0] >= 0).sum()) == ora.hessgrad_occ(0, poses[2], 2, 1)[4]
    met_255 = len(np.intersect1d(RC.distinct_targets(idx255, cols), S1_high))
    assert met_255 > 15000, met_255
    print(f"generation wrap: without the memset at least {met_128} heads at pass 128 and {met_255} at pass 255 would decode as current")


def test_rig_150x113_levels_leave_partly_filled_waves(oracle_mod):
    """RigOracle has no level_dims: the level sizes are the halving rule restated here (RPI.h:300-333), not read from the oracle; the
    oracle side is held only loosely (a pass has rows, and never more than two per pixel and sensor).  The device's own level sizes
    are held by the exact counts of test_rig_eval_parity_at_150x113."""
    f1 = RC.rig_pair()[0]
    rows, cols = f1[0][1].shape
    assert (rows, cols) == (113, 150) and len(f1) == 8
    n = [(rows >> level) * (cols >> level) for level in range(3)]          # (the pyramid halves with floor: RPI.h:300-333)
    assert n == [16950, 4200, 1036]
    assert [v % 64 for v in n] == [54, 40, 12]
    # the oracle's own level sizes, through the Jacobian-row count of a pass: never more rows than 2 per pixel and sensor
    rig = RC.rig_oracle(oracle_mod, RC.rig_pair())
    for level in range(3):
        assert 0 < rig.hessgrad(level, np.eye(4), 2)[4] <= 2 * 8 * n[level]


def _assert_one_sequence(runs, what):
    ref = runs[(1, 1)]
    for modes, run in runs.items():
        status, iters = run[0], run[1]
        assert (status, iters) == (ref[0], ref[1]), (what, modes, status, iters, ref[0], ref[1])
    return ref[0], ref[1]


@pytest.mark.parametrize("from_guess", [False, True])
@pytest.mark.parametrize("occlusion,method", RC.OCC_ALIGNMENTS)
def test_spherical_250x101_alignments_walk_one_sequence(oracle_mod, occlusion, method, from_guess):
    runs = RC.spherical_alignments(oracle_mod, 250, 101, occlusion, method, from_guess)
    status, iters = _assert_one_sequence(runs, ("spherical", occlusion, method, from_guess))
    assert status == 0 and sum(iters) >= 2
    rot, trans = RC.reduce_spread(runs)
    print(f"250x101 occ {occlusion} method {method} guess {from_guess}: iterations {iters}, float32 vs float64 sums {rot:.2e} rad {trans:.2e} m")


@pytest.mark.parametrize("occlusion,method,status", RC.PINHOLE_ALIGNMENTS)
def test_pinhole_250x187_alignments_walk_one_sequence(oracle_mod, occlusion, method, status):
    """Occlusion 2 ends with status 2 (its error gate compares the target depth with the point's INVERSE depth, RPI.h:1687-1690: no
    depth residual on the fine levels) after four iterations on level 1 -- on both sides, which is what the device test asserts."""
    runs = RC.pinhole_alignments(oracle_mod, occlusion, method)
    st, iters = _assert_one_sequence(runs, ("pinhole", occlusion, method))
    assert st == status and sum(iters) >= 3
    rot, trans = RC.reduce_spread(runs)
    print(f"pinhole 250x187 occ {occlusion} method {method}: status {st}, iterations {iters}, float32 vs float64 sums {rot:.2e} rad {trans:.2e} m")


def test_pinhole_250x187_salient_list_alignment_walks_one_sequence(oracle_mod):
    runs = RC.pinhole_alignments(oracle_mod, 0, 2, True)
    st, iters = _assert_one_sequence(runs, "pinhole salient list")
    assert st == 0 and sum(iters) >= 3


@pytest.mark.parametrize("method", [0, 1, 2])
def test_rig_150x113_alignments_walk_one_sequence(oracle_mod, method):
    runs = RC.rig_alignments(oracle_mod, method)
    st, iters = _assert_one_sequence(runs, ("rig", method))
    assert st == 0 and sum(iters) >= 2
    # the registration recovers the 0.04 m / 1.5 degree motion at this size too: to 5e-4 rad / 2 mm as at 160x120 with one modality;
    # with PHOTO_DEPTH the oracle itself ends 2.1 mm from it (the pixels are 7 % larger): 2.5 mm there
    for modes in ((0, 0), (1, 1)):
        rot, trans = synth.pose_error(runs[modes][2], RC.rig_pair()[2])
        assert rot < 5e-4 and trans < RC.RIG_TRUTH_TRANS[method], (modes, rot, trans)
    rot, trans = RC.reduce_spread(runs)
    print(f"rig 150x113 method {method}: iterations {iters}, float32 vs float64 sums {rot:.2e} rad {trans:.2e} m")
