"""The inputs of the ragged-size tests (test_ragged_cases_cpu.py pins what they are on the oracle alone, test_ragged_passes_gpu.py
runs the device on them): sizes at which no pyramid level fills its last wave, rendered once per process and shared read-only.

    spherical  add_occluder(make_pair(250, 101, seed=21)), 3 levels   n = 25250, 6250, 1550   n % 64 = 34, 42, 14   n % 1024 = 674 at level 0
               add_occluder(make_pair(1000, 37, seed=21)), 2 levels   n = 37000, 9000         n % 64 = 8, 40
    pinhole    make_pinhole_pair(250, 187, seed=77), 3 levels         n = 46750, 11625, 2852  n % 64 = 30, 41, 36
    rig        make_rig_pair(150, 113, seed=3, 0.04 m, 1.5 deg)       n = 16950, 4200, 1036   n % 64 = 54, 40, 12

Test infrastructure only: input generation and oracle set-up, no alignment arithmetic."""
import functools

import numpy as np

from rgbd360_amd import synth

SPHERICAL = {(250, 101): 3, (1000, 37): 2}          # (W, H) -> pyramid levels
SPHERICAL_SEED = 21
PINHOLE = (250, 187, 77)                            # W, H, seed
RIG = dict(width=150, height=113, seed=3, trans=0.04, rot_deg=1.5)
ORACLE_MODES = ((0, 0), (0, 1), (1, 0), (1, 1))     # (math_mode, reduce_mode)
OCC_ALIGNMENTS = ((1, 2), (2, 0), (2, 1), (2, 2))   # (occlusion, method) of the spherical alignments
PINHOLE_ALIGNMENTS = ((0, 2, 0), (1, 2, 0), (2, 2, 2), (0, 1, 0))      # (occlusion, method, status) of the pinhole alignments
RIG_TRUTH_TRANS = {0: 2e-3, 1: 2e-3, 2: 2.5e-3}     # m against the true motion per method: test_rig_dense.py's 2 mm; PHOTO_DEPTH: the oracle ends 2.1 mm off
PINHOLE_PUSH = 20.0                                 # the pose of test_pinhole_occlusion_long_arrival_lists that piles hundreds of pixels on one
PINHOLE_PROBE = 0.6                                 # _pinhole_probe_pose of tests/test_gpu_parity.py


def _freeze(frames):
    for rgb, d in frames:
        rgb.setflags(write=False)
        d.setflags(write=False)


@functools.lru_cache(maxsize=None)
def spherical_pair(W, H):
    pair = synth.add_occluder(synth.make_pair(W, H, seed=SPHERICAL_SEED))
    _freeze(pair[:2])
    return pair


@functools.lru_cache(maxsize=None)
def spherical_frames(W=250, H=101, n=3, seed=11):
    """Three consecutive frames of the synthetic trajectory (the sequence route aligns frame j+1 onto frame j)."""
    frames = tuple(synth.render(synth.trajectory_pose(k, seed), W, H, seed) for k in range(n))
    _freeze(frames)
    return frames


@functools.lru_cache(maxsize=None)
def pinhole_pair():
    pair = synth.make_pinhole_pair(PINHOLE[0], PINHOLE[1], seed=PINHOLE[2])
    _freeze(pair[:2])
    return pair


@functools.lru_cache(maxsize=None)
def rig_pair():
    pair = synth.make_rig_pair(**RIG)
    _freeze(pair[0])
    _freeze(pair[1])
    return pair


def schedule_guess():
    """The non-identity start of test_occlusion_fused_schedule_equals_the_three_launch_one."""
    return synth.make_pose(synth.rodrigues(np.array([0.0, 1.0, 0.0]), 0.004), np.array([0.01, 0.0, -0.005]))


def pinhole_push_pose(T, push=PINHOLE_PUSH):
    P = np.eye(4)
    P[2, 3] = push
    return P @ T


def spherical_oracle(O, pair, n_pyr, modes=(1, 1)):
    (rgbA, dA), (rgbB, dB), _ = pair
    ora = O.Oracle(n_pyr=n_pyr, math_mode=modes[0], reduce_mode=modes[1])
    ora.set_target(rgbA, dA)
    ora.set_source(rgbB, dB)
    return ora


def pinhole_oracle(O, pair, modes=(1, 1), saliency=False):
    (rgbA, dA), (rgbB, dB), _, K = pair
    ora = O.Oracle(n_pyr=3, math_mode=modes[0], reduce_mode=modes[1], mask_seams=0)
    ora.set_camera(*K)
    ora.set_target(rgbA, dA)
    ora.set_source(rgbB, dB)
    if saliency:
        ora.use_saliency(True, 0.01)
    return ora


def rig_oracle(O, pair, modes=(1, 1)):
    f1, f2, _, Rt, K = pair
    rig = O.RigOracle(Rt, K, n_pyr=3, math_mode=modes[0], reduce_mode=modes[1])
    for s in range(len(Rt)):
        rig.set_frame(s, True, *f1[s])
        rig.set_frame(s, False, *f2[s])
    return rig


def longest_list(idx):
    """The most source pixels that land on one target pixel; idx = warp_indices (row, column per source pixel, -1 = not visible)."""
    v = idx[:, 0] >= 0
    return int(np.unique(idx[v, 0] * 4096 + idx[v, 1], return_counts=True)[1].max()) if v.any() else 0


def pose_bound(constants, spread, factor=4.0):
    """The pose rule of the ragged-size tests: (rotation, translation) bounds = max(the suite's constant, 4 x the oracle's own distance
    between float32 and float64 accumulation at this input).  4: the device adds float32 partial sums in a third order."""
    return max(constants[0], factor * spread[0]), max(constants[1], factor * spread[1])


# ---- the alignments the device tests run, on the oracle in its four arithmetic settings: {modes: (status, iterations, pose[, H])} ----
@functools.lru_cache(maxsize=None)
def spherical_alignments(O, W, H, occlusion, method, from_guess=False):
    n_pyr = SPHERICAL[(W, H)]
    ora = spherical_oracle(O, spherical_pair(W, H), n_pyr)
    start = schedule_guess() if from_guess else np.eye(4)
    out = {}
    for modes in ORACLE_MODES:
        ora.set_modes(*modes)
        st, pose = ora.align360(start, method, occlusion)
        out[modes] = (st, list(ora.result.iters)[:n_pyr], pose)
    return out


@functools.lru_cache(maxsize=None)
def pinhole_alignments(O, occlusion, method, saliency=False):
    out = {}
    for modes in ORACLE_MODES:
        ora = pinhole_oracle(O, pinhole_pair(), modes, saliency)
        st, pose = ora.align_pinhole(np.eye(4), method, occlusion)
        out[modes] = (st, list(ora.result.iters)[:3], pose)
    return out


@functools.lru_cache(maxsize=None)
def rig_alignments(O, method):
    out = {}
    for modes in ORACLE_MODES:
        rig = rig_oracle(O, rig_pair(), modes)
        st, pose = rig.align(np.eye(4), method)
        out[modes] = (st, list(rig.iters), pose, rig.hessian)
    return out


def reduce_spread(runs):
    """(rad, m) between the oracle's float32-accumulator and float64-accumulator alignments in the device's index arithmetic."""
    return synth.pose_error(runs[(1, 0)][2], runs[(1, 1)][2])


# ---- the generation of the occlusion list heads (kOccGenMax of csrc/occlusion_kernels.h; one memset of the head array per wrap) ----
OCC_GENERATIONS = 127


def generation_wrap_schedule():
    """[(level, index into occlusion_test_poses, occlusion)], one entry per occlusion evaluation of ONE fresh 250x101 context, pass j
    (from 1) carrying generation ((j - 1) % 127) + 1.  Pass 1 runs level 0 at the identity with occlusion 1: every valid pixel heads its
    own list, generation 1.  Passes 2..127 run level 2, which exchanges only heads below its 1550 pixels.  Pass 128 -- generation 1 again,
    behind the memset -- is the first to exchange the level-0 heads from 1550 up since pass 1, at another pose and in the other mode;
    passes 129..254 run level 2 again and pass 255 (generation 1) returns to level 0.  Without the memset the heads that pass 1 (and
    128) left would decode as runs of the current pass.  Two more passes end the schedule at level 2 and level 0."""
    def fill(j):
        return (2, j % 4, 1 + j % 2)
    n = OCC_GENERATIONS - 1
    return [(0, 0, 1)] + [fill(j) for j in range(n)] + [(0, 3, 2)] + [fill(j) for j in range(n)] + [(0, 2, 1), (2, 1, 2), (0, 1, 2)]


def distinct_targets(idx, cols):
    """The head indices a pass over the candidates `idx` (warp_indices) exchanges: row * cols + column of every visible pixel."""
    v = idx[:, 0] >= 0
    return np.unique(idx[v, 0].astype(np.int64) * cols + idx[v, 1])
