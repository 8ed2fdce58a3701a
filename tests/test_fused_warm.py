"""The fused launch (k_eval_fs) lets the waves the solve leaves idle request the target lines of the pass's first two steps at the pose
of the PENDING pass, and drops what arrives (photo_icp_kernels.h, WarmFirstGathers).  That may change no result: this file pins "same
as before" -- the fused schedule against the two-launch schedule (rgbd360_debug_set_schedule: k_eval + k_solve, which has no warm-up),
bit for bit -- at the places where the warm-up is all or more than the span, hits nothing, or asks for records off the image.  Only
entry points the library had before the warm-up are used: the GPU cases pass without it as well (they were run on the commit before).

Sizes (one block = 1024 pixels per step):
  32 x 16     one block, a partial first step, the second step wholly past the span
  80 x 40     ragged: 3200 pixels, the last block short
  256 x 128   three levels: hand-overs between levels (the launch behind a hand-over solves another level's pass and must not warm)
  1280 x 640  two levels: level 0 has spans of four steps, the shortest the shipped warm-up takes part in (kWarmMinSteps; the three
              sizes above are the ones it stays out of, and the ones a build with RGBD360_WARM_SHORT_SPANS warms), level 1 spans of one
Methods 0 (photo) and 2 (photo + depth).  A forced schedule compares pose, status and error; an alignment also the per-level iteration
counts and the H / g of the result record.

The last case needs no GPU: the machine code of k_eval_fs<0,0>.  PARENT_LOADS_PER_INTERVAL is the number of buffer loads between
consecutive s_barrier instructions of the kernel's text (in front of the first, ..., behind the last) as written down from the commit
before the warm-up: [0, 0, 2, 0, 11, 0] -- the two source records of the span's first steps behind the staging barriers, the loop's
loads between the barrier behind the solve and the reduction's.  The warm-up's code lies behind wave 1's in the text (the solve's
fall-through path stays what tests/test_solve_path_isa.py pins), so its loads are found the way an idle wave reaches them: from the
barrier behind solve_totals through the exit the waves other than wave 1 take, then in textual order.  PARENT_LOADS_ON_IDLE_PATH = 0."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import build as B  # noqa: E402
from rgbd360_amd import synth  # noqa: E402

gpu = pytest.mark.gpu

PARENT_LOADS_PER_INTERVAL = [0, 0, 2, 0, 11, 0]
PARENT_LOADS_ON_IDLE_PATH = 0
KERNEL = "_ZN4r3609k_eval_fsILi0ELi0EEE"

SIZES = {"32x16": (32, 16, 1), "80x40": (80, 40, 1), "256x128": (256, 128, 3), "1280x640": (1280, 640, 2)}      # cols, rows, pyramid levels


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(4)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


class Pair:
    """One synthetic pair in two contexts: the fused schedule (the library's default) and the two-launch schedule."""

    def __init__(self, cols, rows, n_pyr):
        from rgbd360_amd.register import RegisterPhotoICP
        (rgbA, dA), (rgbB, dB), self.truth = synth.make_pair(cols, rows, seed=3)
        self.regs = []
        for fused in (True, False):
            r = RegisterPhotoICP()
            r.setNumPyr(n_pyr)
            r.debug_set_schedule(fused_solve=fused, fused_occ=fused)
            r.setTargetFrame(rgbA, dA)
            r.setSourceFrame(rgbB, dB)
            self.regs.append(r)

    def forced(self, level, pose0, method, k, fold_init):
        """K forced iterations on both schedules; fold_init: the fused schedule's first launch initialises the state itself (init.on)."""
        return [r.forced_iters(level, pose0, method, k, want_elapsed=not fold_init) for r in self.regs]

    def align(self, guess, method):
        out = []
        for r in self.regs:
            rc = r.alignFrames360(guess, method)
            out.append(dict(status=rc, pose=r.getOptimalPose().copy(), iters=list(r.num_iterations), H=r.getHessian().copy(), g=r.getGradient().copy()))
        return out


@pytest.fixture(scope="module")
def pairs(hip_lib):
    return {name: Pair(*dims) for name, dims in SIZES.items()}


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _same_forced(a, b, what):
    assert a["status"] == b["status"], (what, a["status"], b["status"])
    assert np.array_equal(_bits(a["pose"]), _bits(b["pose"])), (what, a["pose"], b["pose"])
    assert np.float64(a["rms"]).view(np.uint64) == np.float64(b["rms"]).view(np.uint64), (what, a["rms"], b["rms"])


def _same_align(a, b, what):
    assert a["status"] == b["status"], (what, a["status"], b["status"])
    assert a["iters"] == b["iters"], (what, a["iters"], b["iters"])
    for k in ("pose", "H", "g"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, a[k], b[k])


@gpu
@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("size", list(SIZES))
def test_small_spans(pairs, size, method):
    """The warm-up's two steps are all of the span, or more."""
    p = pairs[size]
    n_pyr = SIZES[size][2]
    a, b = p.align(np.eye(4), method)
    _same_align(a, b, (size, method, "alignment"))
    for level in range(n_pyr):
        for fold_init in (False, True):
            a, b = p.forced(level, np.eye(4), method, 4, fold_init)
            _same_forced(a, b, (size, method, level, fold_init))


@gpu
@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("size", ["256x128", "1280x640"])
def test_far_start_guess(pairs, size, method):
    """30 degrees and 0.5 m off the truth: the first steps are many pixels, the warm-up hits nothing and changes nothing.  The natural
    schedule rejects steps on the way: the launch behind a finished level is a no-op."""
    p = pairs[size]
    off = _rot(1, 30.0)
    off[:3, 3] = (0.3, -0.3, 0.264575)        # |t| = 0.5
    guess = p.truth @ off
    a, b = p.forced(0, guess, method, 6, False)
    _same_forced(a, b, (size, method, "forced"))
    a, b = p.forced(0, guess, method, 6, True)
    _same_forced(a, b, (size, method, "forced, folded initialisation"))
    a, b = p.align(guess, method)
    _same_align(a, b, (size, method, "alignment"))


@gpu
@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("size", ["80x40", "256x128", "1280x640"])
def test_old_pose_indices_off_the_image(pairs, size, method):
    """Finite poses at which the source points leave the target image or land on its poles and seam: quarter and half turns about each
    axis, 5 m away.  K = 3 forced iterations."""
    p = pairs[size]
    for axis in range(3):
        for deg in (90.0, 180.0):
            for t in ((5.0, 0, 0), (0, -5.0, 0), (0, 0, 5.0)):
                pose = _rot(axis, deg)
                pose[:3, 3] = t
                a, b = p.forced(0, pose, method, 3, False)
                _same_forced(a, b, (size, method, axis, deg, t))
    pose = _rot(0, 180.0)
    pose[:3, 3] = (5.0, 5.0, -5.0)
    a, b = p.forced(0, pose, method, 3, True)
    _same_forced(a, b, (size, method, "folded initialisation"))


# ---- the machine code (no GPU) ----
def _hipcc():
    import shutil
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def _instr(line):
    t = line.split(";")[0].strip()
    return t if t and not t.endswith(":") and not t.startswith(".") else ""


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is absent: no ISA to read")
def test_idle_waves_issue_loads_during_the_solve(tmp_path):
    out = str(tmp_path / "api.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-pthread")]
    subprocess.check_call([_hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, B.SRC], stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    st = [i for i, l in enumerate(lines) if l.startswith(KERNEL) and l.split(";")[0].strip().endswith(":")][0]
    end = [i for i in range(st, len(lines)) if lines[i].startswith(".Lfunc_end")][0]
    body = lines[st:end]
    ins = [(i, _instr(l)) for i, l in enumerate(body)]
    ins = [(i, t) for i, t in ins if t]
    bars = [k for k, (_, t) in enumerate(ins) if t.startswith("s_barrier")]
    loads = [k for k, (_, t) in enumerate(ins) if t.startswith("buffer_load")]
    edges = [-1] + bars + [len(ins)]
    per_interval = [sum(a < k < b for k in loads) for a, b in zip(edges, edges[1:])]
    print("buffer loads per barrier interval", per_interval, "at the parent", PARENT_LOADS_PER_INTERVAL)
    assert len(per_interval) == len(PARENT_LOADS_PER_INTERVAL)
    # nothing new in front of the solve or on wave 1's stretch of the text
    assert per_interval[:4] == PARENT_LOADS_PER_INTERVAL[:4]
    # the idle waves' path: the barrier behind solve_totals (the last in front of the first v_readlane_b32, as in test_solve_path_isa),
    # the first conditional branch behind it (wave 1 falls through, every other wave takes it), then textual order
    lanes = [k for k, (_, t) in enumerate(ins) if t.startswith("v_readlane_b32")]
    first = max(b for b in bars if b < lanes[0])
    k = first + 1
    while not ins[k][1].startswith("s_cbranch"):
        assert not re.match(r"s_barrier|s_branch\b|s_endpgm", ins[k][1])
        k += 1
    target = ins[k][1].split()[-1]
    at = [i for i, l in enumerate(body) if l.split(";")[0].strip() == target + ":"]
    assert len(at) == 1, target
    on_path = 0
    for i, t in ins:
        if i <= at[0]:
            continue
        if re.match(r"s_barrier|s_branch\b|s_setpc|s_endpgm", t):
            break
        on_path += t.startswith("buffer_load")
    print("buffer loads on the idle waves' path", on_path, "at the parent", PARENT_LOADS_ON_IDLE_PATH)
    assert on_path >= PARENT_LOADS_ON_IDLE_PATH + 1
    # ... and they are new loads, not the loop's moved
    assert sum(per_interval) == sum(PARENT_LOADS_PER_INTERVAL) + on_path
