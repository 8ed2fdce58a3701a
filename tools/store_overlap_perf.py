"""Cost of the sensed-space overlap of stored frames (rgbd360_store_overlap / _all), in ONE run on one device:
    python tools/store_overlap_perf.py [--out profiles/store_overlap_perf.txt] [--width 2048] [--entries 32] [--reps 24] [--levels 3,0]
32 resident entries at 2048 x 1024, 4 pyramid levels, all 992 ordered pairs at the relative poses of the entries' world poses,
levels 3 and 0:
  (a) the all-pairs call: kernel time of the source-stationary kernel, and the whole call (host clock, through the Python mirror)
  (b) the list kernel on the same 992 pairs: kernel time, and the whole list call
  (c) 992 x the single-launch time of k_warp_indices at that level (rgbd360_time_warp_images, avg_us[3]): the floor of what a caller of
      rgbd360_warp_indices pays today before any upload or counting
Kernel times: HIP events on the store's stream around the launches of one call (rgbd360_store_time_overlap*, rgbd360_hip_diag.h), one
untimed repetition first; median and interquartile range over `reps` repetitions.  (a) and (b) alternate in rounds so that a drift of
the clock reaches both.  8 distinct rendered frames are cycled through the entries (entry e holds frame e % 8 at that frame's pose)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rgbd360_amd import _lib, synth
from rgbd360_amd.register import RegisterPhotoICP, pose_to_cm
from rgbd360_amd.store import OVERLAP_DTYPE, FrameStore

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--width", type=int, default=2048)
ap.add_argument("--entries", type=int, default=32)
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--levels", default="3,0")
args = ap.parse_args()
W, H, N, REPS = args.width, args.width // 2, args.entries, max(args.reps, 20)
N_PYR, UNIQ = 4, 8
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def sh(cmd):
    try:
        return subprocess.run(cmd, shell=True, capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception:
        return "?"


def stats(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return med, q3 - q1


say("box: %s | ROCm %s" % (sh("rocminfo | grep -m1 'Marketing Name.*MI' | sed 's/.*: *//'") or "?", sh("cat /opt/rocm/.info/version") or "?"))
say("%d entries at %d x %d, %d levels, %d ordered pairs, %d repetitions per figure, %d alternating rounds" % (N, W, H, N_PYR, N * (N - 1), REPS, args.rounds))
L = _lib.load()
reg = RegisterPhotoICP()
reg.setNumPyr(N_PYR)
uniq = [synth.render(synth.trajectory_pose(k, 7), W, H, 7) for k in range(UNIQ)]
st = FrameStore(reg, N, H, W)
st.put(list(range(N)), [uniq[e % UNIQ] for e in range(N)])
world = np.stack([synth.trajectory_pose(e % UNIQ, 7) for e in range(N)]).astype(np.float32)
entries = np.arange(N, dtype=np.int32)
world_cm = np.ascontiguousarray(world.transpose(0, 2, 1).reshape(-1))
say("store: %d entries x %.1f MB" % (N, st.entry_bytes / 1e6))

# (c) needs a one-pair context holding two of the frames
reg2 = RegisterPhotoICP()
reg2.setNumPyr(N_PYR)
reg2.setTargetFrame(*uniq[0])
reg2.setSourceFrame(*uniq[3])
T03 = np.linalg.inv(synth.trajectory_pose(0, 7)) @ synth.trajectory_pose(3, 7)

decision = {}
for level in [int(x) for x in args.levels.split(",")]:
    n_px = (H >> level) * (W >> level)
    compact = n_px >= 256 * 1024
    src_bytes = 8 if compact else 16
    par = _lib.OverlapParams()
    L.rgbd360_store_overlap_default_params(st._handle(), C.byref(par))
    par.level = level
    m, rel = st.overlap_matrix(entries, world, level=level)            # warm-up, and the pairs / poses of the list call
    pairs = [(a, b) for a in range(N) for b in range(N) if a != b]
    trg = np.ascontiguousarray([p[0] for p in pairs], np.int32)
    src = np.ascontiguousarray([p[1] for p in pairs], np.int32)
    poses = np.stack([rel[a, b] for a, b in pairs])
    poses_cm = np.ascontiguousarray(poses.transpose(0, 2, 1).reshape(-1))
    lst = st.overlap(pairs, poses=poses, level=level)
    same = m[~np.eye(N, dtype=bool)].tobytes() == lst.tobytes()
    out_m = np.zeros(N * N, OVERLAP_DTYPE)
    out_l = np.zeros(len(pairs), OVERLAP_DTYPE)
    us = np.zeros(REPS + 1, np.float32)
    k_all, k_all_list, k_list, c_all, c_list = [], [], [], [], []

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    for _ in range(args.rounds):
        for kernel, sink in ((1, k_all), (0, k_all_list)):
            rc = L.rgbd360_store_time_overlap_all(st._handle(), N, vp(entries), vp(world_cm), 0.0, C.byref(par), kernel, REPS + 1, vp(us), vp(out_m))
            assert rc == 0, rc
            sink.extend(us[1:].tolist())
        rc = L.rgbd360_store_time_overlap(st._handle(), len(pairs), vp(trg), vp(src), vp(poses_cm), C.byref(par), REPS + 1, vp(us), vp(out_l))
        assert rc == 0, rc
        k_list.extend(us[1:].tolist())
        for _ in range(REPS):
            t0 = time.perf_counter()
            st.overlap_matrix(entries, world, level=level)
            c_all.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            st.overlap(pairs, poses=poses, level=level)
            c_list.append((time.perf_counter() - t0) * 1e6)
    avg = (C.c_float * 4)()
    rc = L.rgbd360_time_warp_images(reg2._ctx(), level, pose_to_cm(T03).ctypes.data_as(C.c_void_p), 2, 50, avg)
    assert rc == 0, rc
    say()
    say("== level %d: %d x %d = %d px, source records %d B/px; all-pairs records byte-equal to the list call: %s" % (level, W >> level, H >> level, n_px, src_bytes, same))
    traffic_list = len(pairs) * n_px * (src_bytes + 4)
    traffic_all = N * n_px * src_bytes + len(pairs) * n_px * 4
    for name, v, traffic in (("(a) all-pairs entry, source-stationary kernel", k_all, traffic_all),
                             ("(b) list kernel, all-pairs entry's rows      ", k_all_list, traffic_list),
                             ("(b) list kernel, list entry                  ", k_list, traffic_list)):
        med, iqr = stats(v)
        say("  %s kernel %9.1f us (IQR %6.1f, n %d)  %7.3f us/pair  algorithmic traffic %7.1f MB -> %6.2f TB/s" %
            (name, med, iqr, len(v), med / len(pairs), traffic / 1e6, traffic / med / 1e6))
    for name, v in (("(a) whole rgbd360_store_overlap_all call (Python mirror)", c_all), ("(b) whole rgbd360_store_overlap call (Python mirror)    ", c_list)):
        med, iqr = stats(v)
        say("  %s %9.1f us (IQR %6.1f, n %d)" % (name, med, iqr, len(v)))
    say("  (c) k_warp_indices, one launch %.2f us -> x %d pairs = %.1f us (no upload, no counting)" % (avg[3], len(pairs), avg[3] * len(pairs)))
    ma, ia = stats(k_all)
    mb, ib = stats(k_all_list)
    decision[level] = (ma, ia, mb, ib)
    say("  mean n_consistent / px over the pairs: %.3f" % float(np.mean(lst["n_consistent"] / n_px)))

say()
say("== stop rule (source-stationary kernel ships only if at least as fast as the list kernel on the same pairs, no margin beyond the spread)")
for level, (ma, ia, mb, ib) in decision.items():
    say("  level %d: source-stationary %.1f us (IQR %.1f) vs list %.1f us (IQR %.1f): %s" %
        (level, ma, ia, mb, ib, "at least as fast" if ma <= mb else "slower"))
st.close()
reg.close()
reg2.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
