"""The map pyramid on the device: what a level costs to build, next to one scan of the same table, and what a coarse-to-fine alignment
costs next to the same chain run by hand over four separately inserted maps.

    python tools/map_pyramid_perf.py [--voxels 100000,1000000] [--frame 2048x1024] [--reps 15] [--rounds 3] [--leaf 0.05]
                                     [--out profiles/map_pyramid_perf.txt]

  * the level build (rgbd360_map_time_coarsen: HIP events, averages over --reps builds, medians over --rounds calls after an untimed one):
    levels 1, 2, 3 each -- the clear of the level's table and of the counters and one k_vmap_coarsen launch over the level below -- and
    the three back to back, on a surface of --voxels voxels (one point per cell on z = 0.3 sin x cos y, the table twice the voxels
    rounded up to a power of two), next to ONE k_vmap_extract launch over the parent's table, the cost of merely scanning it;
  * rgbd360_map_align_c2f_sphere with top_shift 3 of a --frame synthetic frame against a map that holds it, from a guess 0.15 m / 0.03 rad
    off, host wall clock per call (medians over reps x rounds calls; levels warm), from host and from device memory, next to the four
    single-level rgbd360_map_align_sphere calls of the same chain on four maps inserted at leaf x 8, 4, 2, 1 (existing code: the
    yardstick), and next to the first c2f call after the map was written, which rebuilds the three levels.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rgbd360_amd import _lib, synth                                  # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP, pose_to_cm, _ptr  # noqa: E402
from rgbd360_amd.voxel_map import VoxelMap                           # noqa: E402
from map_normals_perf import surface_cloud                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", default="100000,1000000")
    ap.add_argument("--frame", default="2048x1024")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("rgbd360_map_level / rgbd360_map_align_c2f_*: leaf %.3f m, default parameters, microseconds" % a.leaf)
    say("(the clock state is not read: the spread between the minimum and the maximum of each figure stands for it)")
    reg = RegisterPhotoICP()
    L = _lib.load()
    eye = np.eye(4, dtype=np.float32)
    # ---- the level build
    say("level build: HIP events, averages over %d builds per call, medians over %d calls" % (a.reps, a.rounds))
    for n_voxels in (int(v) for v in a.voxels.split(",")):
        capacity = 1
        while capacity < 2 * n_voxels:
            capacity <<= 1
        cloud = surface_cloud(n_voxels, a.leaf)
        with VoxelMap(reg, a.leaf, capacity) as m:
            m.set_box(None, None)
            m.insert_cloud(cloud, None, eye)
            assert not m.full
            us, counters = [], np.zeros(24, np.int64)
            for rnd in range(a.rounds + 1):          # (the first round is the warm-up)
                avg = np.zeros(8, np.float32)
                rc = L.rgbd360_map_time_coarsen(m._handle(), 3, a.reps, _ptr(avg), _ptr(counters))
                assert rc == 0, (rc, L.rgbd360_map_last_error(m._h))
                if rnd:
                    us.append(avg)
            us = np.stack(us)
            med, lo, hi = np.median(us, axis=0), us.min(axis=0), us.max(axis=0)
            c = counters.reshape(6, 4)
            say("%d voxels in %d slots (table %d MiB, levels %.1f MiB): one k_vmap_extract launch over the table %.1f us (min %.1f, max %.1f)"
                % (len(m), capacity, m.bytes >> 20, m.pyramid_bytes / 2.0 ** 20, med[7], lo[7], hi[7]))
            for s in (1, 2, 3):
                say("    level %d: %.1f us (min %.1f, max %.1f) = %.2f scans | %d live slots read, %d voxels created in %d slots, %d points, %d dropped"
                    % (s, med[s - 1], lo[s - 1], hi[s - 1], med[s - 1] / med[7], c[s - 1][0], c[s - 1][1], m.level(s).bytes // 64, c[s - 1][2], c[s - 1][3]))
            say("    levels 1 - 3 back to back: %.1f us (min %.1f, max %.1f) = %.2f scans" % (med[6], lo[6], hi[6], med[6] / med[7]))
    # ---- the alignment
    import map_align_reference as A
    W, H = (int(x) for x in a.frame.split("x"))
    P = synth.trajectory_pose(0, 7).astype(np.float32)
    rgb, depth = synth.render(synth.trajectory_pose(0, 7), W, H, 7)
    guess = A.perturbed(P, 0.15, 0.03, 40)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    d = np.ascontiguousarray(depth)
    d_dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_dev), d.nbytes) == 0 and hip.hipMemcpy(d_dev, _ptr(d), d.nbytes, 1) == 0
    dtype = 0 if d.dtype == np.uint16 else 1
    maps = {s: VoxelMap(reg, float(np.float32(a.leaf) * np.float32(2 ** s)), 1 << 20) for s in (0, 1, 2, 3)}
    try:
        for m in maps.values():
            m.insert_sphere(None, depth, P, convention=2)
            assert not m.full
        m0 = maps[0]
        say("alignment: a %dx%d frame (%d points) against a map of %d voxels (table %d MiB) that holds it, from 0.15 m / 0.03 rad off; host wall clock "
            "per call, medians over %d calls" % (W, H, d.size, len(m0), m0.bytes >> 20, a.reps * a.rounds))
        out, res, res1 = np.zeros(16, np.float32), _lib.MapC2fResult(), _lib.MapAlignResult()

        def c2f(where):
            g = pose_to_cm(guess)
            rc = L.rgbd360_map_align_c2f_sphere(m0._handle(), d_dev if where else _ptr(d), d.strides[0], dtype, H, W, 2, _ptr(g), where, None, _ptr(out), C.byref(res))
            assert rc >= 0, (rc, L.rgbd360_map_last_error(m0._h))
            return out.copy()

        def by_hand(where):
            pose = pose_to_cm(guess)
            for s in (3, 2, 1, 0):
                rc = L.rgbd360_map_align_sphere(maps[s]._handle(), d_dev if where else _ptr(d), d.strides[0], dtype, H, W, 2, _ptr(pose), where, None, _ptr(out),
                                                C.byref(res1))
                assert rc >= 0, (rc, L.rgbd360_map_last_error(maps[s]._h))
                if rc == 0 or s == 0:
                    pose = out.copy()
            return pose

        def wall(call, *args):
            t0 = time.perf_counter()
            r = call(*args)
            return 1e6 * (time.perf_counter() - t0), r

        for where, name in ((0, "host"), (1, "device")):
            for _ in range(2):                  # warm-up: the levels built, code loaded, buffers grown
                pa, pb = c2f(where), by_hand(where)
            assert pa.tobytes() == pb.tobytes(), "the chain by hand over four maps gives the chain's bits"
            ta = np.array([wall(c2f, where)[0] for _ in range(a.reps * a.rounds)])
            tb = np.array([wall(by_hand, where)[0] for _ in range(a.reps * a.rounds)])
            say("    %s memory: rgbd360_map_align_c2f_sphere (top_shift 3) %.1f us (min %.1f, max %.1f) | four rgbd360_map_align_sphere calls on four maps "
                "%.1f us (min %.1f, max %.1f) | c2f / by hand %.3f x" % (name, np.median(ta), ta.min(), ta.max(), np.median(tb), tb.min(), tb.max(),
                                                                       np.median(ta) / np.median(tb)))
        from rgbd360_amd.register import pose_from_cm
        say("    per level (shift: iterations, matched): %s; the pose ends %.2e rad, %.2e m from the truth"
            % (", ".join("%d: %d, %d" % (res.levels[k].shift, res.levels[k].iterations, res.levels[k].n_matched) for k in range(res.n_levels)),
               *A.pose_error(pose_from_cm(out), P)))
        cold = []
        for _ in range(a.rounds):               # the first call after the map was written rebuilds levels 1 - 3
            m0.move_sphere(None, depth, P, P, convention=2)
            cold.append(wall(c2f, 1)[0])
        cold = np.array(cold)
        say("    the first call after the map was written (levels 1 - 3 rebuilt, three synchronisations more), device memory: %.1f us (min %.1f, max %.1f); "
            "levels %.1f MiB beside the table" % (np.median(cold), cold.min(), cold.max(), m0.pyramid_bytes / 2.0 ** 20))
    finally:
        for m in maps.values():
            m.close()
        hip.hipFree(d_dev)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
