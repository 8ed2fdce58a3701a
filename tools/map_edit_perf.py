"""The voxel map's editing kernels on the device: what removing a frame, rebuilding the table and the census cost next to an insert
and to a plain scan of the table.

    python tools/map_edit_perf.py [--sizes 2048x1024,1920x320] [--reps 20] [--rounds 3] [--leaf 0.05] [--out profiles/map_edit_perf.txt]

Per size (the synthetic room, uint16 depth + colour in device memory, convention 2, a general pose, the default box), HIP-event averages
over `reps` launches (rgbd360_map_time_edit), `rounds` times in one process.  The map holds the frame twice when the kernels run, so that
the removal empties no voxel and every round sees the same table:
    the removal kernel next to ONE k_vmap_insert launch into the same populated map, in both of the insert's forms: new voxels counted
    by their claims (a map that never had a voxel emptied), and by the count add that returned 0 (a map that may hold tombstones);
    k_vmap_rehash (with the clear of the new table) and the census scan next to ONE k_vmap_extract scan over the same table;
    a whole move call out of device memory: the removal launch, the insert launch and the one wait.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rgbd360_amd import synth                                        # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP, pose_to_cm, _ptr  # noqa: E402
from rgbd360_amd.voxel_map import VoxelMap                           # noqa: E402
from voxel_map_reference import general_pose                         # noqa: E402  (30 degrees about a skew axis, t = (0.7, -1.3, 0.4))

NAMES = ("k_vmap_insert, claims counted", "removal kernel", "k_vmap_insert, revivals counted", "clear + k_vmap_rehash", "k_vmap_census",
         "k_vmap_extract scan", "whole move call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x1024,1920x320")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def to_device(arr):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), arr.nbytes) == 0 and hip.hipMemcpy(p, _ptr(arr), arr.nbytes, 1) == 0
        return p

    say("rgbd360_map_* editing: HIP-event averages over %d launches, %d rounds in one process, leaf %.3f m, default box, microseconds" % (a.reps, a.rounds, a.leaf))
    reg = RegisterPhotoICP()
    pose = pose_to_cm(general_pose())
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        rgb, depth = synth.render(synth.trajectory_pose(0, 7), W, H, 7)
        rgb, depth = np.ascontiguousarray(rgb), np.ascontiguousarray(depth)
        d_rgb, d_depth = to_device(rgb), to_device(depth)
        with VoxelMap(reg, a.leaf, 1 << 21) as m:
            st = m.insert_sphere(rgb, depth, general_pose(), convention=2)
            say("%dx%d: %d pixels, %d pass the box, %d voxels, table %d MiB (%d slots)" % (W, H, W * H, st["n_added"], st["n_voxels"], m.bytes >> 20, m.bytes // 64))
            rounds = []
            for r in range(a.rounds):
                us = np.zeros(7, np.float32)
                rc = m._L.rgbd360_map_time_edit(m._handle(), d_rgb, W * 3, d_depth, W * depth.itemsize, 0 if depth.dtype == np.uint16 else 1, H, W, 2,
                                                _ptr(pose), a.reps, _ptr(us))
                assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
                rounds.append(us.astype(np.float64))
                say("    round %d: " % r + " | ".join("%s %.1f" % (n, v) for n, v in zip(NAMES, us)))
            t = np.array(rounds)
            mean, spread = t.mean(axis=0), (t.max(axis=0) - t.min(axis=0)) / t.mean(axis=0)
            say("    mean (spread of the rounds): " + " | ".join("%s %.1f (%.1f %%)" % (n, v, 100 * s) for n, v, s in zip(NAMES, mean, spread)))
            say("    removal / insert %.2f x; revival-counting insert / claim-counting insert %.3f x; rehash / extract scan %.2f x; census / extract scan %.2f x"
                % (mean[1] / mean[0], mean[2] / mean[0], mean[3] / mean[5], mean[4] / mean[5]))
            c = m.census()
            assert c["n_inconsistent"] == 0 and c["n_tombstones"] == 0 and c["n_live"] == st["n_voxels"], c
        hip.hipFree(d_rgb)
        hip.hipFree(d_depth)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
