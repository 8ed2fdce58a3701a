"""The voxel map's kernels on the device: what inserting a frame and reading the map out cost next to forming the cloud.

    python tools/voxel_map_perf.py [--sizes 2048x1024,1920x320] [--reps 20] [--leaf 0.05] [--out profiles/voxel_map_perf.txt]

Per size (the synthetic room, uint16 depth + colour in device memory, convention 2, a general pose, the default box), from HIP events
(rgbd360_map_time_kernels): k_vmap_insert into an EMPTY map, k_vmap_insert into a map that already holds the frame's voxels (the
steady state of odometry), k_vmap_extract -- each next to ONE k_sphere_cloud_s4 launch of the same size in the same run and to the
input-bytes floor: 2 or 4 B/px of depth + 3 B/px of colour, READ once at the rate of a device-to-device copy of those bytes measured in
the same run (the copy reads and writes every byte, so the floor is half the copy's time).  And the global slot updates
the insert issues per pixel after on-chip combining, with the atomic bytes they stand for against the chip-wide atomic rate of the
micro-architecture notes (about 1.3 TB/s of added bytes for contiguous 256-byte wave-instructions, one seventeenth of it for one lane
per row).
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

ATOMIC_RATE = 1.3e12          # B/s of added bytes, contiguous wave-instructions (micro-architecture notes, "Global float atomics")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x1024,1920x320")
    ap.add_argument("--reps", type=int, default=20)
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

    say("rgbd360_map_*: HIP-event averages over %d rounds, leaf %.3f m, default box, microseconds" % (a.reps, a.leaf))
    reg = RegisterPhotoICP()
    pose = pose_to_cm(general_pose())
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        rgb, depth = synth.render(synth.trajectory_pose(0, 7), W, H, 7)
        rgb, depth = np.ascontiguousarray(rgb), np.ascontiguousarray(depth)
        n = W * H
        d_rgb, d_depth = to_device(rgb), to_device(depth)
        with VoxelMap(reg, a.leaf, 1 << 21) as m:
            st = m.insert_sphere(rgb, depth, general_pose(), convention=2)
            us = np.zeros(5, np.float32)
            upd = C.c_longlong(0)
            rc = m._L.rgbd360_map_time_kernels(m._handle(), d_rgb, W * 3, d_depth, W * depth.itemsize, 0 if depth.dtype == np.uint16 else 1,
                                               H, W, 2, _ptr(pose), a.reps, _ptr(us), C.byref(upd))
            assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
            in_bytes = n * (depth.itemsize + 3)
            copy_rate = 2 * in_bytes / (us[4] * 1e-6)             # bytes moved per second by the copy: each is read and written
            floor_us = 0.5 * float(us[4])                         # the frame's bytes READ once at that rate
            say("%dx%d: %d pixels, %d pass the box, %d voxels (%.1f points per voxel), table %d MiB"
                % (W, H, n, st["n_added"], st["n_voxels"], st["n_added"] / max(st["n_voxels"], 1), m.bytes >> 20))
            say("    k_vmap_insert, empty map %.1f | map holds the frame %.1f | k_vmap_extract %.1f | one k_sphere_cloud_s4 launch %.1f | "
                "input-bytes floor %.1f (%d B/px read once; the device copy of them took %.1f: %.0f GB/s read + written)"
                % (us[0], us[1], us[2], us[3], floor_us, depth.itemsize + 3, us[4], copy_rate / 1e9))
            say("    insert / cloud kernel: %.2f x (empty), %.2f x (steady); insert / floor: %.1f x, %.1f x"
                % (us[0] / us[3], us[1] / us[3], us[0] / floor_us, us[1] / floor_us))
            u = int(upd.value)
            atomic_bytes = u * 56        # seven 8-byte adds per updated slot, one 64-byte slot per eight lanes
            say("    global slot updates after on-chip combining: %d = %.3f per pixel, %.3f per kept point (%.1f points merged per update); "
                "%.1f MB of atomic adds = %.1f us at the contiguous atomic rate, %.1f us at 1/17 of it"
                % (u, u / n, u / max(st["n_added"], 1), st["n_added"] / max(u, 1), atomic_bytes / 1e6, atomic_bytes / ATOMIC_RATE * 1e6,
                   atomic_bytes / ATOMIC_RATE * 17e6))
        hip.hipFree(d_rgb)
        hip.hipFree(d_depth)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
