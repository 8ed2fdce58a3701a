"""The kernels of the point-to-plane alignment against the voxel map on the device, next to the point-to-point evaluation of the same
frame and map.

    python tools/map_align_plane_perf.py [--sizes 2048x1024,1920x320] [--reps 20] [--leaf 0.05] [--out profiles/map_align_plane_perf.txt]

Per size (the synthetic room, uint16 depth in device memory, convention 2, the map holds the frame at a general pose, the default box;
the alignment starts 1 cm and 3 mrad beside that pose), from HIP events in ONE run (rgbd360_map_time_align_plane): the point-to-plane
evaluation, the point-to-point one with the same five shared parameters, the solve on the plane row, the table slots read per point that reached the search, and a
whole point-to-plane alignment of 10 iterations (enqueue to synchronisation, wall clock; the launches behind a converged loop return at
once).  The two eval kernels alternate in `--rounds` rounds within the process, so that a drift of the clock shows as a spread between
rounds and not as a difference between the kernels; the report gives every round.  Its labels k_vmap_plane_eval, k_vmap_icp_eval and
k_vmap_plane_solve stand for k_vmap_eval<PlaneMethod, SRC>, k_vmap_eval<PointMethod, SRC> and k_vmap_icp_solve<PlaneMethod>
(csrc/map_align.h): labels, not kernel names, kept so that old and new profiles compare line by line.
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

    say("rgbd360_map_align_plane_*: HIP-event averages over %d launches, %d rounds, leaf %.3f m = max_dist, default box, microseconds"
        % (a.reps, a.rounds, a.leaf))
    reg = RegisterPhotoICP()
    P = general_pose()
    beside = P.copy()
    beside[:3, 3] += np.array([0.006, -0.006, 0.005], np.float32)
    c, s = np.cos(0.003), np.sin(0.003)
    beside = (np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]) @ beside.astype(np.float64)).astype(np.float32)
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        _, depth = synth.render(synth.trajectory_pose(0, 7), W, H, 7)
        depth = np.ascontiguousarray(depth)
        d_depth = C.c_void_p()
        assert hip.hipMalloc(C.byref(d_depth), depth.nbytes) == 0 and hip.hipMemcpy(d_depth, _ptr(depth), depth.nbytes, 1) == 0
        with VoxelMap(reg, a.leaf, 1 << 21) as m:
            st = m.insert_sphere(None, depth, P, convention=2)
            pose, res = m.align_sphere_plane(depth, beside, convention=2)
            _, point = m.align_sphere(depth, beside, convention=2)
            p = m.align_plane_params()
            say("%dx%d: %d pixels, %d reach the search, %d voxels in a table of %d MiB" % (W, H, W * H, st["n_added"], st["n_voxels"], m.bytes >> 20))
            say("    point-to-plane: status %d, %d steps, converged %d, %d contributing, %d unsupported, %d nonplanar, fitness %.3e (point scale %.3e)"
                % (res["status"], res["iterations"], res["converged"], res["n_matched"], res["n_unsupported"], res["n_nonplanar"], res["fitness"],
                   res["fitness_point"]))
            say("    point-to-point: status %d, %d steps, converged %d, %d matches, fitness %.3e"
                % (point["status"], point["iterations"], point["converged"], point["n_matched"], point["fitness"]))
            rounds = []
            for _ in range(a.rounds):
                us = np.zeros(4, np.float32)
                probes = C.c_double(0)
                rc = m._L.rgbd360_map_time_align_plane(m._handle(), d_depth, W * depth.itemsize, 0 if depth.dtype == np.uint16 else 1, H, W, 2,
                                                       _ptr(pose_to_cm(beside)), C.byref(p), a.reps, _ptr(us), C.byref(probes))
                assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
                rounds.append(us.copy())
                say("    round %d: k_vmap_plane_eval %.1f | k_vmap_icp_eval %.1f | plane / point %.2f x | k_vmap_plane_solve %.1f | whole alignment of %d "
                    "iterations %.1f" % (len(rounds), us[0], us[1], us[0] / us[1], us[2], p.max_iters, us[3]))
            r = np.array(rounds)
            say("    median over the rounds: plane eval %.1f, point eval %.1f, solve %.1f, alignment %.1f (= %.1f per enqueued iteration); table slots read "
                "per searched point %.2f" % (np.median(r[:, 0]), np.median(r[:, 1]), np.median(r[:, 2]), np.median(r[:, 3]),
                                             np.median(r[:, 3]) / max(p.max_iters, 1), probes.value))
        hip.hipFree(d_depth)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
