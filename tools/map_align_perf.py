"""The kernels of the alignment against the voxel map on the device: what one evaluation, one solve and a whole alignment cost next
to one insert of the same frame and to a copy of its bytes.

    python tools/map_align_perf.py [--sizes 2048x1024,1920x320] [--reps 20] [--leaf 0.05] [--out profiles/map_align_perf.txt]
    python tools/map_align_perf.py --gicp [--rounds 3] --out profiles/map_align_gicp_perf.txt

Per size (the synthetic room, uint16 depth in device memory, convention 2, the map holds the frame at a general pose, the default box;
the alignment starts 1 cm and 3 mrad beside that pose), from HIP events in ONE run (rgbd360_map_time_align): k_vmap_icp_eval,
k_vmap_icp_solve, one k_vmap_insert launch into the populated map, the device-to-device copy of the frame's depth bytes, the table
slots read per point that reached the search, and a whole alignment of 10 iterations (enqueue to synchronisation, wall clock; the
launches behind a converged loop return at once).

--gicp adds the three methods side by side (rgbd360_map_time_align_gicp, and rgbd360_map_time_align_plane for the whole point-to-plane
alignment): the evaluation kernels of generalized ICP, point-to-point and point-to-plane on the same frame, map and buffers in one run,
the solve kernel on the widest row, and a whole alignment of each method, repeated --rounds times so that the spread between rounds
stands next to the differences between the methods.
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


def methods_side_by_side(say, m, d_depth, depth, W, H, beside, a):
    """The evaluation kernels, the solve and a whole alignment of the three methods, `rounds` times; (the map holds the frame twice by now:
    rgbd360_map_time_align inserted it again -- the same voxels, doubled counts)."""
    args = (d_depth, W * depth.itemsize, 0 if depth.dtype == np.uint16 else 1, H, W, 2, _ptr(pose_to_cm(beside)))
    pg, pl, pp = m.align_gicp_params(), m.align_plane_params(), m.align_params()
    _, rg = m.align_sphere_gicp(depth, beside, convention=2)
    _, rl = m.align_sphere_plane(depth, beside, convention=2)
    _, rp = m.align_sphere(depth, beside, convention=2)
    say("    the three methods from the same guess: generalized ICP %d steps (converged %d, %d matches, %d with a target normal), point-to-plane %d steps "
        "(converged %d, %d contributing), point-to-point %d steps (converged %d, %d matches)"
        % (rg["iterations"], rg["converged"], rg["n_matched"], rg["n_target_planes"], rl["iterations"], rl["converged"], rl["n_matched"], rp["iterations"],
           rp["converged"], rp["n_matched"]))
    say("    round | eval: gicp  point  plane | solve (38-word row) | whole alignment: gicp  plane  point | gicp eval / plane eval")
    for r in range(a.rounds):
        ug, ul, up = np.zeros(5, np.float32), np.zeros(4, np.float32), np.zeros(5, np.float32)
        probes = C.c_double(0)
        rc = m._L.rgbd360_map_time_align_gicp(m._handle(), *args, C.byref(pg), a.reps, _ptr(ug), C.byref(probes))
        assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
        rc = m._L.rgbd360_map_time_align_plane(m._handle(), *args, C.byref(pl), a.reps, _ptr(ul), C.byref(probes))
        assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
        # (the point method's whole alignment: rgbd360_map_time_align, which also inserts the frame once more -- the same voxels and centroids)
        rc = m._L.rgbd360_map_time_align(m._handle(), *args, C.byref(pp), a.reps, _ptr(up), C.byref(probes))
        assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
        say("    %5d | %10.1f %6.1f %6.1f | %19.1f | %21.1f %6.1f %6.1f | %.2f" % (r, ug[0], ug[1], ug[2], ug[3], ug[4], ul[3], up[4], ug[0] / ug[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x1024,1920x320")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--out", default="")
    ap.add_argument("--gicp", action="store_true", help="the three methods side by side")
    ap.add_argument("--rounds", type=int, default=3, help="with --gicp: repetitions of the whole comparison")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    say("rgbd360_map_align_*: HIP-event averages over %d launches, leaf %.3f m = max_dist, default box, microseconds" % (a.reps, a.leaf))
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
            pose, res = m.align_sphere(depth, beside, convention=2)
            p = m.align_params()
            us = np.zeros(5, np.float32)
            probes = C.c_double(0)
            rc = m._L.rgbd360_map_time_align(m._handle(), d_depth, W * depth.itemsize, 0 if depth.dtype == np.uint16 else 1, H, W, 2, _ptr(pose_to_cm(beside)),
                                             C.byref(p), a.reps, _ptr(us), C.byref(probes))
            assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
            say("%dx%d: %d pixels, %d reach the search, %d voxels in a table of %d MiB; the alignment: status %d, %d steps, converged %d, %d matches"
                % (W, H, W * H, st["n_added"], st["n_voxels"], m.bytes >> 20, res["status"], res["iterations"], res["converged"], res["n_matched"]))
            say("    k_vmap_icp_eval %.1f | k_vmap_icp_solve %.1f | one k_vmap_insert launch into the populated map %.1f | device copy of the depth bytes %.1f "
                "(%d B/px)" % (us[0], us[1], us[2], us[3], depth.itemsize))
            say("    table slots read per searched point %.2f (27 first probes + what the probe sequences add); eval / insert %.2f x; eval / copy %.1f x"
                % (probes.value, us[0] / us[2], us[0] / us[3]))
            say("    a whole alignment of %d iterations, enqueue to synchronisation: %.1f (= %.1f per enqueued iteration)"
                % (p.max_iters, us[4], us[4] / max(p.max_iters, 1)))
            if a.gicp:
                methods_side_by_side(say, m, d_depth, depth, W, H, beside, a)
        hip.hipFree(d_depth)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
