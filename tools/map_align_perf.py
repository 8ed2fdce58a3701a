"""The kernels of the alignment against the voxel map on the device: what one evaluation, one solve and a whole alignment cost next
to one insert of the same frame and to a copy of its bytes.

    python tools/map_align_perf.py [--sizes 2048x1024,1920x320] [--reps 20] [--leaf 0.05] [--out profiles/map_align_perf.txt]
    python tools/map_align_perf.py --gicp [--rounds 3] --out profiles/map_align_gicp_perf.txt
    python tools/map_align_perf.py --colour [--rounds 3] --out profiles/map_align_colour_perf.txt
    python tools/map_align_perf.py --robust [--rounds 5] --out profiles/map_align_robust_perf.txt

Per size (the synthetic room, uint16 depth in device memory, convention 2, the map holds the frame at a general pose, the default box;
the alignment starts 1 cm and 3 mrad beside that pose), from HIP events in ONE run (rgbd360_map_time_align): the point-to-point
evaluation, k_vmap_icp_solve, one k_vmap_insert launch into the populated map, the device-to-device copy of the frame's depth bytes, the table
slots read per point that reached the search, and a whole alignment of 10 iterations (enqueue to synchronisation, wall clock; the
launches behind a converged loop return at once).

--gicp adds the three methods side by side (rgbd360_map_time_align_gicp, and rgbd360_map_time_align_plane for the whole point-to-plane
alignment): the evaluation kernels of generalized ICP, point-to-point and point-to-plane on the same frame, map and buffers in one run,
the solve kernel on the widest row, and a whole alignment of each method, repeated --rounds times so that the spread between rounds
stands next to the differences between the methods.

--colour reports coloured ICP instead (the map holds the frame WITH its colours): the build of the colour layer next to the build of the
normal layer and to a bare scan of the table in the same run (rgbd360_map_time_colours, medians over --reps builds), then per round
the coloured evaluation next to generalized ICP's on the same frame, map and buffers, the solve and a whole coloured alignment
(rgbd360_map_time_align_colour).

--robust reports the robust form of every method next to its quadratic form (rgbd360_map_time_align_robust: the same frame, map, buffers
and parameters in one process, the launches of the two forms alternating): the evaluation kernel, the solve kernel and a whole alignment
of both forms per method and kind, medians over --rounds calls of --reps pairs each, the ratio robust / quadratic, and the spread of the
quadratic evaluation between the rounds, which is what a ratio has to exceed to mean anything.  The quadratic kernels are the machine
code they were before there was a robust form (tools/device_asm_diff.py), so the quadratic column is the baseline.

The evaluation of every method is one kernel template, k_vmap_eval<M, SRC> (csrc/map_align.h).  The report lines keep the labels
k_vmap_icp_eval, k_vmap_plane_eval, k_vmap_gicp_eval and k_vmap_colour_eval for its four instantiations: they are labels, not kernel
names, kept so that old and new profiles compare line by line.
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


def colour_report(say, hip, reg, P, beside, a):
    """--colour: per size the layer build (against the normal layer's build and a bare table scan) and the evaluation (against
    k_vmap_gicp_eval), all figures from the same run."""
    from rgbd360_amd import _lib
    say("rgbd360_map_colours / rgbd360_map_align_colour_*: HIP events, leaf %.3f m = max_dist, default box, microseconds" % a.leaf)
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        rgb, depth = synth.render(synth.trajectory_pose(0, 7), W, H, 7)[:2]
        rgb, depth = np.ascontiguousarray(rgb), np.ascontiguousarray(depth)
        d_depth, d_rgb = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_depth), depth.nbytes) == 0 and hip.hipMemcpy(d_depth, _ptr(depth), depth.nbytes, 1) == 0
        assert hip.hipMalloc(C.byref(d_rgb), rgb.nbytes) == 0 and hip.hipMemcpy(d_rgb, _ptr(rgb), rgb.nbytes, 1) == 0
        with VoxelMap(reg, a.leaf, 1 << 21) as m:
            st = m.insert_sphere(rgb, depth, P, convention=2)
            cp = m.colour_params()
            build, normals, scan = (np.zeros(a.reps, np.float32) for _ in range(3))
            cs, layer_bytes = _lib.MapColourStats(), C.c_longlong(0)
            rc = m._L.rgbd360_map_time_colours(m._handle(), C.byref(cp), a.reps, _ptr(build), _ptr(normals), _ptr(scan), C.byref(cs), C.byref(layer_bytes))
            assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
            say("%dx%d: %d pixels, %d reach the search, %d voxels in a table of %d MiB, the colour layer %d MiB: %d gradients, %d voxels without a normal, "
                "%d without a gradient" % (W, H, W * H, st["n_added"], st["n_voxels"], m.bytes >> 20, layer_bytes.value >> 20, cs.n_gradients, cs.n_no_normal,
                                           cs.n_no_gradient))
            say("    layer builds, medians of %d: k_vmap_colour_layer %.1f | k_vmap_normals %.1f | bare table scan (k_vmap_extract, centroids) %.1f | "
                "colour / normals %.2f | colour / scan %.2f" % (a.reps, np.median(build), np.median(normals), np.median(scan),
                                                                np.median(build) / np.median(normals), np.median(build) / np.median(scan)))
            pose, res = m.align_sphere_colour(rgb, depth, beside, convention=2)
            _, rg = m.align_sphere_gicp(depth, beside, convention=2)
            say("    coloured ICP from the guess: status %d, %d steps (converged %d), %d contributing, %d dropped without a normal, %d with a zero gradient, "
                "rms %.5f m / %.5f; generalized ICP: %d steps, %d matches" % (res["status"], res["iterations"], res["converged"], res["n_matched"],
                                                                              res["n_no_normal"], res["n_no_gradient"], res["rms_geometric"], res["rms_colour"],
                                                                              rg["iterations"], rg["n_matched"]))
            pc = m.align_colour_params()
            args = (d_rgb, W * 3, d_depth, W * depth.itemsize, 0 if depth.dtype == np.uint16 else 1, H, W, 2, _ptr(pose_to_cm(beside)))
            say("    round | eval: colour  gicp | solve (38-word row) | whole coloured alignment | colour eval / gicp eval | slots read per searched point")
            for r in range(a.rounds):
                us, probes = np.zeros(4, np.float32), C.c_double(0)
                rc = m._L.rgbd360_map_time_align_colour(m._handle(), *args, C.byref(pc), a.reps, _ptr(us), C.byref(probes))
                assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
                say("    %5d | %12.1f %5.1f | %19.1f | %24.1f | %23.2f | %.2f" % (r, us[0], us[1], us[2], us[3], us[0] / us[1], probes.value))
        hip.hipFree(d_depth)
        hip.hipFree(d_rgb)


ROBUST_DELTA = {"point": 0.03, "plane": 0.01, "gicp": 0.3, "colour": 0.01}      # near the median square root of each method's cost term at the guess


def robust_report(say, hip, reg, P, beside, a):
    """--robust: per size, method and kind the robust form next to the quadratic one, all figures from alternating launches of one process."""
    say("rgbd360_map_set_align_robust: robust / quadratic form of every method, HIP events, alternating launches, medians of %d rounds of %d pairs, "
        "leaf %.3f m = max_dist, default box, microseconds" % (a.rounds, a.reps, a.leaf))
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        rgb, depth = (np.ascontiguousarray(x) for x in synth.render(synth.trajectory_pose(0, 7), W, H, 7)[:2])
        d_depth, d_rgb = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_depth), depth.nbytes) == 0 and hip.hipMemcpy(d_depth, _ptr(depth), depth.nbytes, 1) == 0
        assert hip.hipMalloc(C.byref(d_rgb), rgb.nbytes) == 0 and hip.hipMemcpy(d_rgb, _ptr(rgb), rgb.nbytes, 1) == 0
        with VoxelMap(reg, a.leaf, 1 << 21) as m:
            st = m.insert_sphere(rgb, depth, P, convention=2)
            say("%dx%d: %d pixels, %d reach the search, %d voxels in a table of %d MiB" % (W, H, W * H, st["n_added"], st["n_voxels"], m.bytes >> 20))
            say("    method kind          delta | eval: robust  quadratic  ratio (spread of quadratic) | solve: robust  quadratic | whole alignment: robust  quadratic  ratio"
                " | contributing  down-weighted  sum w")
            for code, method in enumerate(("point", "plane", "gicp", "colour")):
                p = getattr(m, {"point": "align_params", "plane": "align_plane_params", "gicp": "align_gicp_params", "colour": "align_colour_params"}[method])()
                head = (d_rgb, W * 3) if method == "colour" else (None, 0)
                args = head + (d_depth, W * depth.itemsize, 0 if depth.dtype == np.uint16 else 1, H, W, 2, _ptr(pose_to_cm(beside)))
                for kind in ("huber", "cauchy", "geman_mcclure"):
                    m.set_align_robust(method, kind, ROBUST_DELTA[method])
                    us = np.zeros((a.rounds, 6), np.float32)
                    for r in range(a.rounds):
                        rc = m._L.rgbd360_map_time_align_robust(m._handle(), code, *args, C.byref(p), a.reps, _ptr(us[r]))
                        assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
                    run = {"point": m.align_sphere, "plane": m.align_sphere_plane, "gicp": m.align_sphere_gicp}.get(method)
                    _ = run(depth, beside, convention=2) if run else m.align_sphere_colour(rgb, depth, beside, convention=2)
                    info = m.robust_info()      # (of that alignment's final evaluation)
                    m.set_align_robust(method, "none")
                    med = np.median(us, axis=0)
                    spread = (us[:, 1].max() - us[:, 1].min()) / med[1]
                    say("    %-6s %-13s %5.2f | %12.1f %10.1f %6.3f (%.3f) | %13.1f %10.1f | %24.1f %10.1f %6.3f | %12d %14d %6.0f"
                        % (method, kind, ROBUST_DELTA[method], med[0], med[1], med[0] / med[1], spread, med[2], med[3], med[4], med[5], med[4] / med[5],
                           info["n"], info["n_downweighted"], info["sum_w"]))
        hip.hipFree(d_depth)
        hip.hipFree(d_rgb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x1024,1920x320")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--out", default="")
    ap.add_argument("--gicp", action="store_true", help="the three methods side by side")
    ap.add_argument("--colour", action="store_true", help="coloured ICP: the layer build and the evaluation next to generalized ICP's")
    ap.add_argument("--robust", action="store_true", help="the robust form of every method next to its quadratic form")
    ap.add_argument("--rounds", type=int, default=3, help="with --gicp / --colour / --robust: repetitions of the whole comparison")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    reg = RegisterPhotoICP()
    P = general_pose()
    beside = P.copy()
    beside[:3, 3] += np.array([0.006, -0.006, 0.005], np.float32)
    c, s = np.cos(0.003), np.sin(0.003)
    beside = (np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]) @ beside.astype(np.float64)).astype(np.float32)
    if a.robust:
        robust_report(say, hip, reg, P, beside, a)
    elif a.colour:
        colour_report(say, hip, reg, P, beside, a)
    else:
        say("rgbd360_map_align_*: HIP-event averages over %d launches, leaf %.3f m = max_dist, default box, microseconds" % (a.reps, a.leaf))
    for size in ([] if a.colour or a.robust else a.sizes.split(",")):
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
