"""The rig calibration against the voxel map (rgbd360_map_calibrate_rig_clouds, csrc/rig_calib.h) next to
rgbd360_map_align_plane_batch_cloud on the same inputs with the same max_iters -- the same evaluation with independent solves -- and the
new solve launches under HIP events.

    python tools/rig_calib_perf.py [--reps 9] [--leaf 0.05] [--iters 10] [--out profiles/rig_calib_perf.txt]

The map holds the 2048 x 1024 frame of the synthetic room at a general pose.  Inputs: K S = 64 (K = 8, S = 8) and 1024 (K = 64, S = 16)
clouds of 4 096 and 76 800 points (a 320 x 240 sensor image) in device memory -- one cloud of the frame's valid points shared by all
inputs, the rig poses and the extrinsics a few millimetres and milliradians beside (map pose, identity) in seeded directions, eps 0 so
that every call takes `iters` steps.  Per shape, after a warm-up: `reps` times the calibration (extrinsics only, then joint with sensor 0
fixed) and the batch call, alternating; medians of the wall times in microseconds and "calibration / batch".  Then the solve launches of
one step on synthetic rows of the same K and S (rgbd360_rig_calib_time_solve: chains of launches between two events, a kernel's time is
the difference of two chains).
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
from map_align_reference import perturbed                            # noqa: E402
from voxel_map_reference import general_pose                         # noqa: E402


def hip_runtime():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def synthetic_rows(n_inputs, seed=1):
    """Well-posed rows of 30 sums: 1000 points whose J are seeded random vectors."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n_inputs, 30))
    for i in range(n_inputs):
        J = rng.normal(size=(1000, 6))
        H, r = J.T @ J, rng.normal(size=1000) * 1e-3
        rows[i, 0] = 1000
        rows[i, 1:22] = [H[a, b] for a in range(6) for b in range(a, 6)]
        rows[i, 22:28] = J.T @ r
        rows[i, 28] = r @ r
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hip, reg = hip_runtime(), RegisterPhotoICP(device=0)
    W, H = 2048, 1024
    depth = np.ascontiguousarray(synth.render(synth.trajectory_pose(0, 7), W, H, 7)[1])
    P = general_pose()
    c = reg.sphere_cloud(depth, 2).reshape(-1, 3)
    valid = c[np.isfinite(c).all(axis=1) & (np.abs(c).sum(axis=1) > 0)]
    eye = np.eye(4, dtype=np.float32)
    with VoxelMap(reg, a.leaf, 1 << 21) as m:
        L, Hm = m._L, m._handle()
        m.insert_sphere(None, depth, P, convention=2)
        say("rgbd360_map_calibrate_rig_clouds against rgbd360_map_align_plane_batch_cloud on the same K S inputs: wall time of the calls in microseconds,")
        say("medians of %d alternating repetitions, inputs in device memory, leaf %.3f m = max_dist, max_iters %d, eps 0, map of %d voxels" % (a.reps, a.leaf, a.iters, len(m)))
        say("K x S      points | steps | extrinsics only |   joint (s0 fixed) |   batch of K S jobs | extrinsics / batch | joint / batch")
        for K, S in ((8, 8), (64, 16)):
            T = np.stack([perturbed(P, 0.004, 0.002, 100 + k) for k in range(K)])
            E = np.stack([perturbed(eye, 0.004, 0.002, 200 + s) for s in range(S)])
            for n in (4096, 76800):
                x = np.ascontiguousarray(valid[np.linspace(0, len(valid) - 1, n).astype(np.int64)])
                d_x = C.c_void_p()
                assert hip.hipMalloc(C.byref(d_x), x.nbytes) == 0 and hip.hipMemcpy(d_x, _ptr(x), x.nbytes, 1) == 0
                I = (_lib.MapBatchCloud * (K * S))()
                J = (_lib.MapBatchJob * (K * S))()
                for i in range(K * S):
                    I[i].xyz, I[i].n = d_x.value, n
                    J[i].input = i
                    J[i].guess[:] = pose_to_cm((T[i // S].astype(np.float64) @ E[i % S].astype(np.float64)).astype(np.float32)).tolist()
                pp = m.align_plane_params(max_iters=a.iters, eps=0.0)
                poses = np.zeros((K * S, 16), np.float32)
                bres = (_lib.MapAlignPlaneResult * (K * S))()
                res = _lib.RigCalibResult()

                def calibrate(joint):
                    p = m.rig_calib_params(max_iters=a.iters, eps=0.0, refine_poses=joint, fixed_sensor=0 if joint else -1)
                    Tc = np.stack([pose_to_cm(q) for q in T]).astype(np.float32)
                    Ec = np.stack([pose_to_cm(q) for q in E]).astype(np.float32)
                    t0 = time.perf_counter()
                    rc = L.rgbd360_map_calibrate_rig_clouds(Hm, I, K, S, 1, _ptr(Tc), _ptr(Ec), C.byref(p), C.byref(res), None)
                    t1 = time.perf_counter()
                    assert rc >= 0, (rc, L.rgbd360_map_last_error(Hm))
                    return (t1 - t0) * 1e6

                def batch():
                    t0 = time.perf_counter()
                    rc = L.rgbd360_map_align_plane_batch_cloud(Hm, I, K * S, 1, J, K * S, C.byref(pp), _ptr(poses), bres)
                    t1 = time.perf_counter()
                    assert rc == 0, (rc, L.rgbd360_map_last_error(Hm))
                    return (t1 - t0) * 1e6

                calibrate(0), calibrate(1), batch()          # warm-up
                steps = []
                t = {0: [], 1: [], "b": []}
                for _ in range(a.reps):
                    for joint in (0, 1):
                        t[joint].append(calibrate(joint))
                        steps.append((res.status, res.iterations))
                    t["b"].append(batch())
                e, j, b = (float(np.median(t[k])) for k in (0, 1, "b"))
                say("%3d x %-3d %8d | %-5s | %15.1f | %18.1f | %19.1f | %18.2f | %13.2f"
                    % (K, S, n, "/".join(sorted({"%d:%d" % s for s in steps})), e, j, b, e / b, j / b))
                hip.hipFree(d_x)
        say()
        say("the solve launches of one step (HIP events, averages of 50 chains, microseconds; a kernel = the difference of two chains):")
        say("K x S      mode       | k_rig_init | k_rig_input | k_rig_frames | k_rig_solve")
        for K, S in ((8, 8), (64, 16)):
            rows = synthetic_rows(K * S)
            Tc = np.stack([pose_to_cm(perturbed(P, 0.004, 0.002, 100 + k)) for k in range(K)]).astype(np.float32)
            Ec = np.stack([pose_to_cm(perturbed(eye, 0.004, 0.002, 200 + s)) for s in range(S)]).astype(np.float32)
            for joint in (0, 1):
                p = m.rig_calib_params(refine_poses=joint, fixed_sensor=0 if joint else -1)
                us = np.zeros(4, np.float32)
                rc = L.rgbd360_rig_calib_time_solve(Hm, _ptr(rows), K, S, _ptr(Tc), _ptr(Ec), C.byref(p), 50, _ptr(us))
                assert rc == 0, (rc, L.rgbd360_map_last_error(Hm))
                say("%3d x %-3d %-10s | %10.1f | %11.1f | %12.1f | %11.1f" % (K, S, "joint" if joint else "extrinsics", us[0], us[1] - us[0], us[2] - us[1], us[3] - us[2]))
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
