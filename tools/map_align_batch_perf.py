"""Many alignments against the voxel map in lock step (rgbd360_map_align_batch_*, csrc/map_align_batch.h) next to the same alignments
as single calls issued back to back: wall time of the calls, inputs in device memory.

    python tools/map_align_batch_perf.py [--reps 15] [--leaf 0.05] [--out profiles/map_align_batch_perf.txt]
    python tools/map_align_batch_perf.py --trace-shape cloud:16384:16:plane      one batch call and nothing else timed: the program of a
                                                                                 `rocprofv3 --kernel-trace --stats -- python tools/...` run

The map holds the 2048 x 1024 frame of the synthetic room at a general pose (default box).  Shapes: clouds of 4 096, 16 384 and 65 536
points spread evenly over the frame's valid points, and the frame itself; both methods; n_jobs 1, 4, 16, 64 (the frame: 1, 4, 16).  The
jobs of a batch share one input and start from guesses 1 cm and 3 mrad beside the map pose in different seeded directions, so they stop
after different numbers of steps, as a lattice of guesses does.  Per shape and n_jobs, after a warm-up of both sides: `reps` times one
batch call, then the n_jobs single calls from the same guesses, alternating inside this one process; the medians of both, and
"singles / batch", the ratio of the two medians (wall time of n_jobs single calls over wall time of one batch call: above 1 the batch
is faster).  The poses of both sides are compared on the spot: they are the same bytes.
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


def to_device(hip, a):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, _ptr(a), a.nbytes, 1) == 0
    return p


class Shape:
    """One input in device memory and the calls on it: batch(n_jobs) and singles(n_jobs), both returning the poses' bytes."""

    def __init__(self, m, method, guesses, cloud=None, frame=None):
        self.m, self.L, self.H, self.plane = m, m._L, m._handle(), method == "plane"
        self.p = (m.align_plane_params if self.plane else m.align_params)()
        self.rt = _lib.MapAlignPlaneResult if self.plane else _lib.MapAlignResult
        self.guesses = [pose_to_cm(g) for g in guesses]
        self.cloud, self.frame = cloud, frame
        prefix = "rgbd360_map_align_plane_" if self.plane else "rgbd360_map_align_"
        self.e_single = getattr(self.L, prefix + ("cloud" if cloud else "sphere"))
        self.e_batch = getattr(self.L, prefix + ("batch_cloud" if cloud else "batch_sphere"))
        self.jobs = (_lib.MapBatchJob * len(guesses))()
        for k, g in enumerate(self.guesses):
            self.jobs[k].input = 0
            self.jobs[k].guess[:] = g.tolist()
        if cloud:
            self.inputs = (_lib.MapBatchCloud * 1)()
            self.inputs[0].xyz, self.inputs[0].n = cloud[0].value, cloud[1]
        else:
            self.inputs = (_lib.MapBatchFrame * 1)()
            self.inputs[0].depth, self.inputs[0].depth_step = frame[0].value, frame[1]
        self.poses = np.zeros((len(guesses), 16), np.float32)
        self.res = (self.rt * len(guesses))()

    def batch(self, n):
        geometry = () if self.cloud else self.frame[2:]
        rc = self.e_batch(self.H, self.inputs, 1, *geometry, 1, self.jobs, n, C.byref(self.p), _ptr(self.poses), self.res)
        assert rc == 0, (rc, self.L.rgbd360_map_last_error(self.H))
        return self.poses[:n].tobytes()

    def singles(self, n):
        out = np.zeros((n, 16), np.float32)
        for k in range(n):
            if self.cloud:
                rc = self.e_single(self.H, self.cloud[0], self.cloud[1], _ptr(self.guesses[k]), 1, C.byref(self.p), _ptr(out[k]), C.byref(self.res[k]))
            else:
                rc = self.e_single(self.H, self.frame[0], self.frame[1], *self.frame[2:], _ptr(self.guesses[k]), 1, C.byref(self.p), _ptr(out[k]),
                                   C.byref(self.res[k]))
            assert rc >= 0, (rc, self.L.rgbd360_map_last_error(self.H))
        return out.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-shape", default=None, help="cloud:N:JOBS:METHOD or frame:JOBS:METHOD -- one warm-up and one batch call")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hip, reg = hip_runtime(), RegisterPhotoICP(device=0)
    W, H = 2048, 1024
    depth = np.ascontiguousarray(synth.render(synth.trajectory_pose(0, 7), W, H, 7)[1])
    P = general_pose()
    guesses = [perturbed(P, 0.01, 0.003, seed) for seed in range(1, 65)]
    c = reg.sphere_cloud(depth, 2).reshape(-1, 3)
    valid = c[np.isfinite(c).all(axis=1) & (np.abs(c).sum(axis=1) > 0)]
    d_depth = to_device(hip, depth)
    frame = (d_depth, W * depth.itemsize, 0 if depth.dtype == np.uint16 else 1, H, W, 2)
    with VoxelMap(reg, a.leaf, 1 << 21) as m:
        m.insert_sphere(None, depth, P, convention=2)
        shapes = [("cloud", n, (1, 4, 16, 64)) for n in (4096, 16384, 65536)] + [("frame", W * H, (1, 4, 16))]
        if a.trace_shape:
            f = a.trace_shape.split(":")
            shapes = [("cloud", int(f[1]), (int(f[2]),))] if f[0] == "cloud" else [("frame", W * H, (int(f[1]),))]
            methods = (f[-1],)
        else:
            methods = ("point", "plane")
            say("rgbd360_map_align_batch_* against n_jobs single calls: wall time of the calls in microseconds, medians of %d alternating repetitions," % a.reps)
            say("inputs in device memory, leaf %.3f m = max_dist, default parameters (10 iterations at most), map of %d voxels" % (a.leaf, len(m)))
            say("shape                 method  n_jobs | steps min..max |   one batch call | n_jobs single calls | singles / batch")
        for kind, n, job_counts in shapes:
            x = d_x = None
            if kind == "cloud":
                x = np.ascontiguousarray(valid[np.linspace(0, len(valid) - 1, n).astype(np.int64)])
                d_x = to_device(hip, x)
            for method in methods:
                s = Shape(m, method, guesses, cloud=(d_x, n) if kind == "cloud" else None, frame=None if kind == "cloud" else frame)
                for n_jobs in job_counts:
                    assert s.batch(n_jobs) == s.singles(n_jobs)          # warm-up of both sides, and the same bytes
                    if a.trace_shape:
                        s.batch(n_jobs)
                        continue
                    steps = [s.res[k].iterations for k in range(n_jobs)]
                    tb, ts = [], []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        s.batch(n_jobs)
                        t1 = time.perf_counter()
                        s.singles(n_jobs)
                        t2 = time.perf_counter()
                        tb.append((t1 - t0) * 1e6)
                        ts.append((t2 - t1) * 1e6)
                    b, sg = float(np.median(tb)), float(np.median(ts))
                    say("%-21s %-6s %7d | %6d..%-6d | %16.1f | %19.1f | %15.2f"
                        % ("cloud of %d" % n if kind == "cloud" else "frame %dx%d" % (W, H), method, n_jobs, min(steps), max(steps), b, sg, sg / b))
            if d_x is not None:
                hip.hipFree(d_x)
    hip.hipFree(d_depth)
    reg.close()
    if a.out and not a.trace_shape:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
