"""Composing voxel maps on the device: what a merge launch costs next to one scan of the source table, what re-posing a submap costs next
to moving the frames that built it, and how many destination voxels a source voxel shares.

    python tools/map_merge_perf.py [--frames 8] [--frame 2048x1024] [--reps 15] [--rounds 5] [--leaf 0.05] [--moves 20] [--sub-slots 524288,131072]
                                   [--out profiles/map_merge_perf.txt]

  * the kernel (rgbd360_map_time_merge: HIP events, averages over --reps launches, medians over --rounds calls after an untimed one): a
    submap of --frames synthetic frames merged into an empty table (every destination voxel claimed), merged again (every one found),
    taken off (the un-merge kernel), next to ONE k_vmap_extract launch over the submap's table, the cost of merely reading it -- in sum
    mode, at a pose between equal leaves, and at a pose into a destination of 8 x the leaf, where tens of source voxels share a
    destination voxel; with each, the destination voxels created per source voxel (the statistics of a real merge into a fresh map);
  * re-posing (host wall clock per operation, medians over --moves operations after two untimed ones, the paths taking turns): the
    path there was before, --frames x rgbd360_map_move_sphere of the frames that built the submap (from host memory, as a caller that
    kept its frames has them, and from device memory), next to one rgbd360_map_unmerge + rgbd360_map_merge of the submap.  All
    alternate between two poses.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import _lib, synth                                  # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP, pose_to_cm, _ptr  # noqa: E402
from rgbd360_amd.voxel_map import VoxelMap                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--frame", default="2048x1024")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--moves", type=int, default=20, help="re-posing operations timed per path")
    ap.add_argument("--sub-slots", default="524288,131072", help="the submap's table sizes; the re-posing runs on the first")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    W, H = (int(x) for x in a.frame.split("x"))
    K = a.frames
    say("rgbd360_map_merge / rgbd360_map_unmerge: a submap of %d synthetic %dx%d frames at leaf %.3f m, microseconds" % (K, W, H, a.leaf))
    say("(the clock state is not read: the spread between the minimum and the maximum of each figure stands for it)")
    reg = RegisterPhotoICP()
    L = _lib.load()
    world = [synth.trajectory_pose(k, 7) for k in range(K)]
    frames = [synth.render(world[k], W, H, 7) for k in range(K)]
    in_window = [(np.linalg.inv(world[0]) @ world[k]).astype(np.float32) for k in range(K)]
    pose_a = world[0].astype(np.float32)
    shift = np.eye(4)
    shift[:3, :3] = [[np.cos(0.01), -np.sin(0.01), 0], [np.sin(0.01), np.cos(0.01), 0], [0, 0, 1]]
    shift[:3, 3] = [0.03, -0.02, 0.04]
    pose_b = (shift @ world[0]).astype(np.float32)

    def run(capacity, repose):
        sub = VoxelMap(reg, a.leaf, capacity)
        for k in range(K):
            sub.insert_sphere(frames[k][0], frames[k][1], in_window[k], convention=2)
            assert not sub.full
        n_src, n_pts = len(sub), sub.census()["n_points"]
        say("the submap: %d voxels, %d points, in %d slots (table %d MiB)" % (n_src, n_pts, sub.bytes // 64, sub.bytes >> 20))
        # ---- the kernel
        say("kernel: HIP events, averages over %d launches per call, medians over %d calls" % (a.reps, a.rounds))
        for name, dst_leaf, pose in (("sum mode, equal leaves", a.leaf, None), ("pose mode, equal leaves", a.leaf, pose_a),
                                     ("pose mode, destination leaf 8 x", 8 * a.leaf, pose_a)):
            with VoxelMap(reg, dst_leaf, 1 << 20) as dst:
                dst.set_box(None, None)
                g = None if pose is None else pose_to_cm(pose)
                us = []
                for rnd in range(a.rounds + 1):         # (the first round is the warm-up)
                    avg = np.zeros(4, np.float32)
                    rc = L.rgbd360_map_time_merge(dst._handle(), sub._handle(), None if g is None else _ptr(g), a.reps, _ptr(avg))
                    assert rc == 0, (rc, L.rgbd360_map_last_error(dst._h))
                    if rnd:
                        us.append(avg)
                us = np.stack(us)
                med, lo, hi = np.median(us, axis=0), us.min(axis=0), us.max(axis=0)
                assert len(dst) == 0
                st = dst.merge(sub, pose)
                assert not dst.full and st["n_voxels_added"] + st["n_voxels_out_of_range"] == n_src
                say("%s (%d slots): one k_vmap_extract launch over the submap's table %.1f us (min %.1f, max %.1f)"
                    % (name, dst.bytes // 64, med[3], lo[3], hi[3]))
                for k, what in enumerate(("merge into an empty table", "merge into the table that holds it", "un-merge")):
                    say("    %-36s %.1f us (min %.1f, max %.1f) = %.2f scans" % (what + ":", med[k], lo[k], hi[k], med[k] / med[3]))
                say("    %d source voxels -> %d destination voxels: %.4f destination voxels per source voxel, %.1f source voxels per destination voxel"
                    % (st["n_voxels_added"], st["n_voxels_new"], st["n_voxels_new"] / st["n_voxels_added"], st["n_voxels_added"] / st["n_voxels_new"]))
        if not repose:
            sub.close()
            return
        # ---- re-posing
        say("re-posing the submap's content in a global map between two poses (0.01 rad, 5 cm apart): host wall clock per operation, medians over %d, the paths taking turns" % a.moves)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        dev = []
        for rgb, depth in frames:
            pair = []
            for img in (np.ascontiguousarray(rgb), np.ascontiguousarray(depth)):
                p = C.c_void_p()
                assert hip.hipMalloc(C.byref(p), img.nbytes) == 0 and hip.hipMemcpy(p, _ptr(img), img.nbytes, 1) == 0
                pair.append(p)
            dev.append(pair)
        frame_pose = {name: [pose_to_cm((top.astype(np.float64) @ in_window[k].astype(np.float64)).astype(np.float32)) for k in range(K)]
                      for name, top in (("a", pose_a), ("b", pose_b))}

        def wall(call, *args):
            t0 = time.perf_counter()
            call(*args)
            return 1e6 * (time.perf_counter() - t0)

        try:
            with VoxelMap(reg, a.leaf, 1 << 21) as by_frame, VoxelMap(reg, a.leaf, 1 << 21) as by_submap:
                for k in range(K):
                    st = _lib.MapStats()
                    rc = L.rgbd360_map_insert_sphere(by_frame._handle(), _ptr(frames[k][0]), W * 3, _ptr(frames[k][1]), W * 2, 0, H, W, 2, _ptr(frame_pose["a"][k]),
                                                     0, C.byref(st))
                    assert rc == 0
                by_submap.merge(sub, pose_a)
                est, ist = _lib.MapEditStats(), _lib.MapStats()

                def move_frames(where, old, new):
                    for k in range(K):
                        rgb, depth = (dev[k][0], dev[k][1]) if where else (_ptr(frames[k][0]), _ptr(frames[k][1]))
                        rc = L.rgbd360_map_move_sphere(by_frame._handle(), rgb, W * 3, depth, W * 2, 0, H, W, 2, _ptr(frame_pose[old][k]),
                                                       _ptr(frame_pose[new][k]), where, C.byref(est), C.byref(ist))
                        assert rc == 0, (rc, L.rgbd360_map_last_error(by_frame._h))

                def move_submap(old, new):
                    by_submap.unmerge(sub, pose_a if old == "a" else pose_b)
                    by_submap.merge(sub, pose_a if new == "a" else pose_b)
                    assert not by_submap.mismatch and not by_submap.full

                # the three paths take turns, round by round, so that whatever else the host does meets all of them alike
                variants = (("%d x rgbd360_map_move_sphere, frames in host memory" % K, move_frames, (0,), "frames"),
                            ("%d x rgbd360_map_move_sphere, frames in device memory" % K, move_frames, (1,), "frames"),
                            ("rgbd360_map_unmerge + rgbd360_map_merge of the submap", move_submap, (), "submap"))
                at = {"frames": "a", "submap": "a"}
                times = [[] for _ in variants]
                for rnd in range(a.moves + 2):                          # (the first two rounds are the warm-up: there and back)
                    for v, (what, call, args, which) in enumerate(variants):
                        old, new = at[which], "b" if at[which] == "a" else "a"
                        us = wall(call, *args, old, new)
                        at[which] = new
                        if rnd >= 2:
                            times[v].append(us)
                results = []
                for (what, _, _, _), t in zip(variants, times):
                    t = np.array(t)
                    results.append(np.median(t))
                    say("    %-58s %.1f us (min %.1f, quartiles %.1f - %.1f, max %.1f, %d operations)"
                        % (what + ":", np.median(t), t.min(), np.percentile(t, 25), np.percentile(t, 75), t.max(), len(t)))
                say("    frames in host memory / submap %.1f x, frames in device memory / submap %.1f x; the maps hold %d (by frame) and %d (by submap) voxels, "
                    "%d and %d tombstones" % (results[0] / results[2], results[1] / results[2], len(by_frame), len(by_submap),
                                              by_frame.census()["n_tombstones"], by_submap.census()["n_tombstones"]))
        finally:
            for pair in dev:
                for p in pair:
                    hip.hipFree(p)
        sub.close()

    for k, capacity in enumerate(int(v) for v in a.sub_slots.split(",")):
        run(capacity, k == 0)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
