"""Surface normals of the voxel map on the device: what the normal layer costs to build, next to one scan of the same table, and what
the surface cast costs next to the plain ray cast of the same map and pose.

    python tools/map_normals_perf.py [--voxels 100000,1000000] [--map-size 1024x512] [--frames 4] [--reps 15] [--rounds 3] [--leaf 0.05]
                                     [--out profiles/map_normals_perf.txt]

Measured with HIP events, one figure per launch, medians over reps x rounds launches, after an untimed warm-up of every shape:
  * the layer build (one k_vmap_normals launch over the slots with the clear of its counters; rgbd360_map_time_normals) on a surface of
    --voxels voxels -- one point per cell on z = 0.3 sin x cos y, the table twice the voxels rounded up to a power of two -- next to ONE
    k_vmap_extract launch over the same table, the cost of merely scanning it;
  * rgbd360_map_raycast_surface_sphere_dev at 2048 x 1024 with a warm layer, on `frames` frames of the synthetic room at --map-size in a
    table of 2^20 slots, from the pose behind the last frame, next to rgbd360_map_raycast_sphere_dev timed the same way (two events
    around the enqueued call) and to rgbd360_map_time_raycast's figure for the traversal launch alone (existing code: the yardstick).
The expectation to confirm or refute: the surface cast adds one 16-byte gather per hit to the plain cast.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import _lib, synth                                  # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP, pose_to_cm, _ptr  # noqa: E402
from rgbd360_amd.voxel_map import VoxelMap                           # noqa: E402


def surface_cloud(n_voxels, leaf):
    """One point per cell of a side x side patch on z = 0.3 sin x cos y, side = ceil(sqrt(n_voxels)): about n_voxels voxels."""
    side = int(np.ceil(np.sqrt(n_voxels)))
    g = (np.arange(side) - side // 2 + 0.5) * leaf
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), (0.3 * np.sin(x) * np.cos(y)).ravel()], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", default="100000,1000000")
    ap.add_argument("--map-size", default="1024x512")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("rgbd360_map_normals / rgbd360_map_raycast_surface*: HIP events, one figure per launch, medians over %d launches (%d per call, %d rounds), "
        "leaf %.3f m, default parameters, microseconds" % (a.reps * a.rounds, a.reps, a.rounds, a.leaf))
    say("(the clock state is not read: the spread between the minimum and the maximum of each figure stands for it)")
    hip =C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    reg = RegisterPhotoICP()
    L = _lib.load()
    eye = np.eye(4, dtype=np.float32)
    # ---- the layer build
    for n_voxels in (int(v) for v in a.voxels.split(",")):
        capacity = 1
        while capacity < 2 * n_voxels:
            capacity <<= 1
        cloud = surface_cloud(n_voxels, a.leaf)
        with VoxelMap(reg, a.leaf, capacity) as m:
            m.set_box(None, None)
            m.insert_cloud(cloud, None, eye)
            assert not m.full
            p = m.normal_params()
            build, scan = [], []
            st, nbytes = _lib.MapNormalStats(), C.c_longlong(0)
            for rnd in range(a.rounds + 1):          # (the first round is the warm-up)
                b, s = np.zeros(a.reps, np.float32), np.zeros(a.reps, np.float32)
                rc = L.rgbd360_map_time_normals(m._handle(), C.byref(p), a.reps, _ptr(b), _ptr(s), C.byref(st), C.byref(nbytes))
                assert rc == 0, (rc, L.rgbd360_map_last_error(m._h))
                if rnd:
                    build.append(b)
                    scan.append(s)
            build, scan = np.concatenate(build), np.concatenate(scan)
            say("layer build, %d voxels in %d slots (table %d MiB, layer %d MiB): %.1f us (min %.1f, max %.1f) | one k_vmap_extract launch over the "
                "table %.1f us (min %.1f, max %.1f) | build / scan %.2f x | %.2f ns per voxel"
                % (len(m), capacity, m.bytes >> 20, nbytes.value >> 20, np.median(build), build.min(), build.max(), np.median(scan), scan.min(), scan.max(),
                   np.median(build) / np.median(scan), 1e3 * np.median(build) / len(m)))
            say("    normals %d, unsupported %d, nonplanar %d, below min_count %d" % (st.n_normals, st.n_unsupported, st.n_nonplanar, st.n_below_min_count))
    # ---- the surface cast
    W, H = (int(x) for x in a.map_size.split("x"))
    rows, cols = 1024, 2048
    n = rows * cols
    with VoxelMap(reg, a.leaf, 1 << 20) as m:
        for k in range(a.frames):
            rgb, depth = synth.render(synth.trajectory_pose(k, 7), W, H, 7)
            m.insert_sphere(rgb, depth, synth.trajectory_pose(k, 7).astype(np.float32), convention=2)
            assert not m.full
        pose = pose_to_cm(synth.trajectory_pose(a.frames, 7).astype(np.float32))
        say("surface cast: %d frames of %dx%d, %d voxels in a table of %d MiB; panorama %dx%d" % (a.frames, W, H, len(m), m.bytes >> 20, cols, rows))
        sizes = [4 * n, 12 * n, 3 * n, 4 * n, 12 * n, 8, 72]
        dev = [C.c_void_p() for _ in sizes]
        for ptr, s in zip(dev, sizes):
            assert hip.hipMalloc(C.byref(ptr), s) == 0
        depth_d, normal_d, rgb_d, count_d, key_d, plane_d, stats_d = dev
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        stream = L.rgbd360_stream(reg._ctx())

        def surface():
            return L.rgbd360_map_raycast_surface_sphere_dev(m._handle(), rows, cols, _ptr(pose), None, None, depth_d, normal_d, rgb_d, count_d, key_d, plane_d,
                                                            stats_d)

        def plain():
            return L.rgbd360_map_raycast_sphere_dev(m._handle(), rows, cols, _ptr(pose), None, depth_d, rgb_d, count_d, key_d, stats_d)

        def timed(call):
            ms = C.c_float(0)
            assert hip.hipEventRecord(e0, stream) == 0 and call() == 0 and hip.hipEventRecord(e1, stream) == 0
            assert hip.hipEventSynchronize(e1) == 0 and hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            return 1e3 * ms.value

        for call in (surface, plain, surface, plain):          # warm-up: the layers built, code loaded
            timed(call)
        us = {surface: [], plain: []}
        for rnd in range(a.rounds):
            for call in (surface, plain):
                us[call] += [timed(call) for _ in range(a.reps)]
        depth, normal, _, _, _, on_plane, stats = m.raycast_surface_sphere(rows, cols, synth.trajectory_pose(a.frames, 7).astype(np.float32))
        c = np.zeros(a.reps * a.rounds, np.float32)
        b = np.zeros(a.reps * a.rounds, np.float32)
        rp = m.raycast_params()
        rc = L.rgbd360_map_time_raycast(m._handle(), 0, None, None, rows, cols, _ptr(pose), C.byref(rp), 0, a.reps * a.rounds, _ptr(b), _ptr(c), None, None, None)
        assert rc == 0, (rc, L.rgbd360_map_last_error(m._h))
        s_us, p_us = np.array(us[surface]), np.array(us[plain])
        say("rgbd360_map_raycast_surface_sphere_dev %.1f us (min %.1f, max %.1f) | rgbd360_map_raycast_sphere_dev %.1f us (min %.1f, max %.1f) | "
            "surface / plain %.3f x | the traversal launch alone (rgbd360_map_time_raycast) %.1f us"
            % (np.median(s_us), s_us.min(), s_us.max(), np.median(p_us), p_us.min(), p_us.max(), np.median(s_us) / np.median(p_us), np.median(c)))
        say("    %d rays, %d hits, %d on the plane, %d with a normal; the surface cast's extra per call: %.1f us = %.2f ns per hit (a 16-byte record "
            "gather, the plane arithmetic and 12 more output bytes per ray)"
            % (stats["n_rays"], stats["n_hits"], on_plane, int(normal.any(axis=2).sum()), np.median(s_us) - np.median(p_us),
               1e3 * (np.median(s_us) - np.median(p_us)) / max(stats["n_hits"], 1)))
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        for ptr in dev:
            hip.hipFree(ptr)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
