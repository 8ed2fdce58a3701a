"""Free-space observation and carving of the voxel map on the device: what an observation of a frame costs next to the ray-cast panorama
of the same size, map and pose (this walk visits every cell up to the measurement, that one stops at the first hit), and what the
carve's scan of the table costs.

    python tools/map_carve_perf.py [--map-size 1024x512] [--frames 4] [--reps 15] [--rounds 3] [--leaf 0.05] [--phantom 200000]
                                   [--out profiles/map_carve_perf.txt]

The map: `frames` frames of the synthetic room along its trajectory at --map-size (uint16 depth, convention 2, the default box) in a
table of 2^20 slots -- the map of tools/map_raycast_perf.py -- plus a phantom cube of --phantom points in the room's free space, so that
there is something to see through.  Measured with HIP events, one figure per launch, medians over reps x rounds
launches, the kernels alternating round by round in one process:
  * rgbd360_map_observe_sphere's kernel over the frame behind the last one, at 2048 x 1024 and at 256 x 128 (device image, uint16), with
    the coarse layer and with the plain walk (rgbd360_map_time_observe);
  * rgbd360_map_raycast_sphere's kernel at the same sizes, map and pose (rgbd360_map_time_raycast, existing code: the yardstick);
  * ONE k_vmap_carve launch over the table with thresholds nothing meets (the scan), next to one k_vmap_extract launch over it.
Also: cells and lookups per measurement, the votes given, the vote array's bytes, and what a carve at the defaults then erases.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-size", default="1024x512")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--phantom", type=int, default=200000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    W, H = (int(x) for x in a.map_size.split("x"))
    say("rgbd360_map_observe_sphere / rgbd360_map_carve: HIP events, one figure per launch, medians over %d launches (%d per call, %d rounds, the kernels "
        "alternating), leaf %.3f m, default parameters, microseconds" % (a.reps * a.rounds, a.reps, a.rounds, a.leaf))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    reg = RegisterPhotoICP()
    with VoxelMap(reg, a.leaf, 1 << 20) as m:
        for k in range(a.frames):
            rgb, depth = synth.render(synth.trajectory_pose(k, 7), W, H, 7)
            m.insert_sphere(rgb, depth, synth.trajectory_pose(k, 7).astype(np.float32), convention=2)
            assert not m.full
        T = synth.trajectory_pose(a.frames, 7).astype(np.float32)
        pose = pose_to_cm(T)
        # something to see through: a cube of 0.4 m of points that no frame contains, 1 m from the observing pose (an accurate map of a
        # static room gives an observation nothing to vote on but the end-votes)
        rng = np.random.default_rng(3)
        phantom = (T[:3, 3].astype(np.float64) + np.array([0.1, 0.6, 0.8]) + rng.uniform(-0.2, 0.2, size=(a.phantom, 3))).astype(np.float32)
        n_room = len(m)
        m.insert_cloud(phantom, None, np.eye(4, dtype=np.float32))
        assert not m.full
        say("phantom: %d points in a cube of 0.4 m, %d voxels, next to the room's %d" % (a.phantom, len(m) - n_room, n_room))
        table_bytes = m.bytes
        say("map: %d frames of %dx%d, %d voxels in a table of %d MiB (%d slots)" % (a.frames, W, H, len(m), table_bytes >> 20, table_bytes // 64))
        sizes = [(1024, 2048), (128, 256)]
        dev = {}
        for rows, cols in sizes:
            depth = np.ascontiguousarray(synth.render(synth.trajectory_pose(a.frames, 7), cols, rows, 7)[1])
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), depth.nbytes) == 0 and hip.hipMemcpy(p, _ptr(depth), depth.nbytes, 1) == 0
            dev[(rows, cols)] = p
        op, rp = m.observe_params(), m.raycast_params()

        def observe(size, plain, reps):
            o, c = np.zeros(reps, np.float32), np.zeros(reps, np.float32)
            st = _lib.MapObserveStats()
            rc = m._L.rgbd360_map_time_observe(m._handle(), dev[size], size[1] * 2, 0, size[0], size[1], 2, _ptr(pose), C.byref(op), plain, reps, _ptr(o), _ptr(c),
                                               C.byref(st))
            assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
            return o, c, {k: getattr(st, k) for k, _ in st._fields_}

        def raycast(size, plain, reps):
            b, c, s = (np.zeros(reps, np.float32) for _ in range(3))
            rc = m._L.rgbd360_map_time_raycast(m._handle(), 0, None, None, size[0], size[1], _ptr(pose), C.byref(rp), plain, reps, _ptr(b), _ptr(c), _ptr(s), None,
                                               None)
            assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
            return c, s

        for size in sizes:          # warm-up: every shape and form once, untimed
            for plain in (0, 1):
                observe(size, plain, 1)
                raycast(size, plain, 1)
        obs = {(s, f): [] for s in sizes for f in (0, 1)}
        ray = {(s, f): [] for s in sizes for f in (0, 1)}
        carve, scan, stats = [], [], {}
        for rnd in range(a.rounds):
            for size in sizes:
                for plain in (0, 1):
                    o, c, st = observe(size, plain, a.reps)
                    obs[(size, plain)].append(o)
                    carve.append(c)
                    stats[(size, plain)] = st
                    c, s = raycast(size, plain, a.reps)
                    ray[(size, plain)].append(c)
                    scan.append(s)
        for size in sizes:
            lay, pla = np.concatenate(obs[(size, 0)]), np.concatenate(obs[(size, 1)])
            rl, rpl = np.concatenate(ray[(size, 0)]), np.concatenate(ray[(size, 1)])
            st0, st1 = stats[(size, 0)], stats[(size, 1)]
            n = st0["n_rays"]
            say("observe %dx%d: layer %.1f us (min %.1f, max %.1f) | plain %.1f us (min %.1f, max %.1f) | layer / plain %.2f x"
                % (size[1], size[0], np.median(lay), lay.min(), lay.max(), np.median(pla), pla.min(), pla.max(), np.median(lay) / np.median(pla)))
            say("    ray-cast panorama, same size, map and pose: layer %.1f us (min %.1f, max %.1f) | plain %.1f us | observe / ray cast %.2f x with the layer, "
                "%.2f x plain" % (np.median(rl), rl.min(), rl.max(), np.median(rpl), np.median(lay) / np.median(rl), np.median(pla) / np.median(rpl)))
            say("    %d measurements, %d valid; per measurement: %.1f cells stepped, %.2f voxel-table lookups with the layer, %.1f without; %d through-votes, "
                "%d end-votes on %d voxels; %.1f ns per measurement with the layer"
                % (n, st0["n_valid"], st0["n_steps"] / n, st0["n_lookups"] / n, st1["n_lookups"] / n, st0["n_through"], st0["n_end"], st0["n_voxels_voted"],
                   1e3 * np.median(lay) / n))
            assert {k: v for k, v in st0.items() if k != "n_lookups"} == {k: v for k, v in st1.items() if k != "n_lookups"}
        carve, scan = np.concatenate(carve), np.concatenate(scan)
        slots = table_bytes // 64
        say("carve scan over %d slots: %.1f us (min %.1f, max %.1f) = %.1f us per million slots | one k_vmap_extract launch over the table %.1f us | "
            "carve / extract %.2f x" % (slots, np.median(carve), carve.min(), carve.max(), np.median(carve) * 1e6 / slots, np.median(scan),
                                        np.median(carve) / np.median(scan)))
        say("vote array: %.1f MiB (8 bytes per slot, %.1f %% of the table)" % (m.vote_bytes() / 2 ** 20, 100.0 * m.vote_bytes() / table_bytes))
        # the votes of the last timed observation are current: what a carve at the defaults erases
        before = len(m)
        cs = m.carve()
        say("carve at the defaults after the last observation: %d voxels voted, %d of %d erased (%d points), %d protected by end-votes"
            % (cs["n_voted"], cs["n_voxels_carved"], before, cs["n_points_carved"], cs["n_protected_end"]))
        for p in dev.values():
            hip.hipFree(p)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
