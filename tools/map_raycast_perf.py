"""Ray casting through the voxel map on the device: what the coarse layer costs to build, and what the traversal costs with it and
without it, next to the splat render of the same map and pose and to one scan of the table.

    python tools/map_raycast_perf.py [--map-size 1024x512] [--frames 4] [--reps 15] [--rounds 3] [--leaf 0.05] [--rays 1000000]
                                     [--out profiles/map_raycast_perf.txt]

The map: `frames` frames of the synthetic room along its trajectory at --map-size (uint16 depth, convention 2, the default box) in a
table of 2^20 slots.  Measured with HIP events, one figure per launch, medians over reps x rounds launches, the two forms of the
traversal alternating round by round in one process (rgbd360_map_time_raycast):
  * the layer build (both scans of the table, their clears and the read-back of the brick count between them) next to ONE
    k_vmap_extract launch over the same table, the cost of merely scanning it;
  * the panorama at 2048 x 1024 and at 256 x 128 from the pose behind the last frame, with the layer and with the plain traversal;
  * a list of --rays random rays from points inside the room, both forms;
  * rgbd360_map_render_sphere_dev's whole sequence at the same sizes, map and pose (rgbd360_map_time_render, existing code: the yardstick).
Also: steps and voxel-table lookups per ray of both forms, the layer's size, and that both forms give the same bytes at the timed sizes.
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

FORMS = ("layer", "plain")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-size", default="1024x512")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--rays", type=int, default=1000000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    W, H = (int(x) for x in a.map_size.split("x"))
    say("rgbd360_map_raycast*: HIP events, one figure per launch, medians over %d launches (%d per call, %d rounds, the forms alternating), "
        "leaf %.3f m, default parameters, microseconds" % (a.reps * a.rounds, a.reps, a.rounds, a.leaf))
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
        p = m.raycast_params()
        table_bytes = m.bytes
        say("map: %d frames of %dx%d, %d voxels in a table of %d MiB (%d slots)" % (a.frames, W, H, len(m), table_bytes >> 20, table_bytes // 64))
        # the list: origins around the trajectory's poses, inside the room; directions uniform on the sphere
        rng = np.random.default_rng(3)
        centres = np.stack([synth.trajectory_pose(k, 7)[:3, 3] for k in range(a.frames + 1)])
        o = (centres[rng.integers(0, len(centres), a.rays)] + rng.uniform(-0.3, 0.3, size=(a.rays, 3))).astype(np.float32)
        d = rng.normal(size=(a.rays, 3)).astype(np.float32)
        dev_o, dev_d = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(dev_o), o.nbytes) == 0 and hip.hipMalloc(C.byref(dev_d), d.nbytes) == 0
        assert hip.hipMemcpy(dev_o, _ptr(o), o.nbytes, 1) == 0 and hip.hipMemcpy(dev_d, _ptr(d), d.nbytes, 1) == 0

        def timed(job, plain, reps):
            """job: (rows, cols) or "list".  Returns (build_us, cast_us, scan_us, stats, layer_bytes)."""
            b, c, s = (np.zeros(reps, np.float32) for _ in range(3))
            st = _lib.MapRaycastStats()
            nbytes = C.c_longlong(0)
            if job == "list":
                rc = m._L.rgbd360_map_time_raycast(m._handle(), a.rays, dev_o, dev_d, 0, 0, None, C.byref(p), plain, reps, _ptr(b), _ptr(c), _ptr(s),
                                                   C.byref(st), C.byref(nbytes))
            else:
                rc = m._L.rgbd360_map_time_raycast(m._handle(), 0, None, None, job[0], job[1], _ptr(pose), C.byref(p), plain, reps, _ptr(b), _ptr(c), _ptr(s),
                                                   C.byref(st), C.byref(nbytes))
            assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
            return b, c, s, {k: getattr(st, k) for k, _ in st._fields_}, nbytes.value

        jobs = [(1024, 2048), (128, 256), "list"]
        names = {(1024, 2048): "panorama 2048x1024", (128, 256): "panorama 256x128", "list": "%d random rays" % a.rays}
        # the same bytes from both forms at the timed sizes
        for rows, cols in jobs[:2]:
            lay = m.raycast_sphere(rows, cols, T)
            m.raycast_set_plain(True)
            pla = m.raycast_sphere(rows, cols, T)
            m.raycast_set_plain(False)
            same = all(x.tobytes() == y.tobytes() for x, y in zip(lay[:4], pla[:4]))
            say("%s: both forms give the same bytes: %s" % (names[(rows, cols)], same))
            assert same
        cast = {(j, f): [] for j in jobs for f in (0, 1)}
        build, scan, stats = [], [], {}
        layer_bytes = 0
        for job in jobs:          # warm-up: every shape and form once, untimed
            for plain in (0, 1):
                timed(job, plain, 1)
        for rnd in range(a.rounds):
            for job in jobs:
                for plain in (0, 1):
                    b, c, s, st, nb = timed(job, plain, a.reps)
                    cast[(job, plain)].append(c)
                    build.append(b)
                    scan.append(s)
                    stats[(job, plain)] = st
                    layer_bytes = nb
        say("layer build %.1f us (median; min %.1f, max %.1f) | one k_vmap_extract launch over the table %.1f us | build / scan %.2f x"
            % (np.median(np.concatenate(build)), np.min(np.concatenate(build)), np.max(np.concatenate(build)), np.median(np.concatenate(scan)),
               np.median(np.concatenate(build)) / np.median(np.concatenate(scan))))
        say("layer: %.2f MiB (%.0f %% of the table's %d MiB)" % (layer_bytes / 2 ** 20, 100.0 * layer_bytes / table_bytes, table_bytes >> 20))
        render = {}
        rp = m.render_params()
        for rows, cols in jobs[:2]:
            us = []
            for rnd in range(a.rounds):
                r5 = np.zeros(5, np.float32)
                rst = _lib.MapRenderStats()
                rc = m._L.rgbd360_map_time_render(m._handle(), rows, cols, _ptr(pose), C.byref(rp), 0, a.reps, _ptr(r5), C.byref(rst), None)
                assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
                us.append(float(r5[3]))
            render[(rows, cols)] = (float(np.median(us)), rst.n_pixels_covered)
        for job in jobs:
            lay, pla = np.concatenate(cast[(job, 0)]), np.concatenate(cast[(job, 1)])
            st0, st1 = stats[(job, 0)], stats[(job, 1)]
            n = st0["n_rays"]
            say("%s: layer %.1f us (min %.1f, max %.1f) | plain %.1f us (min %.1f, max %.1f) | layer / plain %.2f x"
                % (names[job], np.median(lay), lay.min(), lay.max(), np.median(pla), pla.min(), pla.max(), np.median(lay) / np.median(pla)))
            say("    %d rays, %d hits; per ray: %.1f cells stepped, %.2f voxel-table lookups with the layer, %.1f without; %.1f ns per ray with the layer"
                % (n, st0["n_hits"], st0["n_steps"] / n, st0["n_lookups"] / n, st1["n_lookups"] / n, 1e3 * np.median(lay) / n))
            assert {k: v for k, v in st0.items() if k != "n_lookups"} == {k: v for k, v in st1.items() if k != "n_lookups"}
            if job in render:
                say("    rgbd360_map_render_sphere_dev, whole sequence, same map and pose: %.1f us (average of %d launches, median of %d rounds), %d pixels covered; "
                    "ray cast with the layer / splat %.2f x" % (render[job][0], a.reps, a.rounds, render[job][1], np.median(lay) / render[job][0]))
        hip.hipFree(dev_o)
        hip.hipFree(dev_d)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
