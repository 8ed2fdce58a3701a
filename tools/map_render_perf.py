"""The kernels of the map rendered as a spherical frame on the device: what the two scans of the table and the resolve pass cost next
to one extract launch over the same table, in both forms of the footprint loop.

    python tools/map_render_perf.py [--size 2048x1024] [--frames 4] [--reps 20] [--rounds 3] [--leaf 0.02] [--out profiles/map_render_perf.txt]

The map: `frames` frames of the synthetic room along its trajectory at --size (uint16 depth, convention 2, the default box), a few 10^5
voxels in a table of 2^20 slots (leaf 0.02 m: the room's surfaces hold about 3 10^5 such cells).  Rendered at the pose behind the last frame at the same size with the default parameters, from HIP
events in ONE call per form and round (rgbd360_map_time_render): k_vmap_render_depth, k_vmap_render_key, k_vmap_render_resolve, the
whole sequence with its three clears, and ONE k_vmap_extract launch (centroids only) over the same table -- the cost of merely scanning
it.  Also the atomics the depth pass issues per splatted voxel, and the byte floor: the table read twice plus the planes (the two
clears, 12 B/px; the resolve's reads, 12 B/px; the four output planes, 23 B/px).
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

FORMS = ("a lane per voxel", "a wave shares its voxels' footprints")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048x1024")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.02)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    W, H = (int(x) for x in a.size.split("x"))
    say("rgbd360_map_render_*: HIP-event averages over %d launches, %d rounds, leaf %.3f m, default parameters, microseconds" % (a.reps, a.rounds, a.leaf))
    reg = RegisterPhotoICP()
    with VoxelMap(reg, a.leaf, 1 << 20) as m:
        for k in range(a.frames):
            rgb, depth = synth.render(synth.trajectory_pose(k, 7), W, H, 7)
            m.insert_sphere(rgb, depth, synth.trajectory_pose(k, 7).astype(np.float32), convention=2)
        pose = pose_to_cm(synth.trajectory_pose(a.frames, 7).astype(np.float32))
        p = m.render_params()
        table_bytes = m.bytes
        say("%dx%d: %d frames, %d voxels in a table of %d MiB (%d slots)" % (W, H, a.frames, len(m), table_bytes >> 20, table_bytes // 64))
        n = W * H
        rows = {}
        for rnd in range(a.rounds):
            for form in (0, 1):
                us = np.zeros(5, np.float32)
                st = _lib.MapRenderStats()
                atomics = C.c_longlong(0)
                rc = m._L.rgbd360_map_time_render(m._handle(), H, W, _ptr(pose), C.byref(p), form, a.reps, _ptr(us), C.byref(st), C.byref(atomics))
                assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._h))
                rows.setdefault(form, []).append(us.copy())
                if rnd == 0 and form == 0:
                    say("    one render: %d voxels splatted, %d skipped (near / not visible), %d pixels covered of %d; %d atomicMin in the depth pass = "
                        "%.1f per splatted voxel (the key pass issues at most as many)"
                        % (st.n_splatted, st.n_near, st.n_pixels_covered, n, atomics.value, atomics.value / max(st.n_splatted, 1)))
                say("    round %d, %s: k_vmap_render_depth %.1f | k_vmap_render_key %.1f | k_vmap_render_resolve %.1f | whole sequence %.1f | "
                    "one k_vmap_extract launch %.1f" % (rnd, FORMS[form], us[0], us[1], us[2], us[3], us[4]))
        for form in (0, 1):
            med = np.median(np.stack(rows[form]), axis=0)
            say("    median, %s: depth %.1f | key %.1f | resolve %.1f | whole %.1f | extract %.1f; depth / extract %.2f x"
                % (FORMS[form], med[0], med[1], med[2], med[3], med[4], med[0] / med[4]))
        floor = 2 * table_bytes + (12 + 12 + 23) * n
        med = np.median(np.stack(rows[0]), axis=0)
        say("    byte floor: the table twice (%d MiB) + 47 B/px of planes (%d MiB) = %d MiB; the whole sequence moves them at %.0f GB/s (form 0)"
            % (2 * table_bytes >> 20, 47 * n >> 20, floor >> 20, floor / med[3] * 1e-3))
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
