"""Planar regions of the voxel map on the device: what the segmentation costs to build, stage by stage, next to one scan of the same table
and to the build of the normal layer it reads.

    python tools/map_planes_perf.py [--voxels 100000,1000000] [--reps 10] [--rounds 3] [--leaf 0.02] [--wall-leaf 0.01]
                                    [--out profiles/map_planes_perf.txt]

Measured with HIP events, one figure per launch (rgbd360_map_time_planes: every stage of a rebuild between two events of its own; the host
work between the stages -- three waits, the sort of the roots, the fits -- is in none of them), medians over reps x rounds rebuilds after
an untimed warm-up round, with the minimum and the maximum:
  * on a surface of --voxels voxels, one point per cell on z = 0.3 sin x cos y (the table of tools/map_normals_perf.py), the table twice
    the voxels rounded up to a power of two, next to ONE k_vmap_extract launch over the same table and to the build of the normal layer
    (rgbd360_map_time_normals);
  * on one flat wall of the largest --voxels count, where every voxel adds into ONE region's sums: the sums pass with its per-wave merge
    and without it, and the scatter and extremes passes, which only run for planes that pass the filters.
The leaf is smaller than the other tools' 0.05 m because a single region of 10^6 voxels 1000 cells across is out of the range rule of
the sums at 0.05 m (rgbd360_hip.h: N ((E + 2) leaf 2^16)^2 < 2^62) and the call refuses it.
The expectation to confirm or refute: the link pass costs about what the normal build costs, and the whole segmentation stays within a
small multiple of it.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import _lib                                # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP, _ptr     # noqa: E402
from rgbd360_amd.voxel_map import VoxelMap                  # noqa: E402

STAGES = ("init", "link", "compress", "count", "roots", "sums", "scatter", "extremes")


def surface_cloud(n_voxels, leaf, flat=False):
    """One point per cell of a side x side patch on z = 0.3 sin x cos y (flat: on z = half a cell), side = ceil(sqrt(n_voxels))."""
    side = int(np.ceil(np.sqrt(n_voxels)))
    g = (np.arange(side) - side // 2 + 0.5) * leaf
    x, y = np.meshgrid(g, g, indexing="ij")
    z = np.full(x.shape, 0.5 * leaf) if flat else 0.3 * np.sin(x) * np.cos(y)
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.02)
    ap.add_argument("--wall-leaf", type=float, default=0.01)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("rgbd360_map_planes: HIP events, one figure per launch, medians over %d rebuilds (%d per call, %d rounds), default parameters, microseconds"
        % (a.reps * a.rounds, a.reps, a.rounds))
    say("(the clock state is not read: the spread between the minimum and the maximum of each figure stands for it)")
    reg = RegisterPhotoICP()
    L = _lib.load()
    eye = np.eye(4, dtype=np.float32)
    fig = lambda v: "%.1f (min %.1f, max %.1f)" % (np.median(v), v.min(), v.max())

    def stages(m, p, merge):
        """[rounds * reps, 8] stage times of rebuilds, or the return code where the call refuses the map."""
        got, st = [], _lib.MapPlaneSegStats()
        for rnd in range(a.rounds + 1):          # (the first round is the warm-up)
            us = np.zeros((a.reps, 8), np.float32)
            rc = L.rgbd360_map_time_planes(m._handle(), C.byref(p), a.reps, merge, _ptr(us), C.byref(st))
            if rc != 0:
                return rc, L.rgbd360_map_last_error(m._h).decode()
            if rnd:
                got.append(us)
        return np.concatenate(got), st

    def report(us, st):
        say("    " + " | ".join("%s %s" % (name, fig(us[:, k])) for k, name in enumerate(STAGES)))
        say("    voxels %d, eligible %d, links %d, regions %d, planes %d holding %d voxels"
            % (st.n_voxels, st.n_eligible, st.n_links, st.n_regions, st.n_planes_available, st.n_voxels_in_planes))

    sizes = [int(v) for v in a.voxels.split(",")]
    for n_voxels in sizes:
        capacity = 1
        while capacity < 2 * n_voxels:
            capacity <<= 1
        with VoxelMap(reg, a.leaf, capacity) as m:
            m.set_box(None, None)
            m.insert_cloud(surface_cloud(n_voxels, a.leaf), None, eye)
            assert not m.full
            build, scan = [], []
            np_, nst = m.normal_params(), _lib.MapNormalStats()
            for rnd in range(a.rounds + 1):
                b, s = np.zeros(a.reps, np.float32), np.zeros(a.reps, np.float32)
                rc = L.rgbd360_map_time_normals(m._handle(), C.byref(np_), a.reps, _ptr(b), _ptr(s), C.byref(nst), None)
                assert rc == 0, (rc, L.rgbd360_map_last_error(m._h))
                if rnd:
                    build.append(b)
                    scan.append(s)
            build, scan = np.concatenate(build), np.concatenate(scan)
            say("surface z = 0.3 sin x cos y, leaf %.3f m: %d voxels in %d slots (table %d MiB)" % (a.leaf, len(m), capacity, m.bytes >> 20))
            say("    one k_vmap_extract launch over the table %s | the normal layer's build %s" % (fig(scan), fig(build)))
            us, st = stages(m, m.plane_seg_params(), 1)
            if isinstance(us, int):
                say("    rgbd360_map_planes refuses this map (%d): %s" % (us, st))
                continue
            report(us, st)
            whole = us.sum(axis=1)
            say("    the eight stages together %s = %.2f x the normal build, %.2f x the scan; link / normal build %.2f x; label layer and lists %d MiB"
                % (fig(whole), np.median(whole) / np.median(build), np.median(whole) / np.median(scan), np.median(us[:, 1]) / np.median(build),
                   m.plane_bytes() >> 20))
    # ---- one wall: every voxel adds into the same nine sums
    n_voxels = max(sizes)
    capacity = 1
    while capacity < 2 * n_voxels:
        capacity <<= 1
    with VoxelMap(reg, a.wall_leaf, capacity) as m:
        m.set_box(None, None)
        m.insert_cloud(surface_cloud(n_voxels, a.wall_leaf, flat=True), None, eye)
        assert not m.full
        say("one flat wall, leaf %.3f m: %d voxels in %d slots" % (a.wall_leaf, len(m), capacity))
        for merge in (1, 0):
            us, st = stages(m, m.plane_seg_params(), merge)
            if isinstance(us, int):
                say("    rgbd360_map_planes refuses this map (%d): %s" % (us, st))
                break
            say("  the sums pass %s:" % ("with its per-wave merge of equal regions (as shipped)" if merge else "with every lane adding on its own"))
            report(us, st)
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
