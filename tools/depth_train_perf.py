"""The depth-model trainer's kernel on the device: what k_depth_train costs in each of its three accumulation forms next to the surface
cast of the same rays.

    python tools/depth_train_perf.py [--sizes 320x240,640x480] [--voxels 1000000] [--reps 15] [--rounds 3] [--out profiles/depth_train_perf.txt]

Measured with HIP events, one figure per launch, medians over reps x rounds launches, after an untimed warm-up round of every shape
(rgbd360_depth_trainer_time_map alternates the four launches inside a repetition):
  * k_depth_train over a device image of the sensor's size -- every pixel measured, 1 % off the map's depth, so that nearly every lane
    adds an example -- in form 0 (per-lane 64-bit atomics), 1 (the lanes of equal bin merged over the wave, one atomic per bin and word)
    and 2 (a per-block LDS table flushed once per touched word);
  * the yardstick: one launch of k_vmap_raycast<.., SURFACE> over the same rays, formed here by the definition, writing depth, normal and
    status;
on two maps: the three-wall corner (3 m walls, leaf 0.05) seen from inside, and a surface of --voxels voxels (one point per cell on
z = 0.3 sin x cos y) seen from 2.5 m above.  Bins: 4 x 3 pixels at 320 x 240, 8 x 6 at 640 x 480 (the files' frustums), 2 m slices.
Nobody had measured this: there is no target ratio; the tool reports the numbers and which form is the fastest.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import _lib                                         # noqa: E402
from rgbd360_amd.depth_train import DepthTrainer                     # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP, pose_to_cm, _ptr  # noqa: E402
from rgbd360_amd.voxel_map import VoxelMap                           # noqa: E402

F = np.float32
FORMS = ("per-lane atomics", "per-wave merge", "per-block LDS table")


def corner_cloud(size=3.0, step=0.01):
    g = np.arange(0.0, size, step) + 0.5 * step
    u, v = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    z = np.zeros_like(u)
    return np.concatenate([np.stack(c, axis=1) for c in ((z, u, v), (u, z, v), (u, v, z))]).astype(F)


def surface_cloud(n_voxels, leaf):
    side = int(np.ceil(np.sqrt(n_voxels)))
    g = (np.arange(side) - side // 2 + 0.5) * leaf
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), (0.3 * np.sin(x) * np.cos(y)).ravel()], axis=1).astype(F)


def look_at(eye, target, up):
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(np.asarray(up, float), z)
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T.astype(F)


def pinhole_rays(rows, cols, fx, fy, cx, cy, pose):
    """The map route's rays by its definition: float32, every operation rounded on its own."""
    T = np.asarray(pose, F)
    fxs = np.broadcast_to(((np.arange(cols).astype(F) - F(cx)) / F(fx))[None, :], (rows, cols)).ravel().astype(F)
    fys = np.broadcast_to(((np.arange(rows).astype(F) - F(cy)) / F(fy))[:, None], (rows, cols)).ravel().astype(F)
    dirs = np.stack([(T[k, 0] * fxs + T[k, 1] * fys) + T[k, 2] * F(1) for k in range(3)], axis=1).astype(F)
    return np.ascontiguousarray(np.broadcast_to(T[:3, 3], dirs.shape).astype(F)), np.ascontiguousarray(dirs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="320x240,640x480")
    ap.add_argument("--voxels", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("k_depth_train (rgbd360_depth_trainer_accumulate_map) next to k_vmap_raycast<.., SURFACE> on the same rays: HIP events, one figure per "
        "launch, medians over %d launches (%d per call, %d rounds), leaf %.3f m, default parameters, microseconds" % (a.reps * a.rounds, a.reps, a.rounds, a.leaf))
    say("(the clock state is not read: the spread between the minimum and the maximum of each figure stands for it)")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def to_device(arr):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), arr.nbytes) == 0 and hip.hipMemcpy(p, _ptr(arr), arr.nbytes, 1) == 0
        return p

    reg = RegisterPhotoICP()
    L = _lib.load()
    eye = np.eye(4, dtype=F)
    capacity = 1
    while capacity < 2 * a.voxels:
        capacity <<= 1
    scenes = (("three walls of 3 m", corner_cloud(), 1 << 20, look_at((1.6, 1.3, 1.1), (0.0, 0.0, 0.2), (0, 0, 1))),
              ("surface of %d cells" % a.voxels, surface_cloud(a.voxels, a.leaf), capacity, look_at((0.3, -0.2, 2.5), (1.0, 0.8, 0.0), (0, 1, 0))))
    best = {}
    for what, cloud, cap, pose in scenes:
        with VoxelMap(reg, a.leaf, cap) as m:
            m.set_box(None, None)
            m.insert_cloud(cloud, None, eye)
            assert not m.full
            say("%s: %d voxels in %d slots (table %d MiB)" % (what, len(m), cap, m.bytes >> 20))
            for size in a.sizes.split(","):
                cols, rows = (int(x) for x in size.split("x"))
                k = cols / 320.0
                pin = (262.5 * k, 262.5 * k, 160.0 * k - 0.5, 120.0 * k - 0.5)
                with DepthTrainer(reg, cols, rows, cols // 80, rows // 80, 2.0, 1) as t:
                    gt, _ = t.accumulate_map(m, np.ones((rows, cols), F), *pin, pose, min_mult=0.0, max_mult=1e6)       # the map's depth
                    t.clear()
                    meas = np.where(gt > 0, gt * F(1.01), F(1.0)).astype(F)
                    o, d = pinhole_rays(rows, cols, *pin, pose)
                    meas_d, o_d, d_d = to_device(meas), to_device(o), to_device(d)
                    p = t.params(m)
                    st = _lib.DepthTrainStats()
                    g = pose_to_cm(pose)
                    train, cast = [], []
                    for rnd in range(a.rounds + 1):          # (the first round is the warm-up)
                        tr, ca = np.zeros(3 * a.reps, F), np.zeros(a.reps, F)
                        rc = L.rgbd360_depth_trainer_time_map(t._handle(), m._handle(), meas_d, cols * 4, 1, *[C.c_float(x) for x in pin], _ptr(g), C.byref(p), o_d,
                                                              d_d, a.reps, _ptr(tr), _ptr(ca), C.byref(st))
                        assert rc == 0, (rc, L.rgbd360_depth_trainer_last_error(t._h))
                        if rnd:
                            train.append(tr.reshape(3, a.reps))
                            cast.append(ca)
                    assert not any(x.any() for x in t.sums())          # a measurement leaves the trainer as it was
                    for ptr in (meas_d, o_d, d_d):
                        hip.hipFree(ptr)
                    train, cast = np.concatenate(train, axis=1), np.concatenate(cast)
                    c_us = float(np.median(cast))
                    say("  %dx%d, bins %dx%d: %d pixels, %d examples, %d off the plane, %d without a hit | surface cast %.1f us (min %.1f, max %.1f)"
                        % (cols, rows, cols // 80, rows // 80, st.n_pixels, st.n_examples, st.n_off_plane, st.n_no_hit, c_us, cast.min(), cast.max()))
                    for form in range(3):
                        f_us = train[form]
                        say("      form %d, %-20s %.1f us (min %.1f, max %.1f) | train / cast %.3f x" % (form, FORMS[form] + ":", np.median(f_us), f_us.min(),
                                                                                                     f_us.max(), np.median(f_us) / c_us))
                        best.setdefault(form, []).append(float(np.median(f_us)) / c_us)
    mean = {form: float(np.mean(v)) for form, v in best.items()}
    say("mean train / cast over the shapes: " + ", ".join("form %d %.3f x" % (form, r) for form, r in sorted(mean.items())))
    say("fastest on average: form %d (%s)" % (min(mean, key=mean.get), FORMS[min(mean, key=mean.get)]))
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
