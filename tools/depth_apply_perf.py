"""Applying the depth models on the device: what the three kernels of csrc/depth_apply.h cost next to their yardsticks.

    python tools/depth_apply_perf.py [--sizes 320x240,640x480] [--sensors 8] [--reps 15] [--rounds 3] [--out profiles/depth_apply_perf.txt]

Kernel times are HIP events in front of and behind the launch inside the entry (rgbd360_depth_apply_timing, rgbd360_hip_diag.h), one
figure per call, medians over reps x rounds calls after an untimed warm-up round; the host route is wall-clock time.  Per size, a rig of
--sensors sensors whose models are the reference's distortion_model1 .. 8 (bins and, below 640 x 480, image size down-sampled):
  (a) rgbd360_depth_undistort over the S float32 images in device memory (one launch), next to a device-to-device copy of the same
      bytes between the same events, and next to the host route it replaces: S x rgbd360_depth_model_undistort plus the upload of the
      S float images;
  (b) rgbd360_rig_depth_clouds with the set next to the same entry with set NULL, which is k_rig_pinhole_cloud as
      rgbd360_map_calibrate_rig_depth launches it;
  (c) rgbd360_depth_evaluate_map next to k_depth_train in its default form (rgbd360_depth_trainer_time_map) on the same rays and map:
      three walls of 3 m at leaf 0.05 seen from inside, every pixel measured 1 % off the map's depth.
Nobody had measured this: there is no target ratio; the tool reports the numbers.
"""
import argparse
import ctypes as C
import lzma
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rgbd360_amd import _lib                                                # noqa: E402
from rgbd360_amd.depth_train import DepthModels, DepthTrainer               # noqa: E402
from rgbd360_amd.register import DepthModel, RegisterPhotoICP, pose_to_cm, _ptr  # noqa: E402
from rgbd360_amd.voxel_map import VoxelMap                                  # noqa: E402
from depth_train_perf import corner_cloud, look_at, pinhole_rays            # noqa: E402

F = np.float32
MODELS = os.path.join(ROOT, "tests", "golden", "depth_models")


def med(v):
    v = np.asarray(v, float)
    return "%.1f us (min %.1f, max %.1f)" % (np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="320x240,640x480")
    ap.add_argument("--sensors", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n_calls = a.reps * a.rounds
    say("depth_apply.h's kernels next to their yardsticks: HIP events around the launch, one figure per call, medians over %d calls after a warm-up "
        "round; host route: wall clock; %d sensors, the reference's distortion models" % (n_calls, a.sensors))
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
    ctx = reg._ctx()
    assert L.rgbd360_depth_apply_timing(ctx, 1) == 0

    def last_us():
        us = C.c_float()
        assert L.rgbd360_depth_apply_last_us(ctx, C.byref(us)) == 0
        return us.value

    S = a.sensors
    pose = look_at((1.6, 1.3, 1.1), (0.0, 0.0, 0.2), (0, 0, 1))
    with tempfile.TemporaryDirectory() as tmp, VoxelMap(reg, a.leaf, 1 << 20) as m:
        for k in range(8):
            with open(os.path.join(tmp, "m%d" % k), "wb") as f:
                f.write(lzma.decompress(open(os.path.join(MODELS, "distortion_model%d.xz" % (k + 1)), "rb").read()))
        m.set_box(None, None)
        m.insert_cloud(corner_cloud(), None, np.eye(4, dtype=F))
        assert not m.full
        for size in a.sizes.split(","):
            cols, rows = (int(x) for x in size.split("x"))
            down = 640 // cols
            host_models = [DepthModel(os.path.join(tmp, "m%d" % (s % 8)), down) for s in range(S)]
            assert (host_models[0].width, host_models[0].height) == (cols, rows)
            k = cols / 320.0
            pin = (262.5 * k, 262.5 * k, 160.0 * k - 0.5, 120.0 * k - 0.5)
            fpin = [C.c_float(x) for x in pin]
            rng = np.random.default_rng(cols)
            n = rows * cols
            with DepthModels(reg, host_models) as models, DepthTrainer(reg, cols, rows, cols // 80, rows // 80, 2.0, 1) as t:
                gt, _ = t.accumulate_map(m, np.ones((rows, cols), F), *pin, pose, min_mult=0.0, max_mult=1e6)       # the map's depth
                t.clear()
                meas = np.where(gt > 0, gt * F(1.01), F(1.0)).astype(F)
                images = [np.where(rng.random((rows, cols)) < 0.05, F(0), rng.uniform(0.4, 9.5, size=(rows, cols))).astype(F) for _ in range(S)]
                whole = np.stack(images)             # the S images side by side in ONE allocation: the copy yardstick is one copy
                d_all_in, d_all_out = to_device(whole), to_device(whole)
                d_in = [C.c_void_p(d_all_in.value + s * n * 4) for s in range(S)]
                d_out = [C.c_void_p(d_all_out.value + s * n * 4) for s in range(S)]
                d_cloud = to_device(np.zeros((S, n, 3), F))
                d_meas = to_device(meas)
                o, d = pinhole_rays(rows, cols, *pin, pose)
                d_o, d_d = to_device(o), to_device(d)
                I = (_lib.MapBatchFrame * S)()
                for s in range(S):
                    I[s].depth, I[s].depth_step = d_in[s].value, cols * 4
                sen = (C.c_int * S)(*range(S))
                outs = (C.c_void_p * S)(*[p.value for p in d_out])
                g = pose_to_cm(pose)
                p = t.params(m)
                st, sums = _lib.DepthTrainStats(), _lib.DepthEvalSums()
                und, cpy, cl_set, cl_plain, ev, host, up = [], [], [], [], [], [], []
                train = []
                for rnd in range(a.rounds + 1):          # (the first round is the warm-up)
                    keep = rnd > 0
                    for _ in range(a.reps):
                        assert L.rgbd360_depth_undistort(ctx, models._handle(), I, sen, S, 1, rows, cols, 1, outs, cols * 4) == 0
                        keep and und.append(last_us())
                        us = C.c_float()
                        assert L.rgbd360_depth_apply_time_copy(ctx, d_all_out, d_all_in, S * n * 4, C.byref(us)) == 0
                        keep and cpy.append(us.value)
                        assert L.rgbd360_rig_depth_clouds(ctx, models._handle(), I, 1, S, 1, rows, cols, *fpin, 1, d_cloud) == 0
                        keep and cl_set.append(last_us())
                        assert L.rgbd360_rig_depth_clouds(ctx, None, I, 1, S, 1, rows, cols, *fpin, 1, d_cloud) == 0
                        keep and cl_plain.append(last_us())
                        assert L.rgbd360_depth_evaluate_map(ctx, m._handle(), models._handle(), 0, d_meas, cols * 4, 1, rows, cols, *fpin, _ptr(g), 1, C.byref(p),
                                                            C.byref(st), C.byref(sums)) == 0
                        keep and ev.append(last_us())
                    tr, ca = np.zeros(3 * a.reps, F), np.zeros(a.reps, F)
                    assert L.rgbd360_depth_trainer_time_map(t._handle(), m._handle(), d_meas, cols * 4, 1, *fpin, _ptr(g), C.byref(p), d_o, d_d, a.reps, _ptr(tr),
                                                            _ptr(ca), None) == 0
                    keep and train.append(tr.reshape(3, a.reps)[2])
                    if keep:                             # the host route, once per round
                        t0 = time.perf_counter()
                        fixed = [hm.undistort(img) for hm, img in zip(host_models, images)]
                        t1 = time.perf_counter()
                        for buf, f in zip(d_out, fixed):
                            assert hip.hipMemcpy(buf, _ptr(f), f.nbytes, 1) == 0
                        t2 = time.perf_counter()
                        host.append((t1 - t0) * 1e6)
                        up.append((t2 - t1) * 1e6)
                train = np.concatenate(train)
                u, c = np.median(und), np.median(cpy)
                say("%d x %dx%d float32 metres (%d pixels, blob %d KiB):" % (S, cols, rows, S * n, models.nbytes >> 10))
                say("  (a) k_depth_undistort, one launch      %s | device-to-device copy of the same bytes %s | undistort / copy %.2f x" % (med(und), med(cpy), u / c))
                say("      host route: %d x rgbd360_depth_model_undistort %s + upload %s | host route / device kernel %.0f x"
                    % (S, med(host), med(up), (np.median(host) + np.median(up)) / u))
                say("  (b) k_rig_cloud_models (with the set)   %s | k_rig_pinhole_cloud (set NULL) %s | with / without %.2f x"
                    % (med(cl_set), med(cl_plain), np.median(cl_set) / np.median(cl_plain)))
                say("  (c) k_depth_eval, one %dx%d image        %s | k_depth_train (form 2) %s | evaluate / train %.2f x | %d examples"
                    % (cols, rows, med(ev), med(train), np.median(ev) / np.median(train), sums.n))
                for ptr in (d_all_in, d_all_out, d_cloud, d_meas, d_o, d_d):
                    hip.hipFree(ptr)
            for hm in host_models:
                hm.close()
    reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
