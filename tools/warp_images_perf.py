"""rgbd360_warp_images on the device: what the winner pass and the resolve pass cost next to the warp alone.

    python tools/warp_images_perf.py [--sizes 2048x1024,4096x2048] [--reps 50] [--out profiles/warp_images_perf.txt]

Per size (level 0, PHOTO_DEPTH, ground-truth pose of the synthetic pair) and index arithmetic (0 device definition, 1 the reference's
libm), from HIP events over `reps` back-to-back launches (rgbd360_time_warp_images): the winner pass, the resolve pass, the whole
rgbd360_warp_images_dev sequence (clear + both passes), and ONE k_warp_indices launch at the same size in the same run -- the cost
of the warp alone.  Next to them the host's wall clock for rgbd360_warp_images_dev calls (enqueue only, then one synchronise), and
the bytes each pass moves by design.  Back-to-back launches re-read a working set that the 256 MiB Infinity Cache holds at
2048 x 1024 (source records 32 MiB, target records 48 MiB) and does not hold whole at 4096 x 2048.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbd360_amd import synth                                        # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP, pose_to_cm, _ptr  # noqa: E402


def bytes_by_design(n, n_visible, n_hit):
    """Per pass: (read, written) bytes.  Winner: 16 B source record per pixel, a 4 B atomic per visible pixel (the clear before it
    writes 4 B per pixel).  Resolve, all four float planes: 4 B winner + 12 + 12 B target records per pixel, a 16 B source record per
    hit pixel; 4 x 4 B stores per pixel."""
    return dict(clear=(0, 4 * n), winner=(16 * n, 4 * n_visible), resolve=(28 * n + 16 * n_hit, 16 * n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x1024,4096x2048")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    say("rgbd360_warp_images: HIP-event averages over %d back-to-back launches, level 0, PHOTO_DEPTH, microseconds" % a.reps)
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        (rgbA, dA), (rgbB, dB), T = synth.make_pair(W, H, seed=1234)
        n = W * H
        reg = RegisterPhotoICP()
        reg.setNumPyr(1)
        reg.setTargetFrame(rgbA, dA)
        reg.setSourceFrame(rgbB, dB)
        L, ctx, p = reg._L, reg._ctx(), pose_to_cm(T)
        dev = []
        for _ in range(5):
            q = C.c_void_p()
            assert hip.hipMalloc(C.byref(q), n * 4) == 0
            dev.append(q)
        for arithmetic in (0, 1):
            reg.set_index_arithmetic(arithmetic)
            win = reg.warpImages(T, 2)["winner"]
            n_hit = int((win >= 0).sum())
            n_vis = int((reg.warp_indices(0, T)[:, 0] >= 0).sum())
            us = np.zeros(4, np.float32)
            reg._check(L.rgbd360_time_warp_images(ctx, 0, _ptr(p), 2, a.reps, _ptr(us)))
            reg.sync()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                L.rgbd360_warp_images_dev(ctx, 0, _ptr(p), 2, *dev)
            t1 = time.perf_counter()
            reg.sync()
            t2 = time.perf_counter()
            say("%dx%d arithmetic %d: winner pass %.1f  resolve pass %.1f  _dev sequence (clear + both) %.1f  |  one k_warp_indices launch %.1f"
                % (W, H, arithmetic, us[0], us[1], us[2], us[3]))
            say("    rgbd360_warp_images_dev wall clock: %.1f per call to enqueue, %.1f per call with the final synchronise spread over %d calls"
                % ((t1 - t0) / a.reps * 1e6, (t2 - t0) / a.reps * 1e6, a.reps))
            b = bytes_by_design(n, n_vis, n_hit)
            say("    %d pixels, %d visible, %d target pixels hit; bytes by design (read / written): clear %d / %d, winner pass %d / %d (atomics), "
                "resolve pass %d / %d" % (n, n_vis, n_hit, *b["clear"], *b["winner"], *b["resolve"]))
            say("    by design the winner pass moves %.1f MB -> %.0f GB/s, the resolve pass %.1f MB -> %.0f GB/s"
                % (sum(b["winner"]) / 1e6, sum(b["winner"]) / us[0] / 1e3, sum(b["resolve"]) / 1e6, sum(b["resolve"]) / us[1] / 1e3))
        for q in dev:
            hip.hipFree(q)
        reg.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
