"""Wall time per call of the two host-driven alignments (csrc/lm_host.h): the seed-77 method-2 pinhole alignment of tests/test_gpu_parity.py
and the method-2 rig alignment of tests/test_rig_dense.py, both from the identity.
    python tools/host_lm_perf.py LIB [calls]       median and quartiles over `calls` calls (default 300) after 20 warm-up calls; with
                                                   calls = 1 it is the program of a kernel trace (no warm-up: one alignment each)
    python tools/ab_libs.py run ROUNDS hostlm NAME NAME ...      the same, builds alternating in one session"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import _lib
_lib.LIB_PATH = sys.argv[1]
from rgbd360_amd import synth
from rgbd360_amd.register import RegisterPhotoICP
from rgbd360_amd.rig import RegisterDensePhotoICP
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 300

(rgbA, dA), (rgbB, dB), _, K = synth.make_pinhole_pair(320, 240, seed=77)
pin = RegisterPhotoICP(); pin.setNumPyr(3); pin.setMaskSeams(False); pin.setCameraMatrix(K)
pin.setTargetFrame(rgbA, dA); pin.setSourceFrame(rgbB, dB)
f1, f2, _, Rt, Kr = synth.make_rig_pair(160, 120, seed=3, trans=0.04, rot_deg=1.5)
rig = RegisterDensePhotoICP(Rt, Kr, n_pyr=3); rig.setTargetFrame(f1); rig.setSourceFrame(f2)
out = []
for name, call, iters in (("pinhole", lambda: pin.alignFrames(np.eye(4), 2), lambda: pin.num_iterations),
                          ("rig", lambda: rig.align(np.eye(4), 2), lambda: rig.num_iterations)):
    for _ in range(20 if calls > 1 else 0):
        call()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e6)
    q = np.percentile(t, [25, 50, 75])
    out.append("%s iters %s median %.1f us (quartiles %.1f .. %.1f)" % (name, iters(), q[1], q[0], q[2]))
print("; ".join(out))
