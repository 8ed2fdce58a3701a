"""The bytes the two host-driven Levenberg-Marquardt alignments produce -- rgbd360_align_pinhole and rgbd360_rig_align, both through the
one driver of csrc/lm_host.h -- recorded as a fixture: tests/golden/host_lm_bits.json.

    python tools/host_lm_bits.py [--out tests/golden/host_lm_bits.json]       (RGBD360_LIB: the build of the library to record from)

The fixture in the tree was recorded on an MI355X from a build of commit f82c13c ("Add a device pose-graph optimiser for store edges and
map re-posing"), the last one with a loop of its own in each of the two entries.  tests/test_host_lm_bits_gpu.py recomputes every case
with compute() below and compares it with the file, byte for byte: a change of the driver, of a schedule or of the sums record that moves
one bit of a pose, of the normal equations or of a reported residual fails it.  Record from the library a change is measured against,
BEFORE the host code changes.  Every case is computed twice in the process and nothing is written if the two differ.

Inputs, all from seeds or constants (nothing large is stored).  Pinhole cases: 3 levels, setMaskSeams(False); the (level, trip, accepted)
sequences are those of the oracle (math_mode=1, reduce_mode=1), whose `iters` the device reproduced when the fixture was recorded:
  pin72/guess      synth.make_pinhole_pair(160, 120, seed=72), method 2, from rodrigues([0.3, 1, 0.2], 0.06), t = (0.08, -0.05, 0.06):
                   iters [6, 8, 10]: accepted retries on level 0, a rejected retry on level 1, the maxIters cap on level 2
  pin72/identity   the same pair from the identity: an accepted retry on the coarsest level
  pin77/m2/occ0    synth.make_pinhole_pair(320, 240, seed=77) from the identity: accepted trips, a rejected trip and a rejected retry
  pin77/m0/occ0    status 2 (photometric only: x / nValidDepthPts)
  pin77/m2/occ1    the occlusion-aware pass, iters [1, 3, 3]
  pin77/m1/occ1    status 2 (the photometric count is 0)
  pin77/m2/occ2    the sso path
  pinflat/m1, m2   60 x 80, 2 levels, grey 90 and 2000 mm everywhere, K = (70, 70, 39.5, 29.5), target = source, from t_z = 0.05:
                   the ILL-POSED exit, status 1, the guess returned, err_final 0, iters [0, 0]
Rig cases: synth.make_rig_pair(160, 120, seed=3, trans=0.04, rot_deg=1.5), 3 levels:
  rig/m0, m1, m2   from the identity: accepted trips, a rejected trip with a rejected retry
  rig/m2/libm      method 2 with rgbd360_rig_set_index_arithmetic(1)
  rig/blank        all-zero frames: no trip at all
  rig/flat         grey 60 against grey 200, method 0: status 1 with `iters` written for the level that failed
Per case:
  align    status and iters; err_final, rms_photo, rms_depth (float64), sso, pose, hessian, gradient (float32) as hex
  eval     per level, the evaluation entry (rgbd360_eval_pinhole_occ with the case's occlusion / rgbd360_rig_eval) at the guess:
           n_split, n_rows; err2_split, H, g, H64, g64 as hex
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import synth                                # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP            # noqa: E402
from rgbd360_amd.rig import RegisterDensePhotoICP            # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "host_lm_bits.json")
PIN72_GUESS = synth.make_pose(synth.rodrigues(np.array([0.3, 1.0, 0.2]), 0.06), np.array([0.08, -0.05, 0.06]))
RIG_FLAT_GUESS = synth.make_pose(synth.rodrigues(np.array([0.0, 0.0, 1.0]), 0.01), np.array([0.01, 0.0, 0.0])).astype(np.float32)


def _hex(v, dtype):
    return np.asarray(v, dtype).tobytes().hex()


def _align_record(status, res, n_pyr, pose):
    return {"status": int(status), "iters": [int(res.iters[l]) for l in range(n_pyr)], "err_final": _hex(res.err_final, np.float64),
            "rms_photo": _hex(res.rms_photo, np.float64), "rms_depth": _hex(res.rms_depth, np.float64), "sso": _hex(res.sso, np.float32),
            "pose": _hex(pose, np.float32), "hessian": _hex(list(res.hessian), np.float32), "gradient": _hex(list(res.gradient), np.float32)}


def _eval_record(e):
    return {"n_split": [int(x) for x in e["n_split"]], "n_rows": int(e["n_rows"]), "err2_split": _hex(e["err2_split"], np.float64),
            "H": _hex(e["H"], np.float32), "g": _hex(e["g"], np.float32), "H64": _hex(e["H64"], np.float64), "g64": _hex(e["g64"], np.float64)}


def pinhole_case(frames, K, n_pyr, guess, method, occlusion):
    (rgbA, dA), (rgbB, dB) = frames
    reg = RegisterPhotoICP()
    reg.setNumPyr(n_pyr)
    reg.setMaskSeams(False)
    reg.setCameraMatrix(K)
    reg.setTargetFrame(rgbA, dA)
    reg.setSourceFrame(rgbB, dB)
    ev = [_eval_record(reg.eval_pinhole(level, guess, method, occlusion)) for level in range(n_pyr)]
    status = reg.alignFrames(guess, method, occlusion)
    rec = {"align": _align_record(status, reg._res, n_pyr, reg.getOptimalPose()), "eval": ev}
    reg.close()
    return rec


def rig_case(Rt, K, f1, f2, guess, method, libm=0):
    reg = RegisterDensePhotoICP(Rt, K, n_pyr=3)
    reg.set_index_arithmetic(libm)
    reg.setTargetFrame(f1)
    reg.setSourceFrame(f2)
    ev = [_eval_record(reg.eval(level, guess, method)) for level in range(3)]
    reg.align(guess, method)
    rec = {"align": _align_record(reg.status, reg._res, 3, reg.getPose()), "eval": ev}
    reg.close()
    return rec


def inputs():
    """The rendered inputs, made once: compute() runs twice per recording and once per test session."""
    A72, B72, _, K72 = synth.make_pinhole_pair(160, 120, seed=72)
    A77, B77, _, K77 = synth.make_pinhole_pair(320, 240, seed=77)
    flat = (np.full((60, 80, 3), 90, np.uint8), np.full((60, 80), 2000, np.uint16))
    f1, f2, _, Rt, Kr = synth.make_rig_pair(160, 120, seed=3, trans=0.04, rot_deg=1.5)
    return dict(p72=((A72, B72), K72), p77=((A77, B77), K77), flat=((flat, flat), (70.0, 70.0, 39.5, 29.5)), rig=(f1, f2, Rt, Kr))


def compute(inp=None):
    """{case: {"align": ..., "eval": [per level]}} of every case on the device."""
    inp = inp or inputs()
    eye = np.eye(4)
    cases = {}
    cases["pin72/guess"] = pinhole_case(*inp["p72"], 3, PIN72_GUESS, 2, 0)
    cases["pin72/identity"] = pinhole_case(*inp["p72"], 3, eye, 2, 0)
    for method, occ in ((2, 0), (0, 0), (2, 1), (1, 1), (2, 2)):
        cases["pin77/m%d/occ%d" % (method, occ)] = pinhole_case(*inp["p77"], 3, eye, method, occ)
    ahead = np.eye(4)
    ahead[2, 3] = 0.05
    for method in (1, 2):
        cases["pinflat/m%d" % method] = pinhole_case(*inp["flat"], 2, ahead, method, 0)
    f1, f2, Rt, K = inp["rig"]
    for method in (0, 1, 2):
        cases["rig/m%d" % method] = rig_case(Rt, K, f1, f2, eye, method)
    cases["rig/m2/libm"] = rig_case(Rt, K, f1, f2, eye, 2, libm=1)
    blank = [(np.zeros_like(a), np.zeros_like(d)) for a, d in f1]
    cases["rig/blank"] = rig_case(Rt, K, blank, blank, eye, 2)
    cases["rig/flat"] = rig_case(Rt, K, [(np.full_like(a, 60), d) for a, d in f1], [(np.full_like(a, 200), d) for a, d in f1], RIG_FLAT_GUESS, 0)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    inp = inputs()
    first, second = compute(inp), compute(inp)
    differ = [k for k in first if first[k] != second[k]]
    if differ:
        sys.exit("two runs in one process differ, nothing written: %s" % ", ".join(differ))
    with open(a.out, "w") as f:
        json.dump({"cases": first}, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(first):
        print("%-16s status %d iters %s" % (k, first[k]["align"]["status"], first[k]["align"]["iters"]))
    print("%d cases -> %s (%d bytes)" % (len(first), a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
