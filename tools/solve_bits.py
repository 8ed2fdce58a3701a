"""The bits of the serial Gauss-Newton step (k_solve: solve_totals -> solve_waves -> solve_finish, csrc/photo_icp_kernels.h) on the
hand-made cases of tests/solve_cases.py, recorded as a fixture: tests/golden/solve_bits.json.

    python tools/solve_bits.py [--out tests/golden/solve_bits.json]       (RGBD360_LIB: the build of the library to record from)

The fixture in the tree was recorded on an MI355X from a build of commit 7588574 ("Fetch the fused launch's pending rows in 16-byte
loads on eight waves"), the last one in which k_solve ran a solve form of its own: wave 1's chain with lane-masked regions and a row
swap under a branch at every elimination step, wave 0's bookkeeping as a second copy.  k_solve now runs the fall-through form the
fused launches run; the recorded bits are the old form's.  tests/test_fused_solve_shape.py and tests/test_gn_solve_exact.py compare
all three routes of rgbd360_debug_solve_state with the file, bit for bit: a change of the solve that moves one bit of a candidate
pose, an update, an error or a decision fails them.  Record from the library a change is measured against, BEFORE the kernels
change.  Every case is computed twice in the process and nothing is written if the two differ.

Per case: route 0 of debug_solve_state on synth.make_pair(256, 128, seed=3), 3 levels (the state does not depend on the frames), every
key the call returns -- status, done, level_active, it, n_evals, pend_nb, iters as integers; cand, pose, update (float32) and lam,
error, new_error, diff_error (float64) as the hex of their bytes.  The cases: the 21 pivot choices, the zero pivot and the rank-3
matrices, the 11 arms of the exponential and the 6 turns of the state machine (test_fused_solve_shape.py); the pseudo-exponential's
branches, the bookkeeping cases and the rank and pivot edges (test_gn_solve_exact.py).  The large sweeps of the latter stay out: the
update is pinned by gn_reference.update_f32 and the verdicts by the oracle.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rgbd360_amd import synth                                # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP            # noqa: E402
import solve_cases as S                                      # noqa: E402

OUT = S.GOLDEN


def make_reg(cols=256, rows=128):
    (rgbA, dA), (rgbB, dB), _ = synth.make_pair(cols, rows, seed=3)
    reg = RegisterPhotoICP()
    reg.setNumPyr(3)
    reg.setTargetFrame(rgbA, dA)
    reg.setSourceFrame(rgbB, dB)
    return reg


def compute(reg, cases=None, route=0):
    """{case name: recorded form of the state} of every case on the device."""
    return {c["name"]: S.encode(reg.debug_solve_state(c["level"], c["row"], route=route, **c["kw"])) for c in (cases or S.all_cases())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    reg, cases = make_reg(), S.all_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    first, second = compute(reg, cases), compute(reg, cases)
    differ = [k for k in first if first[k] != second[k]]
    if differ:
        sys.exit("two runs in one process differ, nothing written: %s" % ", ".join(differ))
    with open(a.out, "w") as f:
        json.dump({"cases": first}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s (%d bytes); status 0 / 1 / 2: %s" % (len(first), a.out, os.path.getsize(a.out),
                                                             " / ".join(str(sum(r["status"] == s for r in first.values())) for s in (0, 1, 2))))


if __name__ == "__main__":
    main()
