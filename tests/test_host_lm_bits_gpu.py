"""The bytes of the two host-driven Levenberg-Marquardt alignments (rgbd360_align_pinhole, rgbd360_rig_align: one driver, csrc/lm_host.h)
against the fixture recorded on an MI355X while each entry still had a loop of its own (tests/golden/host_lm_bits.json,
tools/host_lm_bits.py): per case the status, the iterations per level, the reported residuals, pose and normal equations of the alignment
and the evaluation entry's whole out-parameter block at the guess on every level, byte for byte.  The oracle tests bound the poses to
1e-4; this one holds every accept / reject / retry decision, the damping sequence and the float32 / float64 unpacking of the sums still."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorder():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import host_lm_bits
    return host_lm_bits


@pytest.fixture(scope="module")
def recorded(recorder):
    with open(recorder.OUT) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def computed(hip_lib, recorder):
    return recorder.compute()


def test_every_case_equals_the_fixture_byte_for_byte(recorded, computed):
    # 9 pinhole cases (2 of seed 72, 5 of seed 77, 2 ILL-POSED) and 6 rig cases
    assert len(recorded) == 15 and sorted(recorded) == sorted(computed)
    differ = []
    for case in sorted(recorded):
        want, got = recorded[case], computed[case]
        for field in sorted(set(want["align"]) | set(got["align"])):
            if want["align"].get(field) != got["align"].get(field):
                differ.append("%s align.%s: recorded %s, computed %s" % (case, field, want["align"].get(field), got["align"].get(field)))
        assert len(want["eval"]) == len(got["eval"]), case
        for level, (w, g) in enumerate(zip(want["eval"], got["eval"])):
            for field in sorted(set(w) | set(g)):
                if w.get(field) != g.get(field):
                    differ.append("%s eval[%d].%s: recorded %s, computed %s" % (case, level, field, w.get(field), g.get(field)))
    assert not differ, "\n".join(differ)


def test_the_cases_are_not_trivial(recorded):
    """From the recorded values: every exit status occurs, one level runs into the maxIters cap, one takes no step, and the two pinhole
    pairs end at different poses."""
    align = {case: rec["align"] for case, rec in recorded.items()}
    assert {a["status"] for a in align.values()} == {0, 1, 2}
    iters = [n for a in align.values() for n in a["iters"]]
    assert 10 in iters and 0 in iters
    assert align["pin72/guess"]["iters"] == [6, 8, 10] and align["pin77/m2/occ1"]["iters"] == [1, 3, 3]      # the oracle's sequences
    assert align["pin72/identity"]["pose"] != align["pin77/m2/occ0"]["pose"] and align["pin72/guess"]["pose"] != align["pin77/m2/occ0"]["pose"]
    for case in ("pinflat/m1", "pinflat/m2"):      # the pinhole ILL-POSED exit: the guess comes back, err_final 0, no `iters` entry written
        assert align[case]["status"] == 1 and align[case]["iters"] == [0, 0] and align[case]["err_final"] == "00" * 8
    assert align["rig/flat"]["status"] == 1 and align["rig/blank"]["status"] == 0 and align["rig/blank"]["iters"] == [0, 0, 0]
