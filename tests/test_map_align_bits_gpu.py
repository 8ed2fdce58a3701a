"""The bytes of the four alignments against the voxel map (csrc/map_align.h and the methods' headers) against the fixture recorded on an MI355X
before the evaluation kernels were last changed (tests/golden/map_align_bits.json, tools/map_align_bits.py): per case the float64 sums,
the counters, a digest of every per-point output, and the whole alignment -- pose, normal equations, fitness, every trace record -- byte
for byte.  The restatement tests bound the sums to 2e-6; this one holds the summation order and the schedule-independent bits still."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorder():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_align_bits
    return map_align_bits


@pytest.fixture(scope="module")
def computed(hip_lib, recorder):
    from rgbd360_amd.register import RegisterPhotoICP
    reg = RegisterPhotoICP(device=0)
    cases = recorder.compute(reg)
    reg.close()
    return cases


def test_every_case_equals_the_fixture_byte_for_byte(recorder, computed):
    with open(recorder.OUT) as f:
        want = json.load(f)["cases"]
    # 6 inputs x 4 methods x 2 poses, the strip and both leaves of the frame among them, and generalized ICP with source normals on the 3 clouds
    assert len(want) == 54 and sorted(want) == sorted(computed)
    assert {"frame/leaf0.05/point/map_pose", "frame/leaf0.1/plane/perturbed", "strip/leaf0.1/plane/perturbed", "ragged/leaf0.1/point/perturbed",
            "frame/leaf0.05/gicp/map_pose", "strip/leaf0.1/gicp/perturbed", "cloud/leaf0.05/gicp_normals/perturbed", "ragged/leaf0.1/gicp_normals/map_pose",
            "frame/leaf0.1/colour/perturbed", "strip/leaf0.1/colour/map_pose", "ragged/leaf0.1/colour/perturbed"} <= set(want)
    differ = []
    for case in sorted(want):
        for part in ("eval", "align"):
            for field in sorted(set(want[case][part]) | set(computed[case][part])):
                if want[case][part].get(field) != computed[case][part].get(field):
                    differ.append("%s %s.%s: recorded %s, computed %s" % (case, part, field, want[case][part].get(field), computed[case][part].get(field)))
    assert not differ, "\n".join(differ)


def test_the_cases_are_not_trivial(recorder, computed):
    """Every case matched points and took at least one step from the perturbed pose; the methods and the poses give different bytes."""
    import numpy as np
    for case, rec in computed.items():
        sums = np.frombuffer(bytes.fromhex(rec["eval"]["sums"]), np.float64)
        assert sums[0] > 100 and rec["eval"]["counters"][0] > 1000, case
        assert rec["align"]["status"] == 0 and rec["align"]["n_matched"] > 100, case
        if case.endswith("perturbed"):
            assert rec["align"]["iterations"] >= 2 and len(rec["align"]["trace"]) == rec["align"]["iterations"], case
        else:
            assert rec["eval"]["sums"] != computed[case.replace("map_pose", "perturbed")]["eval"]["sums"], case
    for case, rec in computed.items():      # step 1 of every other definition: the same key and d2 per point as point-to-point
        method = case.split("/")[2]
        if method != "point":
            other = computed[case.replace("/%s/" % method, "/point/")]["eval"]
            assert rec["eval"]["key3"] == other["key3"] and rec["eval"]["d2"] == other["d2"], case
