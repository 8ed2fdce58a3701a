"""The host Levenberg-Marquardt driver of both host-driven alignments (csrc/lm_host.h) without a device: tools/lm_host_check.cpp, a
stand-alone program around a closed-form 6-parameter least-squares evaluator, built with AddressSanitizer and UBSan and run as it is.
Every branch of the loop is walked under both schedules: accepted trips, a rejected trip with a rejected retry, the ILL-POSED exit under
both values of the `iters` flag, a NaN error, and an evaluation that fails."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "c0e00000" * 16      # pose_out of the program before a run: -7 everywhere


@pytest.fixture(scope="module")
def scenarios(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tools/lm_host_check.cpp"
    exe = str(tmp_path_factory.mktemp("lm_host") / "lm_host_check")
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "rgbd360_amd", "csrc"), os.path.join(ROOT, "tools", "lm_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {"schedule": {}}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "schedule":
            out["schedule"][w[1]] = dict(zip(w[2::2], w[3::2]))
        elif w[0] == "scenario":
            cur = out[w[1]] = {"steps": []}
        elif w[0] in ("trip", "retry"):
            cur["steps"].append(dict(zip(["kind"] + w[1::2], [w[0]] + w[2::2])))
        else:
            assert w[0] == "end", line
            cur.update(zip(w[1::2], w[2::2]))
    return out


def _walk(sc):
    return [(s["kind"], int(s["level"]), int(s["accepted"])) for s in sc["steps"]]


def test_the_schedules_are_the_reference_literals(scenarios):
    pin, rig = scenarios["schedule"]["pinhole"], scenarios["schedule"]["rig"]
    assert float(pin["lambda0"]) == pytest.approx(0.01, rel=1e-7) and float(rig["lambda0"]) == pytest.approx(0.001, rel=1e-7)
    assert (pin["step"], pin["maxIters"], pin["LM_maxIters"]) == ("10", "10", "1") == (rig["step"], rig["maxIters"], rig["LM_maxIters"])
    assert (pin["tol_residual"], pin["tol_update"]) == ("%.17g" % 1e-4,) * 2
    assert (rig["tol_residual"], rig["tol_update"]) == ("%.17g" % 10 ** -1, "%.17g" % 10 ** -6)
    assert (pin["undamped_first"], pin["ill_posed_records_iters"]) == ("1", "0") and (rig["undamped_first"], rig["ill_posed_records_iters"]) == ("0", "1")


@pytest.mark.parametrize("path,first,lambda0", [("pinhole", "undamped", 0.01), ("rig", "damped", 0.001)])
def test_convergence_and_the_damping_sequence(scenarios, path, first, lambda0):
    sc = scenarios["converge/" + path]
    assert (sc["rc"], sc["status"], sc["iters0"], sc["iters1"], sc["any_trip"]) == ("0", "0", "0", "3", "1")
    trips = sc["steps"]
    # every trip on the coarse level, each accepted: `iters` counts them and the fine level starts below tol_residual
    assert _walk(sc) == [("trip", 1, 1)] * 3 and [int(t["it"]) for t in trips] == [0, 1, 2]
    assert sc["pose"] != SENTINEL
    # the pinhole's first candidate is the update of lm_update(H, g, -1, ...), the rig's that of lm_update(H, g, lambda, ...)
    assert all(t["first"] == first for t in trips)
    # lambda / 10 after every accept, from the schedule's start
    lam = [float(t["lambda"]) for t in trips]
    assert lam[0] == pytest.approx(lambda0, rel=1e-7)
    assert all(b == pytest.approx(a / 10, rel=1e-6) for a, b in zip(lam, lam[1:]))
    assert float(sc["final_error"]) < 1e-4


def test_both_paths_reach_the_same_pose(scenarios):
    import numpy as np
    a, b = (np.frombuffer(bytes.fromhex(scenarios["converge/" + p]["pose"]), ">u4").astype("<u4").view(np.float32) for p in ("pinhole", "rig"))
    assert np.abs(a - b).max() < 1e-5 and not np.array_equal(a, b)


@pytest.mark.parametrize("name,iters_level1,has_error", [("rank3/pinhole", 0, False), ("rank3/rig", 1, True), ("rank3/pinhole+records", 1, True),
                                                         ("rank3/rig-records", 0, False)])
def test_ill_posed_exit_under_both_values_of_the_flag(scenarios, name, iters_level1, has_error):
    """One accepted trip, then an H of rank 3: status 1, the pose reached returned, the fine level never entered; the level's `iters` entry
    (1) and its error are recorded only where the schedule says so."""
    sc = scenarios[name]
    assert (sc["rc"], sc["status"], sc["calls"]) == ("0", "1", "2") and _walk(sc) == [("trip", 1, 1)]
    assert (sc["iters0"], sc["iters1"], sc["any_trip"]) == ("0", str(iters_level1), "1")
    assert sc["pose"] != SENTINEL and sc["pose"] != scenarios["nan/pinhole"]["pose"]      # the accepted step is kept
    assert (float(sc["final_error"]) > 0) == has_error


def test_nan_error_runs_no_trip(scenarios):
    sc = scenarios["nan/pinhole"]
    assert (sc["rc"], sc["status"], sc["any_trip"], sc["calls"]) == ("0", "0", "0", "2") and sc["steps"] == []
    assert math.isnan(float(sc["final_error"]))


@pytest.mark.parametrize("path,lambda0", [("pinhole", 0.01), ("rig", 0.001)])
def test_every_candidate_worse(scenarios, path, lambda0):
    """Reject, retry with lambda * 10, reject, stop -- on both levels, the guess returned."""
    sc = scenarios["worse/" + path]
    assert (sc["rc"], sc["status"], sc["iters0"], sc["iters1"], sc["calls"]) == ("0", "0", "0", "0", "6")
    assert _walk(sc) == [("trip", 1, 0), ("retry", 1, 0), ("trip", 0, 0), ("retry", 0, 0)]
    for trip, retry in (sc["steps"][0:2], sc["steps"][2:4]):
        assert float(trip["lambda"]) == pytest.approx(lambda0, rel=1e-7) and float(retry["lambda"]) == pytest.approx(10 * lambda0, rel=1e-6)
    assert sc["pose"] == scenarios["nan/pinhole"]["pose"]      # = the guess


@pytest.mark.parametrize("path", ["pinhole", "rig"])
def test_failing_evaluation_returns_its_rc_and_leaves_the_pose(scenarios, path):
    sc = scenarios["fail/" + path]
    assert sc["rc"] == "-1703" and sc["calls"] == "2" and sc["steps"] == [] and sc["pose"] == SENTINEL
