"""Many alignments against the voxel map in lock step (rgbd360_map_align_batch_*, csrc/map_align_batch.h), the parts that need no GPU:
the winner rule (rgbd360_map_align_best / _plane_best) on hand-made results, the declarations and exports, the example, and the
multi-start scenario in the numpy restatement alone (map_align_reference, map_align_plane_reference, voxel_map_reference) -- the
scenario tests/test_map_align_batch_gpu.py runs end to end on the device, with the values measured here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_align_plane_reference as PL
import map_align_reference as A
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)

# The scenario: the three-wall corner sampled every 2 cm is the map at leaf 0.1 (no box), the same corner sampled every 4 cm and seen from
# the general pose is the cloud (7 500 points), the centre guess is the truth moved by OFFSET, the lattice 3 x 3 x 3 guesses SPACING apart
# around it (job 13 is the centre).  Measured with the restatement (this file, test_multi_start_in_the_restatement prints them):
#   point-to-point  centre: OK, 438 matches, 0.324 m off; winner job 6 with 7500 matches, runner-up 4972; winner 4.862 mm from the truth
#   point-to-plane  centre: ILL_POSED at step 0, 0.330 m off; winner job 3 with 6718 matches, runner-up 6540 (a lead of 2.6 %); 8.482 mm
LEAF, OFFSET, SPACING = 0.1, (0.21, -0.17, 0.19), 0.2
MEASURED_WINNER = {"point": 6, "plane": 3}
MEASURED_WINNER_ERR = {"point": 4.862e-3, "plane": 8.482e-3}      # metres; the bound is 1.5 x (device and restatement agree to 5e-6)
MIN_MATCHED = 6


def moved(T, d):
    T = np.array(T, np.float32).copy()
    T[:3, 3] += np.asarray(d, np.float32)
    return T


def scenario():
    """(truth, map cloud, source cloud, the 27 guesses): shared with the GPU test, which repeats it."""
    P = R.general_pose()
    centre = moved(P, OFFSET)
    guesses = [moved(centre, (SPACING * i, SPACING * j, SPACING * k)) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    return P, PL.corner_scene(101, step=0.02), PL.corner_scene(201, P, step=0.04), guesses


def ranked(rows, min_matched):
    """The winner rule restated: indices of the eligible (status, n_matched, fitness) rows, best first."""
    ok = [k for k, r in enumerate(rows) if r[0] == A.OK and r[1] >= min_matched]
    return sorted(ok, key=lambda k: (-rows[k][1], rows[k][2], k))


@pytest.fixture(scope="module")
def lib():
    from rgbd360_amd import _lib, build
    L = C.CDLL(build.build())
    for name, rt in (("rgbd360_map_align_best", _lib.MapAlignResult), ("rgbd360_map_align_plane_best", _lib.MapAlignPlaneResult)):
        getattr(L, name).argtypes = [C.POINTER(rt), C.c_int, C.c_longlong]
        getattr(L, name).restype = C.c_int
    return L


def best(lib, plane, rows, min_matched=0, n=None):
    from rgbd360_amd import _lib
    res = ((_lib.MapAlignPlaneResult if plane else _lib.MapAlignResult) * max(len(rows), 1))()
    for k, (status, n_matched, fitness) in enumerate(rows):
        res[k].status, res[k].n_matched, res[k].fitness = status, n_matched, fitness
    return (lib.rgbd360_map_align_plane_best if plane else lib.rgbd360_map_align_best)(res, len(rows) if n is None else n, min_matched)


@pytest.mark.parametrize("plane", (False, True))
def test_best_on_hand_made_results(lib, plane):
    OK, ILL, NONE = A.OK, A.ILL_POSED, A.NO_VALID_PIXELS
    assert best(lib, plane, [(OK, 10, 1.0), (OK, 30, 5.0), (OK, 20, 0.1)]) == 1                  # by matches, whatever the fitness
    assert best(lib, plane, [(OK, 30, 2.0), (OK, 30, 1.0), (OK, 30, 1.5)]) == 1                  # the fitness tie-break
    assert best(lib, plane, [(OK, 5, 1.0), (OK, 30, 1.0), (OK, 30, 1.0), (OK, 30, 1.0)]) == 1    # the index tie-break
    assert best(lib, plane, [(OK, 10, 1.0), (OK, 30, 5.0), (OK, 20, 0.1)], min_matched=31) == -1
    assert best(lib, plane, [(OK, 10, 1.0), (OK, 30, 5.0), (OK, 20, 0.1)], min_matched=30) == 1
    assert best(lib, plane, [(OK, 10, 1.0), (OK, 19, 5.0), (OK, 20, 0.1)], min_matched=20) == 2
    assert best(lib, plane, [(ILL, 90, 0.0), (OK, 10, 1.0), (NONE, 80, 0.0)]) == 1               # a non-OK status is skipped
    assert best(lib, plane, [(ILL, 90, 0.0), (NONE, 80, 0.0)]) == -1                             # none eligible
    assert best(lib, plane, [(OK, 10, 1.0)], n=0) == -1 and best(lib, plane, [(OK, 10, 1.0)], n=-3) == -1
    assert (lib.rgbd360_map_align_plane_best if plane else lib.rgbd360_map_align_best)(None, 4, 0) == -1
    # the restated rule of this file agrees on a mixed list
    rows = [(OK, 30, 2.0), (ILL, 99, 0.0), (OK, 30, 1.0), (OK, 7, 0.0), (OK, 30, 1.0)]
    assert best(lib, plane, rows, 8) == ranked(rows, 8)[0] == 2


NEW_SYMBOLS = ("rgbd360_map_align_batch_cloud", "rgbd360_map_align_batch_sphere", "rgbd360_map_align_plane_batch_cloud",
               "rgbd360_map_align_plane_batch_sphere", "rgbd360_map_align_best", "rgbd360_map_align_plane_best", "rgbd360_map_align_batch_trace")


def test_declared_exported_and_mirrored(lib):
    from rgbd360_amd import _lib
    from rgbd360_amd.voxel_map import VoxelMap
    pub = open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
        assert name + "(" in (diag if name.endswith("_trace") else pub), name
    for text in ("RGBD360_MAP_BATCH_MAX ", "RGBD360_MAP_BATCH_MAX_ROWS", "RGBD360_MAP_BATCH_MAX_UPLOAD", "rgbd360_map_batch_cloud;", "rgbd360_map_batch_frame;",
                 "rgbd360_map_batch_job;"):
        assert text in pub, text
    assert _lib.MAP_BATCH_MAX == 1024 and "#define RGBD360_MAP_BATCH_MAX        1024" in pub
    assert C.sizeof(_lib.MapBatchJob) == 68 and C.sizeof(_lib.MapBatchCloud) == 16 and C.sizeof(_lib.MapBatchFrame) == 16
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("alignBatchCloud", "alignBatchSphere", "alignBatchCloudPlane", "alignBatchSpherePlane", "batchTrace", "bestJob"):
        assert name + "(" in hpp, name
    for name in ("align_batch_cloud", "align_batch_sphere", "align_batch_trace", "best_job"):
        assert callable(getattr(VoxelMap, name)), name


def test_the_example_compiles_with_wall(tmp_path):
    from rgbd360_amd import build
    lib_path = build.build()
    exe = tmp_path / "map_multistart"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "map_multistart.cpp"), "-L" + os.path.dirname(lib_path), "-lrgbd360_hip",
                           "-Wl,-rpath," + os.path.dirname(lib_path), "-o", str(exe)])
    assert exe.exists()


def test_multi_start_in_the_restatement():
    """The centre guess alone fails; the lattice has a clear winner by the rule of rgbd360_map_align_best, and it is at the truth."""
    P, map_cloud, src, guesses = scenario()
    assert len(src) == 7500 and len(guesses) == 27
    tgt = R.Map([(map_cloud, None, EYE)], LEAF, None)
    for method, cls in (("point", A.Alignment), ("plane", PL.PlaneAlignment)):
        runs = [cls(tgt, src, g, LEAF, None, LEAF) for g in guesses]
        rows = [(r.status, r.n_matched, r.fitness) for r in runs]
        centre = runs[13]
        centre_err = A.pose_error(centre.pose, P)[1]
        order = ranked(rows, MIN_MATCHED)
        winner, runner_up = runs[order[0]], runs[order[1]]
        err = A.pose_error(winner.pose, P)[1]
        print(method, "centre: status", centre.status, "matched", centre.n_matched, "error", centre_err, "| winner job", order[0], "matched", winner.n_matched,
              "runner-up job", order[1], "matched", runner_up.n_matched, "| winner error", err)
        assert not (centre.status == A.OK and centre_err <= 0.1)
        assert winner.n_matched - runner_up.n_matched >= 0.01 * winner.n_matched
        assert order[0] == MEASURED_WINNER[method]
        assert err <= 1.5 * MEASURED_WINNER_ERR[method]
        assert err >= MEASURED_WINNER_ERR[method] / 1.5          # (the recorded value is this run's, not a loose ceiling)
