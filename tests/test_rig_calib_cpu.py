"""The rig calibration against the voxel map (rgbd360_map_calibrate_rig_*, csrc/rig_calib.h), the parts that need no GPU: the host build
of the one solve text (rgbd360_rig_calib_solve_host) against the scalar restatement (tests/rig_calib_reference.py) bit for bit, the
ill-posed cases, the refusals of the solve entry, the scenario in the restatement alone, the extrinsics files, the declarations and the
example.  tests/test_rig_calib_gpu.py runs the same cases and the scenario on the device.

The scenario (rig_calib_reference.scene): a closed 2 m cube sampled every 2 cm is the map at leaf 0.1; the same cube sampled every 4 cm
(other seeds) is what K = 6 rig poses x S = 4 sensors see, 593 - 2544 points per input, 24 inputs; max_flatness 5e-4; every start is
sqrt(3) x 0.02 m and sqrt(3) x 0.01 rad off (the expected norms of N(0, 0.02) / N(0, 0.01) per axis) in seeded directions; 10 steps,
eps 0.  Measured with the restatement (test_the_scenario_in_the_restatement prints them):
  residual at the true poses        rms 2.9 mm over 27 915 points (supports bent round the cube's edges remain at this gate)
  extrinsics only (fixed_sensor -1) largest translation error of an extrinsic 35.0 mm -> 4.77 mm; condition number of the reduced matrix 21.6 - 23.4
  joint (sensor 0 fixed)            extrinsics 35.0 mm -> 2.65 mm, rig poses 58.3 mm -> 8.34 mm (a left increment turns the rig about the world's
                                    origin, 1.7 m away: its translation error starts larger than the increment's); condition number 72.5 - 76.4
  the iterates do not settle: the last steps are 8.3 mm (extrinsics only) and 14.4 mm (joint) long, the floor of the evaluation at leaf 0.1
  K = S = 1, T = I against PlaneAlignment on the same cloud after 10 steps: 1.8e-8 rad, 3.3e-16 m apart (2.3e-6 m after one step)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gn_reference as G
import map_align_plane_reference as PL
import map_align_reference as A
import rig_calib_reference as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
POSE_TOL = 5e-6          # the device / restatement pose bound of tests/test_map_align_plane_gpu.py (rad, m)
MEASURED = {0: {"E": 4.77e-3}, 1: {"E": 2.65e-3, "T": 8.34e-3}}      # metres, see above; the bound is 1.5 x
MEASURED_SINGLE_GAP = (1.8e-8, 3.3e-16)                              # rad, m: RigCalibration (K = S = 1) against PlaneAlignment


def cm(Ms):
    """[n, 4, 4] row-by-column -> the library's column-major floats."""
    return np.ascontiguousarray(np.transpose(np.asarray(Ms, F), (0, 2, 1)))


def params(refine=0, fixed=-1, lam=0.0, min_input=6, min_matches=6):
    from rgbd360_amd import _lib
    p = _lib.RigCalibParams()
    p.refine_poses, p.fixed_sensor, p.lambda_, p.min_input_matches = refine, fixed, lam, min_input
    p.plane.min_matches = min_matches
    return p


def run_solve(entry, head, rows, T, E, kw):
    """(rc, status, updates, T_new, E_new) of a solve entry (head: the arguments in front of rows)."""
    K, S = len(T), len(E)
    p = params(**kw)
    rows = np.ascontiguousarray(rows, np.float64)
    Tc, Ec = cm(T), cm(E)
    upd, Tn, En, st = np.full((K + S, 6), 7, F), np.zeros_like(Tc), np.zeros_like(Ec), C.c_int(-9)
    rc = entry(*head, rows.ctypes.data, K, S, Tc.ctypes.data, Ec.ctypes.data, C.byref(p), upd.ctypes.data, Tn.ctypes.data, En.ctypes.data, C.byref(st))
    return rc, st.value, upd, np.transpose(Tn, (0, 2, 1)), np.transpose(En, (0, 2, 1))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


@pytest.fixture(scope="module")
def lib():
    from rgbd360_amd import _lib, build
    L = C.CDLL(build.build())
    vp, i32 = C.c_void_p, C.c_int
    L.rgbd360_rig_calib_solve_host.argtypes = [vp, i32, i32, vp, vp, C.POINTER(_lib.RigCalibParams), vp, vp, vp, C.POINTER(i32)]
    L.rgbd360_rig_save_extrinsics.argtypes = [vp, i32, C.c_char_p]
    return L


CASES = ("extrinsics", "joint", "extrinsics_lambda", "joint_lambda", "extrinsics_empty_input", "joint_empty_input", "extrinsics_small_input",
         "joint_small_input", "extrinsics_empty_frame", "joint_empty_frame", "one_by_one", "sixteen", "sixteen_joint")


@pytest.mark.parametrize("name", CASES)
def test_host_solve_equals_the_restatement_bit_for_bit(lib, name):
    rows, T, E, kw = RC.solve_cases()[name]
    ref = RC.Solve(rows, T, E, **kw)
    rc, status, upd, Tn, En = run_solve(lib.rgbd360_rig_calib_solve_host, (), rows, T, E, kw)
    assert rc == 0 and status == ref.status == A.OK
    assert same_bits(upd, ref.updates) and same_bits(Tn, ref.T) and same_bits(En, ref.E)
    # what the case is about really happens
    K, S = len(T), len(E)
    if name.endswith("empty_input"):
        assert ref.used == K * S - 1
    if name.endswith("small_input"):
        assert ref.used == K * S - 4
    if name.endswith("empty_frame"):
        assert ref.skipped == 1 and same_bits(Tn[2], T[2]) and not upd[2].any()
    if kw["refine"]:
        assert not upd[K + kw["fixed"]].any() and same_bits(En[kw["fixed"]], E[kw["fixed"]])
        assert all(upd[k].any() for k in range(K) if ref.frames[k].has)
    else:
        assert not upd[:K].any() and same_bits(Tn, T)
    if "lambda" in name:
        plain = RC.Solve(rows, T, E, **dict(kw, lam=0.0))
        assert not same_bits(plain.updates, ref.updates)


@pytest.mark.parametrize("case", ("wall", "singular"))
def test_ill_posed(lib, case):
    rows, T, E, kw = RC.wall_case() if case == "wall" else RC.singular_rows()
    ref = RC.Solve(rows, T, E, **kw)
    rc, status, upd, Tn, En = run_solve(lib.rgbd360_rig_calib_solve_host, (), rows, T, E, kw)
    assert (rows[:, 0] >= 6).all()
    assert rc == 0 and status == ref.status == A.ILL_POSED
    assert same_bits(Tn, T) and same_bits(En, E) and not upd.any()


def test_a_wall_seen_from_turned_rig_poses_is_well_posed():
    """The other side of wall_case: the same wall from rig poses of different orientation constrains all six directions."""
    sc = RC.scene()
    w = PL.corner_scene(201, step=0.04)
    wall = w[(w[:, 2] == 0) & (w[:, 0] > 0.3) & (w[:, 0] < 1.7) & (w[:, 1] > 0.3) & (w[:, 1] < 1.7)]
    T, E = sc["T"][:3], sc["E"][:1]
    clouds = []
    for k in range(3):
        P = np.linalg.inv(T[k].astype(np.float64) @ E[0].astype(np.float64))
        clouds.append((wall.astype(np.float64) @ P[:3, :3].T + P[:3, 3]).astype(F))
    rows = RC.rows_of(sc["target"], clouds, T, E, RC.LEAF, RC.LEAF, **RC.plane_kw())
    assert RC.Solve(rows, T, E).status == A.OK


def test_too_few_points(lib):
    rows, T, E, kw = RC.solve_cases()["extrinsics"]
    kw = dict(kw, min_matches=int(rows[:, 0].sum()) + 1)
    rc, status, upd, Tn, En = run_solve(lib.rgbd360_rig_calib_solve_host, (), rows, T, E, kw)
    assert rc == 0 and status == RC.Solve(rows, T, E, **kw).status == A.NO_VALID_PIXELS and not upd.any()


def test_refusals_of_the_solve_entry(lib):
    rows, T, E, _ = RC.solve_cases()["extrinsics"]
    ok = dict(refine=0, fixed=-1)
    assert run_solve(lib.rgbd360_rig_calib_solve_host, (), rows, T, E, ok)[0] == 0
    for kw in (dict(refine=1, fixed=-1),         # the gauge: T_k G^-1, G E_s changes no residual
               dict(refine=0, fixed=4), dict(refine=0, fixed=-2), dict(refine=2, fixed=0), dict(ok, lam=-1.0), dict(ok, lam=float("nan")),
               dict(ok, min_input=0)):
        rc, status, upd, Tn, En = run_solve(lib.rgbd360_rig_calib_solve_host, (), rows, T, E, kw)
        assert rc == -1 and status == -9 and (upd == 7).all(), kw
    bad = T.copy()
    bad[1, 0, 3] = np.inf
    assert run_solve(lib.rgbd360_rig_calib_solve_host, (), rows, bad, E, ok)[0] == -1
    bad = E.copy()
    bad[0, 1, 1] = np.nan
    assert run_solve(lib.rgbd360_rig_calib_solve_host, (), rows, T, bad, ok)[0] == -1
    p = params()
    assert lib.rgbd360_rig_calib_solve_host(None, 1, 1, cm(T).ctypes.data, cm(E).ctypes.data, C.byref(p), None, None, None, None) == -1
    big = np.zeros((17, 4, 4), F) + np.eye(4, dtype=F)
    assert run_solve(lib.rgbd360_rig_calib_solve_host, (), np.zeros((17, 30)), T[:1], big, ok)[0] == -1


def scenario(joint):
    """The restated loop of one mode; shared with the GPU test through the module's cache."""
    key = "loop%d" % joint
    sc = RC.scene()
    if key not in sc:
        T0, E0, refine, fixed = RC.start(joint)
        sc[key] = RC.RigCalibration(sc["target"], sc["clouds"], T0, E0, RC.LEAF, RC.LEAF, max_iters=10, eps=0.0, refine=refine, fixed=fixed, **RC.plane_kw())
    return sc[key]


@pytest.mark.parametrize("joint", (0, 1))
def test_the_scenario_in_the_restatement(joint):
    sc = RC.scene()
    T0, E0, refine, fixed = RC.start(joint)
    cal = scenario(joint)
    rows = RC.rows_of(sc["target"], sc["clouds"], sc["T"], sc["E"], RC.LEAF, RC.LEAF, **RC.plane_kw())
    e0, e1 = RC.largest_translation_error(E0, sc["E"]), RC.largest_translation_error(cal.E, sc["E"])
    t0, t1 = RC.largest_translation_error(T0, sc["T"]), RC.largest_translation_error(cal.T, sc["T"])
    print("joint", joint, "points per input", min(len(c) for c in sc["clouds"]), max(len(c) for c in sc["clouds"]), "| at the truth: n", rows[:, 0].sum(), "rms",
          np.sqrt(rows[:, 28].sum() / rows[:, 0].sum()), "| extrinsics", e0, "->", e1, "| poses", t0, "->", t1, "| cond", min(cal.conds), max(cal.conds),
          "| last step", cal.trace[-1][2] ** 0.5, "| status", cal.status, "steps", cal.iterations, "converged", cal.converged)
    assert cal.status == A.OK and cal.iterations == 10 and cal.converged == 0
    assert e1 <= 1.5 * MEASURED[joint]["E"] and e1 >= MEASURED[joint]["E"] / 1.5
    assert e1 <= 0.25 * e0          # a looser result would hide a wrong Jacobian
    if joint:
        assert t1 <= 1.5 * MEASURED[joint]["T"] and t1 >= MEASURED[joint]["T"] / 1.5
        assert t1 <= 0.25 * t0
    else:
        assert np.array_equal(cal.T, T0)


def single():
    """K = S = 1 with T = I: (the cloud, the guess, PlaneAlignment, RigCalibration), ten steps each."""
    sc = RC.scene()
    if "single" not in sc:
        x = sc["clouds"][0]
        P0 = G.mat4_mul_f32(sc["T"][0], sc["E"][0])
        g = A.perturbed(P0, 0.02, 0.01, 5)
        pa = PL.PlaneAlignment(sc["target"], x, g, RC.LEAF, None, RC.LEAF, max_iters=10, eps=0.0, **RC.plane_kw())
        rc = RC.RigCalibration(sc["target"], [x], np.eye(4, dtype=F)[None], g[None], RC.LEAF, RC.LEAF, max_iters=10, eps=0.0, **RC.plane_kw())
        sc["single"] = (x, g, pa, rc)
    return sc["single"]


def test_one_frame_one_sensor_is_the_single_alignment():
    """The solves differ (float32 gn::step there, float64 Cholesky here); the iterates stay within the pose tolerance of each other."""
    x, g, pa, rc = single()
    dr, dt = A.pose_error(rc.E[0], pa.pose)
    print("K = S = 1 against PlaneAlignment:", dr, "rad", dt, "m; statuses", pa.status, rc.status, "steps", pa.iterations, rc.iterations)
    assert pa.status == rc.status == A.OK and pa.iterations == 10      # (the float64 solve reaches an update of exactly zero after 3 steps and stops)
    assert dr <= POSE_TOL and dt <= POSE_TOL
    assert dr <= 1.5 * MEASURED_SINGLE_GAP[0] and dt <= max(1.5 * MEASURED_SINGLE_GAP[1], 1e-15)


LOADER = r"""
#include <cstdio>
#include "rgbd360/Frame360.hpp"
int main(int argc, char** argv) {
    rgbd360::Calib360 a, b;
    if (argc < 3 || !a.loadExtrinsicCalibration(argv[1])) return 2;
    float flat[8 * 16];
    for (int s = 0; s < 8; ++s)
        for (int k = 0; k < 16; ++k) flat[16 * s + k] = a.Rt_[(size_t)s].m[k];
    if (rgbd360_rig_save_extrinsics(flat, 8, argv[2]) != 0) return 3;
    if (!b.loadExtrinsicCalibration(argv[2])) return 4;
    for (int s = 0; s < 8; ++s)
        for (int k = 0; k < 16; ++k)
            if (a.Rt_[(size_t)s].m[k] != b.Rt_[(size_t)s].m[k]) return 5;
    return 0;
}
"""


def test_saved_extrinsics_load_through_the_frame360_loader(lib, tmp_path):
    """Rt_0N.txt: four lines of four numbers, row by row, %.9g -- a float32 survives.  The golden files (at most three decimals) come back
    exactly, through Calib360::loadExtrinsicCalibration and through a plain text read."""
    from rgbd360_amd import build
    lib_path = build.build()
    golden = os.path.join(ROOT, "tests", "golden", "sample_pair")
    src, exe, out = tmp_path / "loader.cpp", tmp_path / "loader", tmp_path / "out"
    out.mkdir()
    src.write_text(LOADER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.dirname(lib_path),
                           "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib_path), "-o", str(exe)])
    assert subprocess.call([str(exe), golden, str(out)]) == 0
    for s in range(1, 9):
        want = np.loadtxt(os.path.join(golden, "Rt_0%d.txt" % s)).astype(F)
        text = (out / ("Rt_0%d.txt" % s)).read_text()
        assert len(text.splitlines()) == 4 and all(len(line.split()) == 4 for line in text.splitlines())
        assert np.array_equal(np.array(text.split(), np.float64).reshape(4, 4).astype(F), want)
    # awkward floats survive too, and the refusals
    rng = np.random.default_rng(3)
    M = rng.normal(size=(2, 4, 4)).astype(F)
    assert lib.rgbd360_rig_save_extrinsics(cm(M).ctypes.data, 2, str(out).encode()) == 0
    for s in range(2):
        assert np.array_equal(np.loadtxt(out / ("Rt_0%d.txt" % (s + 1))).astype(F), M[s])
    assert lib.rgbd360_rig_save_extrinsics(cm(M).ctypes.data, 2, str(out / "missing").encode()) == 1
    assert lib.rgbd360_rig_save_extrinsics(None, 2, str(out).encode()) == -1 and lib.rgbd360_rig_save_extrinsics(cm(M).ctypes.data, 17, str(out).encode()) == -1


NEW_SYMBOLS = ("rgbd360_map_default_rig_calib_params", "rgbd360_map_calibrate_rig_clouds", "rgbd360_map_calibrate_rig_depth", "rgbd360_rig_save_extrinsics",
               "rgbd360_rig_calib_solve_host", "rgbd360_rig_calib_solve_dev", "rgbd360_rig_calib_trace")


def test_declared_exported_and_mirrored(lib):
    from rgbd360_amd import _lib
    from rgbd360_amd.voxel_map import VoxelMap
    pub = open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
        assert name + "(" in (diag if "rig_calib_solve" in name or name.endswith("_trace") else pub), name
    for text in ("#define RGBD360_RIG_CALIB_MAX_SENSORS 16", "rgbd360_rig_calib_params;", "rgbd360_rig_calib_result;", "rgbd360_rig_calib_sensor;"):
        assert text in pub, text
    assert "rgbd360_rig_calib_step;" in diag
    assert _lib.RIG_CALIB_MAX_SENSORS == RC.MAX_SENSORS == 16
    assert C.sizeof(_lib.RigCalibParams) == C.sizeof(_lib.MapAlignPlaneParams) + 24 == 56
    assert C.sizeof(_lib.RigCalibResult) == 48 and C.sizeof(_lib.RigCalibSensor) == 184 and C.sizeof(_lib.RigCalibStep) == 24
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("calibrateRigClouds", "calibrateRigDepth", "rigCalibParams", "saveExtrinsics"):
        assert name + "(" in hpp, name
    for name in ("calibrate_rig_clouds", "calibrate_rig_depth", "rig_calib_params", "rig_calib_trace"):
        assert callable(getattr(VoxelMap, name)), name
    for doc, text in (("README.md", "rgbd360_map_calibrate_rig"), ("DESIGN.md", "3.29"), ("INTEGRATION.md", "loadExtrinsicCalibration")):
        assert text in open(os.path.join(ROOT, doc)).read(), doc


def test_the_example_compiles_with_wall(tmp_path):
    from rgbd360_amd import build
    lib_path = build.build()
    exe = tmp_path / "calibrate_extrinsics"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "calibrate_extrinsics.cpp"), "-L" + os.path.dirname(lib_path), "-lrgbd360_hip",
                           "-Wl,-rpath," + os.path.dirname(lib_path), "-o", str(exe)])
    assert exe.exists()
    assert subprocess.call([str(exe)], stderr=subprocess.DEVNULL) == 2
