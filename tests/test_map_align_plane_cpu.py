"""CPU tests of the point-to-plane alignment against the voxel map: the plane function of the restatement
(tests/map_align_plane_reference.py) against numpy.linalg.eigh and, bit for bit, against the library's host compile of the function the
kernel calls; the restatement on an analytic room corner, where point-to-plane must come closer to the true pose than point-to-point;
and the agreement of the header, the ctypes binding and the C++ adapter."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_align_plane_reference as PL
import map_align_reference as A
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
MAX_FLATNESS = 0.05
# Largest angle between the restatement's normal and eigh's eigenvector over the supports below whose verdict is planar and whose
# eigh ratio l0 / l1 is a factor 2 inside the gate: MEASURED_ANGLE (radians, 4000 supports, seed 11); the test asserts 10 x that.
MEASURED_ANGLE = 2.75e-12
# Pose errors (rotation in radians, translation in metres) of the two restatements on the corner scene, seeds 1, 2, 3, measured:
#   point-to-point  (1.84e-3, 4.51e-3)  (2.15e-3, 5.67e-3)  (2.31e-3, 6.11e-3)      converged after 7 / 8 / 9 steps
#   point-to-plane  (7.68e-4, 1.97e-3)  (6.58e-4, 1.97e-3)  (7.85e-4, 2.52e-3)      10 steps, the iteration limit
# The test asserts plane <= point per seed and plane below 4 x the largest measured value.
CORNER_SEEDS = (1, 2, 3)
MEASURED_PLANE_ERR = (7.85e-4, 2.52e-3)


def random_rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def supports(kind, count, rng):
    """`count` supports of 5-27 points at the scale of a 5 cm lattice's centroids around a point, as covariance upper triangles."""
    out = []
    for _ in range(count):
        m = int(rng.integers(5, 28))
        if kind == "plane":          # a wall, centroids within about 1 mm of it
            p = np.c_[rng.uniform(-0.075, 0.075, (m, 2)), rng.normal(0, 0.001, m)]
        elif kind == "line":         # an edge seen alone: thin in two directions
            p = np.c_[rng.uniform(-0.075, 0.075, m), rng.normal(0, 0.001, (m, 2))]
        elif kind == "corner":       # two walls at a right angle
            p = np.c_[rng.uniform(-0.075, 0.075, (m, 2)), rng.normal(0, 0.001, m)]
            up = rng.random(m) < 0.5
            p[up] = p[up][:, [0, 2, 1]]
            p[up, 2] = np.abs(p[up, 2])
        else:                        # a blob
            p = rng.uniform(-0.075, 0.075, (m, 3))
        p = p @ random_rotation(rng).T + rng.uniform(-0.025, 0.025, 3)
        mean = p.mean(axis=0)
        c = (p[:, :, None] * p[:, None, :]).mean(axis=0) - mean[:, None] * mean[None, :]
        out.append([c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]])
    return np.array(out)


@pytest.fixture(scope="module")
def support_set():
    rng = np.random.default_rng(11)
    return {kind: supports(kind, 1000, rng) for kind in ("plane", "line", "corner", "blob")}


def full(c):
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])


def test_plane_function_against_eigh(support_set):
    worst, planar_seen, rejected_seen = 0.0, 0, 0
    for kind, cov in support_set.items():
        n, planar, l0, l1 = PL.plane_fit(cov, MAX_FLATNESS)
        verdicts = 0
        for k in range(len(cov)):
            ev, vec = np.linalg.eigh(full(cov[k]))
            ratio = ev[0] / ev[1]
            if ratio <= 0.5 * MAX_FLATNESS:
                assert planar[k], (kind, k, ratio)
                angle = np.arcsin(min(1.0, np.linalg.norm(np.cross(n[k], vec[:, 0]))))
                worst = max(worst, angle)
                assert abs(np.linalg.norm(n[k]) - 1.0) < 1e-15
                assert abs(l0[k] - ev[0]) <= 1e-12 * ev[2] and abs(l1[k] - ev[1]) <= 1e-12 * ev[2]
                planar_seen += 1
                verdicts += 1
            elif ratio >= 2.0 * MAX_FLATNESS:
                assert not planar[k], (kind, k, ratio)
                rejected_seen += 1
                verdicts += 1
        print(kind, "supports", len(cov), "with a verdict", verdicts, "planar", int(planar.sum()))
        assert verdicts > 0.8 * len(cov)
        assert (planar.sum() > 0.9 * len(cov)) if kind == "plane" else (planar.sum() < 0.1 * len(cov))
    print("largest angle to eigh's eigenvector", worst)
    assert planar_seen > 900 and rejected_seen > 2500
    assert worst <= 10 * MEASURED_ANGLE


def test_plane_function_special_supports():
    # a single candidate, or all in one place: C = 0, no cross product, not planar
    n, planar, l0, l1 = PL.plane_fit(np.zeros((1, 6)), MAX_FLATNESS)
    assert not planar[0] and (n == 0).all()
    # an exact plane z = 0: l0 = 0, the normal is the z axis, planar even with max_flatness = 0
    n, planar, l0, l1 = PL.plane_fit(np.array([[2.0, 0.5, 0, 1.0, 0, 0]]), 0.0)
    assert planar[0] and l0[0] == 0.0 and abs(n[0, 2]) == 1.0 and n[0, 0] == 0.0 and n[0, 1] == 0.0
    # an exact line: l0 = l1 = 0 -> l1 > 0 fails
    n, planar, l0, l1 = PL.plane_fit(np.array([[1.0, 0, 0, 0, 0, 0]]), 1.0)
    assert not planar[0]
    # the sphere: a triple root, which Newton's method approaches by a third per step (12 steps from 0: 1 - (2/3)^12); the gate rejects it
    n, planar, l0, l1 = PL.plane_fit(np.array([[1.0, 0, 0, 1.0, 0, 1.0]]), MAX_FLATNESS)
    assert not planar[0] and 0.99 < l0[0] < 1.0 and abs(l1[0] - 1.0) < 0.01


def test_the_library_function_is_the_restatement_bit_for_bit(support_set):
    """rgbd360_map_plane_fit is the host compile of the function the point-to-plane evaluation (PlaneTail) calls: + - x / sqrt in float64 without contraction
    give the same bits as numpy's, verdict, normal and both eigenvalues."""
    from rgbd360_amd import build
    L = C.CDLL(build.build())
    L.rgbd360_map_plane_fit.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    for mf in (MAX_FLATNESS, 0.0, 0.3):
        for kind, cov in support_set.items():
            n, planar, l0, l1 = PL.plane_fit(cov, mf)
            for k in range(0, len(cov), 4):
                c, out, eig = np.ascontiguousarray(cov[k]), np.zeros(3), np.zeros(2)
                rc = L.rgbd360_map_plane_fit(c.ctypes.data, float(np.float32(mf)), out.ctypes.data, eig.ctypes.data)
                assert rc == int(planar[k]), (kind, k)
                assert out.tobytes() == n[k].tobytes() and eig[0].tobytes() == l0[k].tobytes() and eig[1].tobytes() == l1[k].tobytes(), (kind, k)
    assert L.rgbd360_map_plane_fit(None, 0.05, None, None) == -1


@pytest.fixture(scope="module")
def corner():
    """Both restatements on the room corner, per seed: a map of one sampling at the identity, another sampling seen from P as source."""
    P = R.general_pose()
    out = {}
    for seed in CORNER_SEEDS:
        tgt = R.Map([(PL.corner_scene(100 + seed), None, EYE)], 0.05, None)
        src = PL.corner_scene(200 + seed, P)
        guess = A.perturbed(P, 0.02, np.radians(0.5), seed)
        out[seed] = dict(P=P, guess=guess, point=A.Alignment(tgt, src, guess, 0.05, None, 0.05), plane=PL.PlaneAlignment(tgt, src, guess, 0.05, None, 0.05))
    return out


@pytest.mark.parametrize("seed", CORNER_SEEDS)
def test_point_to_plane_is_closer_on_the_room_corner(corner, seed):
    c = corner[seed]
    point, plane = c["point"], c["plane"]
    (rp, tp), (rl, tl) = A.pose_error(point.pose, c["P"]), A.pose_error(plane.pose, c["P"])
    print("seed", seed, "guess", A.pose_error(c["guess"], c["P"]), "point-to-point", (rp, tp), point.iterations, "point-to-plane", (rl, tl), plane.iterations,
          "contributing", plane.n_matched, plane.final.counters, "fitness", plane.fitness, "fitness_point", plane.fitness_point, point.fitness)
    assert point.status == A.OK and plane.status == A.OK
    assert rl <= rp and tl <= tp
    assert rl <= 4 * MEASURED_PLANE_ERR[0] and tl <= 4 * MEASURED_PLANE_ERR[1]
    # the three edges: supports that straddle two walls are rejected
    assert plane.final.counters["n_nonplanar"] > 0 and plane.n_matched > 100000
    near_edge = plane.final.cls == PL.NONPLANAR
    src_world = R.transform(PL.corner_scene(200 + seed, c["P"]), plane.pose)
    assert (np.sort(np.abs(src_world[near_edge]), axis=1)[:, 1] < 0.11).all()       # within two cells of an edge: two coordinates are small
    # the plane distance is far below the distance to the centroid of the same matches
    assert plane.fitness < 0.1 * plane.fitness_point


def test_a_single_wall_is_ill_posed():
    wall = PL.corner_scene(5)[:40000:4]          # the plane x = 0 alone
    assert (wall[:, 0] == 0).all()
    tgt = R.Map([(wall, None, EYE)], 0.05, None)
    guess = EYE.copy()
    guess[0, 3] = 0.01
    al = PL.PlaneAlignment(tgt, wall, guess, 0.05, None, 0.05)
    assert al.status == A.ILL_POSED and al.iterations == 0 and al.n_matched > 5000 and al.pose.tobytes() == guess.tobytes()


def test_header_binding_and_adapter_agree():
    from rgbd360_amd import _lib, build
    L = C.CDLL(build.build())
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    for name in ("rgbd360_map_default_align_plane_params", "rgbd360_map_align_plane_sphere", "rgbd360_map_align_plane_cloud"):
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS
    for name in ("rgbd360_map_align_plane_eval", "rgbd360_map_plane_fit", "rgbd360_map_time_align_plane"):
        assert re.search(r"\b%s\s*\(" % name, diag) and name not in main and hasattr(L, name) and name in _lib.SYMBOLS

    def fields(text, struct):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, text).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
        return names

    for struct, cls, size in (("rgbd360_map_align_plane_params", _lib.MapAlignPlaneParams, 32), ("rgbd360_map_align_plane_result", _lib.MapAlignPlaneResult, 248)):
        assert fields(main, struct) == [n for n, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    # the existing structs keep their sizes, and the new ones begin with them
    assert C.sizeof(_lib.MapAlignParams) == 24 and C.sizeof(_lib.MapAlignResult) == 224
    assert fields(main, "rgbd360_map_align_plane_params")[:5] == fields(main, "rgbd360_map_align_params")
    assert fields(main, "rgbd360_map_align_plane_result")[:10] == fields(main, "rgbd360_map_align_result")
    L.rgbd360_map_default_align_plane_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapAlignPlaneParams)]
    L.rgbd360_map_default_align_plane_params.restype = None
    p = _lib.MapAlignPlaneParams()
    L.rgbd360_map_default_align_plane_params(None, C.byref(p))
    assert (p.max_iters, p.min_count, p.min_matches, p.min_support) == (10, 1, 6, 5)
    assert p.eps == np.float32(1e-6) and p.max_dist == np.float32(0.05) and p.max_flatness == np.float32(0.05)
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("alignSpherePlane", "alignCloudPlane", "alignPlaneParams", "alignPlaneResult", "rgbd360_map_align_plane_sphere", "rgbd360_map_align_plane_cloud",
                 "rgbd360_map_default_align_plane_params"):
        assert name in hpp, name
    py = open(os.path.join(ROOT, "rgbd360_amd", "voxel_map.py")).read()
    assert "def align_sphere_plane" in py and "def align_cloud_plane" in py
    assert "--refine-on-map-plane" in open(os.path.join(ROOT, "examples", "odometry_replay.cpp")).read()
