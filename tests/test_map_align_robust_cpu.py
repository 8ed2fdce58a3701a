"""CPU tests of the robust kernels of the alignments against the voxel map (include/rgbd360_hip.h, "robust kernels of the alignments
against the map"): the host build of gn::robust_rho_w -- the one text the device compiles too -- against the numpy weights
of tests/map_align_robust_reference.py, the exact degenerations of the restatement, the trial that shows what the kernels are for, and
the declarations, exports and mirrors.  No device is needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_align_gicp_reference as GI
import map_align_plane_reference as PL
import map_align_reference as A
import map_align_robust_reference as RB
import map_colour_reference as CO
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HOST_PROGRAM = r'''
#include <cstdio>
#include "gn_math.h"
// stdin: n, then n records kind delta s (hex floats); stdout per record: rho w as hex floats
int main() {
    int n;
    if (scanf("%d", &n) != 1) return 1;
    for (int k = 0; k < n; ++k) {
        int kind;
        double delta, s, rho, w;
        if (scanf("%d %lf %lf", &kind, &delta, &s) != 3) return 1;
        gn::robust_rho_w(kind, delta, s, &rho, &w);
        printf("%a %a\n", rho, w);
    }
    return 0;
}
'''


def test_the_weight_text_equals_the_numpy_weights_bit_for_bit(tmp_path):
    """gn::robust_rho_w built for the host (g++, as tests/test_pose_graph_robust_cpu.py builds it) on a grid of s straddling delta^2, with
    s = 0, s = delta^2 exactly and denormal s: w bit-equal for every kind, rho bit-equal for Huber and Geman-McClure (the same IEEE
    operations in the same order), Cauchy's rho to 1e-14 relative (log1p of two libraries: the pose-graph test's tolerance)."""
    src = tmp_path / "robust_host.cpp"
    src.write_text(_HOST_PROGRAM)
    exe = tmp_path / "robust_host"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "rgbd360_amd", "csrc"), str(src),
                           "-o", str(exe)])
    rng = np.random.default_rng(11)
    recs = []
    for delta in (0.01, 0.02, 0.01 * 8, 0.25, 3.0):
        d2 = np.float64(delta) * np.float64(delta)
        grid = [0.0, 5e-324, 2.5e-310, 1e-300, float(d2), float(np.nextafter(d2, 0.0)), float(np.nextafter(d2, 1.0))]
        grid += [float(d2 * r) for r in (1e-6, 0.03, 0.5, 0.999, 1.001, 2.0, 17.0, 1e4)] + [float(d2 * r) for r in rng.uniform(0.2, 5.0, 40)]
        recs += [(kind, delta, s) for kind in (RB.NONE,) + RB.KINDS for s in grid]
    text = "%d\n" % len(recs) + "\n".join("%d %s %s" % (k, float(d).hex(), float(s).hex()) for k, d, s in recs) + "\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(recs)
    worst = 0.0
    for (kind, delta, s), line in zip(recs, out):
        rho, w = (float.fromhex(t) for t in line.split())
        rho_ref, w_ref = (float(v[0]) for v in RB.rho_w(kind, delta, np.array([s])))
        assert np.float64(w).tobytes() == np.float64(w_ref).tobytes(), (kind, delta, s, w, w_ref)
        if kind == RB.CAUCHY:
            err = abs(rho - rho_ref) / rho_ref if rho_ref != 0.0 else abs(rho)
            worst = max(worst, err)
            assert err <= 1e-14, (delta, s, rho, rho_ref)
        else:
            assert np.float64(rho).tobytes() == np.float64(rho_ref).tobytes(), (kind, delta, s, rho, rho_ref)
        if s == 0.0 or kind == RB.NONE or (kind == RB.HUBER and s <= np.float64(delta) * np.float64(delta)):
            assert (rho, w) == (s, 1.0)
        else:       # (w rounds to 1 for a denormal s, and for Huber an ulp above delta^2)
            assert 0.0 < w <= 1.0 and 0.0 <= rho <= s and (w < 1.0 or s < 1e-6 * delta * delta or kind == RB.HUBER)
    print("Cauchy's rho, host against numpy: largest relative difference", worst)


@pytest.fixture(scope="module")
def scene():
    """The trial's map and source with lift 0.04 m, and a coloured map and source for the two methods that need normals and colours."""
    target, cloud, P, guess, n_raised = RB.trial(0.04)
    return dict(target=target, cloud=cloud, P=P, guess=guess, n_raised=n_raised)


@pytest.fixture(scope="module")
def coloured():
    m_xyz, m_rgb, s_xyz, s_rgb = CO.sliding_scene(n_map=20000, n_source=1500)
    leaf = 0.05
    target = R.Map([(m_xyz, m_rgb, np.eye(4, dtype=np.float32))], leaf, None)
    return dict(target=target, xyz=s_xyz, rgb=s_rgb, leaf=leaf, guess=CO.sliding_guess(0.02))


def _quadratic_and_robust(method, delta, target, xyz, pose, leaf, **kw):
    quad = {RB.POINT: lambda: A.Evaluation(target, xyz, pose, leaf, None, leaf),
            RB.PLANE: lambda: PL.PlaneEvaluation(target, xyz, pose, leaf, None, leaf),
            RB.GICP: lambda: GI.GicpEvaluation(target, xyz, pose, leaf, None, leaf, kw.get("normals")),
            RB.COLOUR: lambda: CO.ColourEvaluation(target, xyz, kw.get("rgb"), pose, leaf, None, leaf)}[method]()
    return quad, RB.RobustEvaluation(method, RB.HUBER, delta, target, xyz, pose, leaf, None, leaf, **kw)


@pytest.mark.parametrize("method", [RB.POINT, RB.PLANE, RB.GICP, RB.COLOUR], ids=["point", "plane", "gicp", "colour"])
def test_huber_with_a_large_delta_is_the_quadratic_evaluation(scene, coloured, method):
    """delta above the square root of the largest cost term: w = 1.0 exactly, 1.0 t = t, rho = s -- every weighted word and sum rho equal
    the quadratic restatement's bytes, nothing is down-weighted and sum w = n.  (Point: delta > max_dist.  Generalized ICP's cost is at most
    e.e / epsilon: delta > max_dist / sqrt(1e-3).  Colour: the cost is below max_dist^2 + 1.)"""
    if method == RB.COLOUR:
        quad, rob = _quadratic_and_robust(method, 2.0, coloured["target"], coloured["xyz"], coloured["guess"], coloured["leaf"], rgb=coloured["rgb"])
    else:
        delta = {RB.POINT: 0.11, RB.PLANE: 0.11, RB.GICP: 4.0}[method]
        quad, rob = _quadratic_and_robust(method, delta, scene["target"], scene["cloud"], scene["guess"], 0.1)
    assert quad.n > 500 and rob.n == quad.n
    assert rob.s.max() < rob.delta ** 2
    assert rob.sums.tobytes() == np.asarray(quad.sums, np.float64).tobytes()
    assert rob.n_downweighted == 0 and rob.sum_w == quad.n and np.all(rob.w[rob.idx] == 1.0) and rob.w.sum() == quad.n
    assert rob.row[-2] == quad.n and rob.row[-1] == 0 and len(rob.row) == RB.WORDS[method] + 2
    # and below the largest cost term the same kind does down-weight
    tight = RB.RobustEvaluation(method, RB.HUBER, float(np.sqrt(np.median(rob.s[rob.s > 0]))), *(
        (coloured["target"], coloured["xyz"], coloured["guess"], coloured["leaf"], None, coloured["leaf"]) if method == RB.COLOUR
        else (scene["target"], scene["cloud"], scene["guess"], 0.1, None, 0.1)), **({"rgb": coloured["rgb"]} if method == RB.COLOUR else {}))
    assert 0 < tight.n_downweighted < tight.n and tight.sum_w < tight.n and tight.sums[RB.SUM_SQ[method]] < quad.sums[RB.SUM_SQ[method]]


@pytest.mark.parametrize("method", [RB.POINT, RB.PLANE], ids=["point", "plane"])
def test_huber_with_a_large_delta_is_the_quadratic_loop(scene, method):
    """... and the pose sequence: every step's update, the trace and the final pose are the quadratic loop's bytes."""
    t, x, g = scene["target"], scene["cloud"], scene["guess"]
    quad = A.Alignment(t, x, g, 0.1, None, 0.1) if method == RB.POINT else PL.PlaneAlignment(t, x, g, 0.1, None, 0.1)
    rob = RB.RobustAlignment(method, RB.HUBER, 0.11, t, x, g, 0.1, None, 0.1)
    assert quad.iterations >= 2 and (rob.status, rob.iterations, rob.converged) == (quad.status, quad.iterations, quad.converged)
    assert rob.pose.tobytes() == quad.pose.tobytes()
    for (n, ss, u), (qn, qss, qu) in zip(rob.trace, quad.trace):
        assert n == qn and ss == qss and u.tobytes() == qu.tobytes()
    assert rob.fitness == quad.fitness and rob.hessian.tobytes() == quad.hessian.tobytes() and rob.gradient.tobytes() == quad.gradient.tobytes()
    assert rob.info["n_downweighted"] == 0 and rob.info["sum_w"] == rob.info["n"] == quad.n_matched


def test_the_device_order_of_summation_is_a_reordering(scene):
    """order="device" sums the same weighted terms in the kernels' order: the same counts, the sums within the rounding of 7500 additions."""
    a = RB.RobustEvaluation(RB.PLANE, RB.CAUCHY, 0.01, scene["target"], scene["cloud"], scene["guess"], 0.1, None, 0.1)
    b = RB.RobustEvaluation(RB.PLANE, RB.CAUCHY, 0.01, scene["target"], scene["cloud"], scene["guess"], 0.1, None, 0.1, order="device")
    assert a.n == b.n and a.n_downweighted == b.n_downweighted and a.w.tobytes() == b.w.tobytes()
    scale = np.abs(a.terms).sum(axis=0)
    assert np.all(np.abs(a.sums - b.sums) <= 7500 * 2.0 ** -53 * scale)
    ones = np.ones((2085, 3))
    assert RB.device_sum(ones, np.arange(2085), 2085).tolist() == [2085.0] * 3
    assert RB.device_sum(ones[:300], np.arange(300) * 4, 1200, shape=(1, 1200)).tolist() == [300.0] * 3


def trial_errors(lift, run):
    """{kind: (angle, distance)} of the trial with `lift`; run(kind, target, cloud, guess) -> the end pose (kind NONE: quadratic)."""
    target, cloud, P, guess, n_raised = RB.trial(lift)
    assert len(cloud) == 7500 and n_raised == 619
    return {kind: A.pose_error(run(kind, target, cloud, guess), P) for kind in (RB.NONE,) + RB.KINDS}


def assert_trial(err, lift):
    """The three assertions of the trial; the restatement measured distance ratios quadratic / Geman-McClure of 6.7 and
    11.7, so "half" leaves a factor of 3."""
    print("lift %.2f m:" % lift, {RB.KIND_NAMES[k]: "%.3f mrad %.2f mm" % (1e3 * r, 1e3 * t) for k, (r, t) in err.items()})
    (rq, tq) = err[RB.NONE]
    for kind in RB.KINDS:
        assert err[kind][0] < rq and err[kind][1] < tq, RB.KIND_NAMES[kind]
    assert err[RB.GEMAN_MCCLURE][1] <= err[RB.CAUCHY][1] <= err[RB.HUBER][1]
    assert err[RB.GEMAN_MCCLURE][1] <= 0.5 * tq


@pytest.mark.parametrize("lift", [0.04, 0.06])
def test_the_trial(lift):
    """A patch of the floor (619 of 7500 source points) lifted by 4 or 6 cm still matches at leaf 0.1 m and drags the quadratic
    point-to-plane alignment 9.5 / 14.0 mm off; every robust kind with delta 0.01 m ends closer in angle and distance, in the order
    Geman-McClure <= Cauchy <= Huber, and Geman-McClure at most at half the quadratic distance."""
    def run(kind, target, cloud, guess):
        if kind == RB.NONE:
            return PL.PlaneAlignment(target, cloud, guess, 0.1, None, 0.1, max_iters=10).pose
        return RB.RobustAlignment(RB.PLANE, kind, 0.01, target, cloud, guess, 0.1, None, 0.1, max_iters=10).pose
    assert_trial(trial_errors(lift, run), lift)


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_declarations_exports_and_mirrors():
    """The header against rgbd360_amd/_lib.py against the built library's symbols; the enums equal the graph's kinds; the mirrors exist."""
    from rgbd360_amd import _lib, build
    main, diag = _code("rgbd360_hip.h"), _code("rgbd360_hip_diag.h")
    product = ("rgbd360_map_set_align_robust", "rgbd360_map_get_align_robust", "rgbd360_map_align_robust_info", "rgbd360_map_align_batch_robust_info")
    measurement = ("rgbd360_map_align_robust_eval", "rgbd360_map_time_align_robust")
    L = C.CDLL(build.build())
    for name in product + measurement:
        assert re.search(r"\b%s\s*\(" % name, main if name in product else diag), name
        assert name not in (diag if name in product else main), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    for k, name in enumerate(("NONE", "HUBER", "CAUCHY", "GEMAN_MCCLURE")):
        assert re.search(r"\bRGBD360_MAP_ROBUST_%s\s*=\s*%d\b" % (name, k), main) and re.search(r"\bRGBD360_GRAPH_ROBUST_%s\s*=\s*%d\b" % (name, k), main)
        assert getattr(_lib, "MAP_ROBUST_" + name) == k
    for k, name in enumerate(("POINT", "PLANE", "GICP", "COLOUR")):
        assert re.search(r"\bRGBD360_MAP_METHOD_%s\s*=\s*%d\b" % (name, k), main) and getattr(_lib, "MAP_METHOD_" + name) == k
    # the structs: the header's fields in the header's order, and their sizes
    for struct, cls in (("rgbd360_map_robust", _lib.MapRobust), ("rgbd360_map_robust_info", _lib.MapRobustInfo)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, main).group(1)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].replace("long ", "").split(",")]
        assert fields == [n for n, _ in cls._fields_], (struct, fields)
    assert C.sizeof(_lib.MapRobust) == 16 and C.sizeof(_lib.MapRobustInfo) == 40
    # the public parameter and result structs keep their layout
    assert (C.sizeof(_lib.MapAlignParams), C.sizeof(_lib.MapAlignResult), C.sizeof(_lib.MapAlignPlaneParams), C.sizeof(_lib.MapAlignPlaneResult)) == (24, 224, 32, 248)
    assert (C.sizeof(_lib.MapAlignGicpParams), C.sizeof(_lib.MapAlignGicpResult), C.sizeof(_lib.MapAlignColourParams), C.sizeof(_lib.MapAlignColourResult)) == (40, 256, 48, 256)
    from rgbd360_amd.voxel_map import VoxelMap
    for name in ("set_align_robust", "align_robust", "robust_info"):
        assert callable(getattr(VoxelMap, name))
    assert VoxelMap.METHODS == {"point": 0, "plane": 1, "gicp": 2, "colour": 3} and VoxelMap.ROBUST_KINDS["geman_mcclure"] == 3
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("setAlignRobust", "alignRobust", "robustInfo"):
        assert re.search(r"\b%s\(" % name, hpp), name
    assert "--map-robust" in open(os.path.join(ROOT, "examples", "odometry_replay.cpp")).read()


def test_refusals_that_need_no_device():
    """A NULL map is refused by every new entry before anything is looked at."""
    from rgbd360_amd import _lib
    L = _lib.load()
    r, info = _lib.MapRobust(_lib.MAP_ROBUST_HUBER, 0, 0.01), _lib.MapRobustInfo(7, 7, 7.0, 7.0, 7, 7)
    assert L.rgbd360_map_set_align_robust(None, 0, C.byref(r)) == -1 and L.rgbd360_map_get_align_robust(None, 0, C.byref(r)) == -1
    assert (r.kind, r.scale_with_level, r.delta) == (_lib.MAP_ROBUST_HUBER, 0, 0.01)
    assert L.rgbd360_map_align_robust_info(None, C.byref(info)) == -1 and L.rgbd360_map_align_batch_robust_info(None, 0, C.byref(info)) == -1
    assert (info.method, info.kind, info.delta_eff, info.sum_w, info.n, info.n_downweighted) == (7, 7, 7.0, 7.0, 7, 7)
    row = np.full(40, 7.0)
    assert L.rgbd360_map_align_robust_eval(None, 1, None, 0, None, 0, 0, 0, 0, 0, None, None, None, 0, None, 0, None, row.ctypes.data_as(C.c_void_p), None) == -1
    assert (row == 7.0).all()


def test_the_cpp_mirror_compiles(tmp_path):
    """GlobalMap::setAlignRobust / alignRobust / robustInfo against the header (host compiler, syntax only)."""
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "rgbd360/GlobalMap.hpp"\n'
                   "double f(rgbd360::GlobalMap& g) {\n"
                   "    g.setAlignRobust(RGBD360_MAP_METHOD_PLANE, RGBD360_MAP_ROBUST_CAUCHY, 0.01, true);\n"
                   "    const rgbd360_map_robust r = g.alignRobust(RGBD360_MAP_METHOD_PLANE);\n"
                   "    const rgbd360_map_robust_info a = g.robustInfo(), b = g.robustInfo(3);\n"
                   "    return r.delta + a.sum_w + (double)b.n_downweighted;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src)])
