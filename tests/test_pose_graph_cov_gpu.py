"""GPU tests of the pose-graph covariances (rgbd360_graph_marginals, rgbd360_graph_relative_covariances, csrc/pose_graph_cov.h) against the
dense inverse of tests/pose_graph_cov_reference.py on the graphs of tests/pose_graph_cases.py, at the reference optimum.  The accuracy
bound is 8 x the recorded error of the numpy restatement of the device's conjugate gradients plus 1e-13 (tests/golden/pose_graph_cov.json,
pose_graph_cov_reference.device_bound): measured against the reference, never against the device."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_cov_reference as CR
import pose_graph_robust_reference as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
IDS = [CR.case_id(n, f) for n, f in CR.CASES]


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    r.setNumPyr(3)
    yield r
    r.close()


def make(reg, c, poses=None):
    from rgbd360_amd.pose_graph import PoseGraph
    g = PoseGraph(reg)
    assert g.add_vertices(c["poses"] if poses is None else poses, fixed=c["fixed"]) == 0
    g.add_edges(c["ei"], c["ej"], c["Z"], c["Om"])
    return g


def check_blocks(tag, got, res, wants, bound, cg_tol=CR.CG_TOL):
    worst = 0.0
    for k, want in enumerate(wants):
        if want.any():
            err = CR.error(got[k], want)
            worst = max(worst, err)
            assert np.array_equal(got[k], got[k].T)
            assert 1 <= res["cg_iterations"][k] <= CR.CG_MAX_ITERS and res["cg_residual"][k] <= cg_tol
        else:      # a fixed or isolated vertex, (v, v), two fixed ends: exact zeros
            assert not got[k].any() and res["cg_iterations"][k] == 0 and res["cg_residual"][k] == 0.0
    print(tag, "worst error", worst, "bound", bound, "iterations", res["cg_iterations"].tolist(), "largest residual", res["cg_residual_max"])
    assert worst <= bound
    return worst


def check_result(g, dev, res, n):
    cost, dof, vf = CR.variance_factor(g)
    assert res["status"] == 0 and res["n_queries"] == n and res["n_not_converged"] == 0
    assert res["cost"] == dev.chi2()      # the bits rgbd360_graph_chi2 returns
    assert res["dof"] == dof and res["variance_factor"] == (res["cost"] / dof if dof > 0 else 1.0)
    assert abs(res["variance_factor"] - vf) <= 1e-9 * vf + 1e-12
    assert (res["n_fixed"], res["n_isolated"]) == (int(g.user_fixed.sum()), int(g.isolated.sum()))
    assert res["cg_iterations_max"] == res["cg_iterations"].max() and res["cg_residual_max"] == res["cg_residual"].max()


@pytest.mark.parametrize("name,form", CR.CASES, ids=IDS)
def test_covariances_match_the_dense_inverse(reg, name, form):
    g, poses, _, _, marg, rel = CR.case_dense(name, form)
    bound = CR.device_bound(name, form)
    with make(reg, cases.case(name, form), poses) as dev:
        before = dev.poses().tobytes()
        cov, res = dev.marginals(list(marg))
        check_result(g, dev, res, len(marg))
        check_blocks("%s %s marginals" % (name, form), cov, res, list(marg.values()), bound)
        cov, res = dev.relative_covariances([p[0] for p in rel], [p[1] for p in rel])
        check_result(g, dev, res, len(rel))
        check_blocks("%s %s relative" % (name, form), cov, res, list(rel.values()), bound)
        assert dev.poses().tobytes() == before


def test_robust_weights_and_disabled_edges(reg):
    g, poses, _, _, marg, rel = CR.case_dense(CR.ROBUST_CASE, "noisy")
    c, _ = RR.corrupted("n70")
    bound = CR.device_bound(CR.ROBUST_CASE, "noisy")
    with make(reg, c, poses) as dev:
        dev.set_edge_robust(0, RR.closure_kinds("n70", RR.CAUCHY), RR.DELTA)
        for e in CR.ROBUST_DISABLED:
            dev.set_edge_enabled(e, [0])
        cov, res = dev.marginals(list(marg))
        check_result(g, dev, res, len(marg))
        assert res["dof"] == 6 * 79 - 6 * 69
        check_blocks("robust marginals", cov, res, list(marg.values()), bound)
        cov, res = dev.relative_covariances([p[0] for p in rel], [p[1] for p in rel])
        check_blocks("robust relative", cov, res, list(rel.values()), bound)


def test_lock_step_is_query_by_query(reg):
    """17 queries on n300 are one more than a batch of 16: bit for bit the 17 results of 17 single-query calls, in any order, twice."""
    g, poses, _, _, _, _ = CR.case_dense("n300", "noisy")
    verts = [int(v) for v in np.linspace(1, 299, 17).astype(int)]
    assert len(set(verts)) == 17
    with make(reg, cases.case("n300", "noisy"), poses) as dev:
        cov, res = dev.marginals(verts)
        assert res["status"] == 0
        for k, v in enumerate(verts):
            one, r1 = dev.marginals([v])
            assert one[0].tobytes() == cov[k].tobytes(), v
            assert (r1["cg_iterations"][0], r1["cg_residual"][0]) == (res["cg_iterations"][k], res["cg_residual"][k])
        perm = np.random.default_rng(3).permutation(17)
        cov_p, res_p = dev.marginals([verts[k] for k in perm])
        assert cov_p.tobytes() == cov[perm].tobytes() and np.array_equal(res_p["cg_iterations"], res["cg_iterations"][perm])
        again, res2 = dev.marginals(verts)
        assert again.tobytes() == cov.tobytes() and np.array_equal(res2["cg_residual"], res["cg_residual"])
        # relative covariances: a batch with zero blocks in it, against single calls
        frm = verts[:-1] + [0, 5]
        to = verts[1:] + [7, 5]
        rel, rr = dev.relative_covariances(frm, to)
        assert rr["status"] == 0 and not rel[-1].any()
        for k in (0, 8, 15, 16):
            one, _ = dev.relative_covariances([frm[k]], [to[k]])
            assert one[0].tobytes() == rel[k].tobytes(), k


def test_covariances_keep_the_parents_bits(reg):
    """tests/golden/pose_graph_cov_bits.json was recorded with tests/golden/make_golden_pose_graph_cov_bits.py from the library before the
    optimiser and the covariance batch shared one set of conjugate-gradient kernels.  Marginals and relative covariances after optimising
    (a zero block, one workgroup and two, a full batch of 16 plus a batch of one, every column cut off at cg_max_iters = 3) and the operator
    product at lambda = 1e-3 and 0 give those bits: cov, iterations, residuals, every result field, y.  Equality only."""
    import make_golden_pose_graph_cov_bits as G
    want = json.load(open(G.OUT))
    got = G.compute(reg)
    assert sorted(got) == sorted(want) == ["apply", "cov"]
    assert sorted(got["cov"]) == sorted(want["cov"]) == sorted(c[0] for c in G.COV_CASES)
    assert sorted(got["apply"]) == sorted(want["apply"]) == sorted("%s/%s" % nf for nf in G.APPLY_CASES)
    for key in want["cov"]:
        assert sorted(got["cov"][key]) == sorted(want["cov"][key]), key
        for what, rec in want["cov"][key].items():
            for field in ("result", "cg_iterations", "cg_residual", "cov_sha256"):
                assert got["cov"][key][what][field] == rec[field], (key, what, field)
    assert want["cov"]["n300/noisy/capped"]["marginals"]["result"]["status"] == CR.NOT_CONVERGED
    for key in want["apply"]:
        assert got["apply"][key] == want["apply"][key], key


def test_covariance_calls_leave_the_optimiser_alone(reg):
    c = cases.case("n70", "noisy")
    with make(reg, c) as a, make(reg, c) as b:
        res_a = a.optimize(**cases.OPT)
        cov0, r0 = b.marginals([1, 35, 69])
        b.relative_covariances([0, 35], [69, 36])
        assert b.poses().tobytes() == c["poses"].tobytes() and b.trace() == []
        res_b = b.optimize(**cases.OPT)
        assert res_a == res_b and a.poses().tobytes() == b.poses().tobytes() and a.trace() == b.trace()
        cov1, r1 = b.marginals([1, 35, 69])
        assert r1["status"] == 0 and b.trace() == a.trace() and b.poses().tobytes() == a.poses().tobytes()
        assert r1["cost"] == b.chi2() == res_b["chi2_final"]
        assert cov1.tobytes() != cov0.tobytes()      # H is the matrix at the CURRENT poses


def raw_call(dev, verts, cov, frm=None, params=None):
    from rgbd360_amd import _lib
    res = _lib.GraphCovResult()
    v = None if verts is None else np.ascontiguousarray(verts, np.int32)
    n = 0 if v is None else len(v)
    vp = None if v is None else v.ctypes.data_as(C.c_void_p)
    cp = None if cov is None else cov.ctypes.data_as(C.c_void_p)
    pp = None if params is None else C.byref(params)
    if frm is None:
        rc = dev._L.rgbd360_graph_marginals(dev._h, n, vp, pp, cp, None, None, C.byref(res))
    else:
        f = np.ascontiguousarray(frm, np.int32)
        rc = dev._L.rgbd360_graph_relative_covariances(dev._h, n, f.ctypes.data_as(C.c_void_p), vp, pp, cp, None, None, C.byref(res))
    return rc, res, dev._L.rgbd360_graph_last_error(dev._h).decode()


def test_statuses(reg):
    from rgbd360_amd.pose_graph import ILL_POSED, NOT_CONVERGED
    from rgbd360_amd.register import Rgbd360Error
    c = dict(cases.case("n70", "noisy"))
    for k in ("ei", "ej", "Z", "Om"):      # the odometry chain alone: every edge anchors what lies behind it
        c[k] = c[k][:69]
    with make(reg, c) as dev:
        sentinel = np.full((3, 36), -7.0)
        cov = sentinel.copy()
        rc, res, msg = raw_call(dev, [5, 40, 69], cov)
        assert rc == 0 and res.status == 0 and not (cov == -7.0).any()
        dev.set_edge_enabled(10, [0])      # 10 -> 11: vertices 11 .. 69 hang on no fixed vertex
        cov = sentinel.copy()
        rc, res, msg = raw_call(dev, [5, 40, 69], cov)
        print(msg)
        assert rc == ILL_POSED and res.status == ILL_POSED and "query 1" in msg and "vertex 40" in msg
        assert np.array_equal(cov, sentinel)
        rc, res, msg = raw_call(dev, [40, 3], cov[:2], frm=[5, 5])
        assert rc == ILL_POSED and "query 0" in msg and np.array_equal(cov, sentinel)
        rc, res, msg = raw_call(dev, [5, 10], cov[:2])      # the anchored part is still served
        assert rc == 0 and not (cov[:2] == -7.0).any()
        dev.set_edge_enabled(10, [1])
    with make(reg, cases.case("n70", "noisy")) as dev:
        cov, res = dev.marginals([1, 35, 69, 0], cg_max_iters=3)
        assert res["status"] == NOT_CONVERGED == CR.NOT_CONVERGED and 0 < res["n_not_converged"] <= 3 and np.isfinite(cov).all()
        assert res["n_not_converged"] == int((res["cg_residual"] > CR.CG_TOL).sum()) and res["cg_iterations_max"] == 3
        assert "message" in res and not cov[3].any()
        with pytest.raises(Rgbd360Error, match="query 1: vertex = 70"):
            dev.marginals([0, 70])
        with pytest.raises(Rgbd360Error, match="query 0: from = -1"):
            dev.relative_covariances([-1], [3])
        with pytest.raises(Rgbd360Error, match="query 2: to = 99"):
            dev.relative_covariances([1, 2, 3], [3, 4, 99])
        for bad in (dict(cg_max_iters=0), dict(cg_max_iters=100001), dict(cg_tol=0.0), dict(cg_tol=1.0), dict(cg_tol=float("nan"))):
            with pytest.raises(Rgbd360Error):
                dev.marginals([1], **bad)
        buf = np.zeros((1, 36))
        assert raw_call(dev, [1], None)[0] == -1                      # a NULL output with n > 0
        assert dev._L.rgbd360_graph_marginals(dev._h, 1, None, None, buf.ctypes.data_as(C.c_void_p), None, None, None) == -1
        assert dev._L.rgbd360_graph_relative_covariances(dev._h, 1, None, None, None, buf.ctypes.data_as(C.c_void_p), None, None, None) == -1
        rc, res, _ = raw_call(dev, None, None)                        # n == 0
        assert rc == 0 and res.status == 0 and res.n_queries == 0
        cov, res = dev.marginals([])
        assert cov.shape == (0, 6, 6) and res["status"] == 0
        cov, res = dev.marginals([1])                                  # and the graph still answers
        assert res["status"] == 0 and cov[0].any()


CPP = r"""
#include <cstdio>
#include "rgbd360/PoseGraph.hpp"
int main() {
    rgbd360::RegisterPhotoICP align;
    rgbd360::PoseGraph graph(align);
    for (int v = 0; v < 4; ++v) {
        rgbd360::Mat4f T = rgbd360::Mat4f::Identity();
        T(0, 3) = 0.5f * v;
        T(1, 3) = 0.25f * (v % 2);
        graph.addVertex(T);
    }
    const int from[4] = {0, 1, 2, 3}, to[4] = {1, 2, 3, 0};
    for (int e = 0; e < 4; ++e) {
        rgbd360::Mat4f Z = rgbd360::Mat4f::Identity();
        Z(0, 3) = e == 3 ? -1.5f : 0.5f;
        Z(1, 3) = e == 3 ? -0.25f : (e % 2 ? -0.25f : 0.25f);
        rgbd360::Mat6f I{};
        for (int d = 0; d < 6; ++d) I.m[d * 7] = 100.f * (1 + d + e);
        graph.addEdge(from[e], to[e], Z, I);
    }
    const auto M = graph.marginals({2, 0});
    const auto C = graph.relativeCovariances({1, 3}, {3, 2});
    printf("status %d dof %lld factor %.17g\n", graph.covResult().status, graph.covResult().dof, graph.covResult().variance_factor);
    for (const auto* set : {&M, &C})
        for (const auto& B : *set) {
            for (int k = 0; k < 36; ++k) printf("%.17g ", B.m[k]);
            printf("\n");
        }
    return 0;
}
"""


def test_mirrors_agree_with_the_c_abi(reg, tmp_path):
    from rgbd360_amd import build
    from rgbd360_amd.pose_graph import PoseGraph
    lib = build.build()
    src, exe = tmp_path / "cov_mirror.cpp", str(tmp_path / "cov_mirror")
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.dirname(lib),
                           "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-pthread", "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    lines = out.stdout.splitlines()
    assert lines[0].split()[:4] == ["status", "0", "dof", "6"]
    cpp = np.array([[float(x) for x in l.split()] for l in lines[1:]])
    T = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))
    Z = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))
    Om = np.zeros((4, 6, 6), np.float32)
    for v in range(4):
        T[v, 0, 3], T[v, 1, 3] = 0.5 * v, 0.25 * (v % 2)
    for e in range(4):
        Z[e, 0, 3] = -1.5 if e == 3 else 0.5
        Z[e, 1, 3] = -0.25 if e == 3 else (-0.25 if e % 2 else 0.25)
        Om[e] = np.diag([100.0 * (1 + d + e) for d in range(6)])
    with PoseGraph(reg) as g:
        g.add_vertices(T, fixed=[0])
        g.add_edges([0, 1, 2, 3], [1, 2, 3, 0], Z, Om)
        raw = np.zeros((4, 36))
        rc, res, _ = raw_call(g, [2, 0], raw[:2])
        assert rc == 0
        rc, res, _ = raw_call(g, [3, 2], raw[2:], frm=[1, 3])
        assert rc == 0 and float(lines[0].split()[5]) == res.variance_factor
        M, _ = g.marginals([2, 0])
        Cr, _ = g.relative_covariances([1, 3], [3, 2])
        py = np.concatenate([M, Cr]).transpose(0, 2, 1).reshape(4, 36)      # back to column-major
        assert py.tobytes() == raw.tobytes()
        assert np.array_equal(cpp, raw)      # %.17g round-trips a double
        assert raw[0].any() and not raw[1].any()


def test_pose_graph_slam_example_radius_sigmas(hip_lib, tmp_path):
    """examples/pose_graph_slam.cpp with its 10th argument: 0 is byte for byte the run without it; 3 prints one `uncertainty` line per
    (earlier keyframe, new keyframe) pair and considers at least the closures of the radius rule."""
    from rgbd360_amd import build
    lib = build.build()
    exe = os.path.join(str(tmp_path), "pose_graph_slam")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "pose_graph_slam.cpp"),
                           "-L" + os.path.dirname(lib), "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-pthread", "-o", exe])
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "8", "256", "128"])
    args = [exe, str(seq), "8", "256", "128", "0.0", "10.0", "8", "0", "0"]
    plain = subprocess.run(args, capture_output=True)
    zero = subprocess.run(args + ["0"], capture_output=True)
    three = subprocess.run(args + ["3"], text=True, capture_output=True)
    print(three.stdout, three.stderr)
    assert plain.returncode == zero.returncode == three.returncode == 0
    assert plain.stdout == zero.stdout and b"uncertainty" not in plain.stdout
    lines = three.stdout.splitlines()
    unc = [l.split() for l in lines if l.startswith("uncertainty ")]
    keyframes = len([l for l in lines if l.startswith("keyframe ")])
    assert keyframes == 8 and len(unc) == sum(range(keyframes - 1))      # keyframe v considers the keyframes before its predecessor
    sig = np.array([float(u[3]) for u in unc])
    assert np.isfinite(sig).all() and (sig >= 0.0).all() and (sig > 0.0).any()

    def closures(text):
        return {tuple(l.split()[1:3]) for l in text.splitlines() if l.startswith("closure ")}
    assert closures(three.stdout) >= closures(plain.stdout.decode()) and len(closures(three.stdout)) > 0
