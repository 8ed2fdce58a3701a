"""CPU tests of the pose-graph optimiser's definition (rgbd360_graph_*): the numpy restatement against finite
differences and ground truth, its two linear solvers against each other, the host build of the gn_math.h additions against it, and the
boundary (header, binding, adapters, example)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand_tangent(rng, norm):
    x = rng.normal(size=6)
    return x * (norm / np.linalg.norm(x))


def test_log_inverts_exp():
    """se3_log(se3_exp(x)) = x for angles up to 3 rad and at every branch of both functions.  The bound is float64 rounding of the about
    10^2 operations of the two functions at magnitude <= 10, with the 1 / sin(angle) amplification of the axis at 3 rad (7) on top: 1e-12.
    Below angle^2 = 1e-8 gn::se3_exp (MRPT's CPose3D::exp, restated) drops the term w x (w x u) / 6 of the translation, at most
    angle^2 |u| / 6: there the bound is that truncation of the EXISTING exponential plus the rounding."""
    rng = np.random.default_rng(1)
    worst = worst_small = 0.0
    for angle in (0.0, 1e-9, 5e-5, 9e-5, 2e-4, 5e-4, 2e-3, 0.05, 0.09, 0.11, 0.5, 1.0, 2.0, 3.0):
        for _ in range(20):
            w = rng.normal(size=3)
            w *= angle / np.linalg.norm(w)
            x = np.concatenate([rng.uniform(-5, 5, 3), w])
            err = np.abs(R.se3_log(R.se3_exp(x)) - x).max()
            if angle * angle < 1e-8:
                worst_small = max(worst_small, err)
                assert err <= angle * angle * np.linalg.norm(x[:3]) / 6.0 + 1e-12, (angle, err)
            else:
                worst = max(worst, err)
    print("log(exp(x)) - x: max", worst, "; below angle^2 = 1e-8:", worst_small)
    assert worst <= 1e-12


def test_log_is_finite_for_every_rotation():
    rng = np.random.default_rng(2)
    for E in (np.diag([1.0, -1.0, -1.0, 1.0]), np.diag([-1.0, -1.0, 1.0, 1.0]), np.diag([-1.0, 1.0, -1.0, 1.0]), np.zeros((4, 4)), np.eye(4) * 3.0):
        assert np.isfinite(R.se3_log(E)).all()
    for _ in range(50):      # within 1e-4 of pi, where the axis comes from the symmetric part: the rotation is still recovered
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        x = np.concatenate([rng.uniform(-1, 1, 3), n * (np.pi - rng.uniform(0, 1e-5))])
        E = R.se3_exp(x)
        r = R.se3_log(E)
        assert np.isfinite(r).all() and np.abs(R.se3_exp(r) - E).max() <= 1e-6


def test_jacobian_against_central_differences():
    """A = dr/dx_i and -A = dr/dx_j against central differences with h = 1e-6 for |r| <= 0.5: truncation of the series below 3e-9 plus
    differencing error below 1e-9; the bound is 1e-7 relative."""
    rng = np.random.default_rng(3)
    h = 1e-6
    worst = 0.0
    for norm in (1e-3, 0.1, 0.3, 0.5):
        for _ in range(5):
            Ti = R.se3_exp(np.concatenate([rng.uniform(-20, 20, 3), rng.uniform(-1, 1, 3)]))
            Tj = R.se3_exp(np.concatenate([rng.uniform(-20, 20, 3), rng.uniform(-1, 1, 3)]))
            Z = R.se3_exp(_rand_tangent(rng, norm)) @ R.rigid_inv(Ti) @ Tj
            r, A = R.edge_terms(Ti, Tj, Z)
            assert abs(np.linalg.norm(r) - norm) <= 1e-9
            Ni, Nj = np.zeros((6, 6)), np.zeros((6, 6))
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                Ni[:, k] = (R.edge_terms(R.se3_exp(d) @ Ti, Tj, Z)[0] - R.edge_terms(R.se3_exp(-d) @ Ti, Tj, Z)[0]) / (2 * h)
                Nj[:, k] = (R.edge_terms(Ti, R.se3_exp(d) @ Tj, Z)[0] - R.edge_terms(Ti, R.se3_exp(-d) @ Tj, Z)[0]) / (2 * h)
            worst = max(worst, np.linalg.norm(A - Ni) / np.linalg.norm(A), np.linalg.norm(-A - Nj) / np.linalg.norm(A))
    print("A against central differences: max relative difference", worst)
    assert worst <= 1e-7


@pytest.mark.parametrize("name", cases.NAMES)
def test_reference_recovers_the_truth_of_a_consistent_graph(name):
    c = cases.case(name, "consistent")
    T, res, trace = cases.reference_optimum(name, "consistent")
    connected = ~cases.reference_graph(c).isolated      # a vertex without edges comes back as it went in: nothing says where it is
    err = np.abs(T - c["gt"])[connected].max()
    print(name, "iterations", res["iterations"], "chi2", res["chi2_initial"], "->", res["chi2_final"], "max |T - truth|", err, "bound", cases.truth_bound(c))
    assert res["status"] == 0 and res["chi2_final"] < res["chi2_initial"]
    assert err <= cases.truth_bound(c)
    fixed_or_isolated = np.flatnonzero(cases.reference_graph(c).fixed)
    assert np.array_equal(T[fixed_or_isolated], c["poses"][fixed_or_isolated].astype(np.float64))


@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_pcg_form_and_dense_form_end_at_the_same_poses(name, form):
    """The condition that makes the GPU tolerance fair: at the test settings the reference with its own block-Jacobi PCG and with the exact
    dense solve end within 1e-9 of each other."""
    Td, rd, _ = cases.reference_optimum(name, form, "dense")
    Tp, rp, tp = cases.reference_optimum(name, form, "pcg")
    diff = np.abs(Td - Tp).max()
    print(name, form, "dense iterations", rd["iterations"], "pcg iterations", rp["iterations"], "cg per solve", [t["cg_iterations"] for t in tp],
          "max |dense - pcg|", diff)
    assert rd["status"] == rp["status"] == 0
    assert diff <= 1e-9


def test_trace_of_the_reference_keeps_its_invariants():
    T, res, trace = cases.reference_optimum("n70", "noisy")
    assert res["iterations"] == len(trace)
    for a, b in zip(trace, trace[1:]):
        assert b["chi2"] == (a["chi2_trial"] if a["accepted"] else a["chi2"])
        assert np.isclose(b["lam"], max(a["lam"] / 10, 1e-9) if a["accepted"] else a["lam"] * 10, rtol=1e-15)


_HOST_PROGRAM = r'''
#include <cstdio>
#include "gn_math.h"
// stdin: n, then n records of 6 + 16 doubles (a tangent x and a rigid transform T); stdout per record: se3_exp(x) (16), se3_log(se3_exp(x))
// (6), se3_log(T) (6), se3_adjoint(T) (36), se3_jl_inv(x) (36), rigid_inv(T) (16), rigid_mul(T, se3_exp(x)) (16), as hex floats
int main() {
    int n;
    if (scanf("%d", &n) != 1) return 1;
    for (int k = 0; k < n; ++k) {
        double x[6], T[16], E[16], l[6], lt[6], Ad[36], J[36], I[16], P[16];
        for (double& v : x) if (scanf("%lf", &v) != 1) return 1;
        for (double& v : T) if (scanf("%lf", &v) != 1) return 1;
        gn::se3_exp(x, E); gn::se3_log(E, l); gn::se3_log(T, lt); gn::se3_adjoint(T, Ad); gn::se3_jl_inv(x, J); gn::rigid_inv(T, I); gn::rigid_mul(T, E, P);
        for (double v : E) printf("%a ", v);
        for (double v : l) printf("%a ", v);
        for (double v : lt) printf("%a ", v);
        for (double v : Ad) printf("%a ", v);
        for (double v : J) printf("%a ", v);
        for (double v : I) printf("%a ", v);
        for (double v : P) printf("%a ", v);
        printf("\n");
    }
    return 0;
}
'''


def test_host_build_of_the_gn_math_additions_matches_numpy(tmp_path):
    """gn_math.h is one text for host and device: its host build (g++, no device) against the numpy restatement, to 1e-12 relative to the
    magnitude of each output."""
    src = tmp_path / "pg_host.cpp"
    src.write_text(_HOST_PROGRAM)
    exe = tmp_path / "pg_host"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "rgbd360_amd", "csrc"), str(src), "-o", str(exe)])
    rng = np.random.default_rng(5)
    recs = []
    for angle in (0.0, 1e-9, 5e-5, 5e-4, 0.05, 0.3, 1.0, 2.5, 3.0):
        for _ in range(4):
            w = rng.normal(size=3)
            w *= angle / np.linalg.norm(w)
            x = np.concatenate([rng.uniform(-0.4, 0.4, 3), w])
            T = R.se3_exp(np.concatenate([rng.uniform(-100, 100, 3), rng.uniform(-1.5, 1.5, 3)]))
            recs.append((x, T))
    text = "%d\n" % len(recs) + "\n".join(" ".join(float(v).hex() for v in np.concatenate([x, T.T.reshape(-1)])) for x, T in recs) + "\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(recs)
    worst = 0.0
    for (x, T), line in zip(recs, out):
        v = np.array([float.fromhex(t) for t in line.split()])
        assert v.size == 16 + 6 + 6 + 36 + 36 + 16 + 16
        E = R.se3_exp(x)
        want = [E.T.reshape(-1), R.se3_log(E), R.se3_log(T), R.adjoint(T).T.reshape(-1), R.jl_inv(x).T.reshape(-1), R.rigid_inv(T).T.reshape(-1),
                (T @ E).T.reshape(-1)]
        o = 0
        for w_ in want:
            got = v[o:o + w_.size]
            o += w_.size
            worst = max(worst, np.abs(got - w_).max() / max(1.0, np.abs(w_).max()))
    print("host gn_math.h against numpy: max relative difference", worst)
    assert worst <= 1e-12


def _strip(txt):
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_binding_and_mirrors_name_the_graph_entries():
    from rgbd360_amd import _lib, build, pose_graph
    main = _strip(open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read())
    diag = _strip(open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read())
    L = C.CDLL(build.build())
    entries = ["create", "destroy", "last_error", "add_vertices", "add_edges", "set_poses", "set_fixed", "n_vertices", "n_edges", "clear",
               "default_params", "optimize", "get_poses", "chi2", "get_trace"]
    for e in entries:
        name = "rgbd360_graph_" + e
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS, name
    for e in ("linearize", "apply", "time_kernels"):
        name = "rgbd360_graph_" + e
        assert re.search(r"\b%s\s*\(" % name, diag) and name not in main and hasattr(L, name) and name in _lib.SYMBOLS, name

    def fields(struct):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, main).group(1)
        return [n for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(long long|double|int|float)\s+", "", decl.strip()).replace(" ", "").split(",")]
    for struct, cls in (("rgbd360_graph_params", _lib.GraphParams), ("rgbd360_graph_result", _lib.GraphResult), ("rgbd360_graph_iteration", _lib.GraphIteration)):
        assert [n.rstrip("_") for n, _ in cls._fields_] == fields(struct), struct
    # the defaults need no device; a null graph is refused by every entry before anything else is looked at
    p = _lib.GraphParams()
    L.rgbd360_graph_default_params.argtypes = [C.c_void_p]
    L.rgbd360_graph_default_params(C.byref(p))
    assert (p.max_iters, p.cg_max_iters, p.tol_update, p.lambda_init, p.lambda_max, p.cg_tol) == (10, 400, 1e-6, 1e-3, 1e30, 1e-8)
    for name in ("rgbd360_graph_optimize", "rgbd360_graph_clear", "rgbd360_graph_n_vertices", "rgbd360_graph_chi2"):
        f = getattr(L, name)
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p][:{"rgbd360_graph_clear": 1, "rgbd360_graph_n_vertices": 1}.get(name, 3)]
        assert f(*([None] * len(f.argtypes))) == -1, name
    assert "pose_graph.h" in build.UNITS["rgbd360_api.hip"]
    for m in ("add_vertices", "add_edges", "add_alignments", "optimize", "poses", "chi2", "trace"):
        assert callable(getattr(pose_graph.PoseGraph, m)), m
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "PoseGraph.hpp")).read()
    for m in ("addVertex(", "addEdge(", "optimizeGraph(", "getPoses(", "result() const"):
        assert m in hpp, m
    example = open(os.path.join(ROOT, "examples", "pose_graph_slam.cpp")).read()
    assert "optimizeGraph()" in example and "globalMap.move(" in example and "store.align(" in example


_SNIPPET = r'''
#include "rgbd360/PoseGraph.hpp"
int use(rgbd360::PoseGraph& g, const rgbd360::Mat4f& a, const rgbd360::Mat4f& z, const rgbd360::Mat6f& info) {
    const int v0 = g.addVertex(a), v1 = g.addVertex(a);
    g.addEdge(v0, v1, z, info);
    g.addEdge(v0, v1, z);
    const bool ok = g.optimizeGraph();
    std::vector<rgbd360::Mat4f> poses;
    g.getPoses(poses);
    const rgbd360_graph_result& r = g.result();
    return ok && r.status == RGBD360_OK && (int)poses.size() == g.numVertices() && g.numEdges() == 2 ? (int)g.trace().size() : -1;
}
'''


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_headers"])
def test_adapter_and_example_compile_against_the_header(tmp_path, mock):
    extra = ["-I" + os.path.join(ROOT, "tests", "mock_headers")] if mock else []
    src = tmp_path / "graph_snippet.cpp"
    src.write_text(_SNIPPET)
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + extra
    subprocess.check_call(base + [str(src)])
    subprocess.check_call(base + [os.path.join(ROOT, "examples", "pose_graph_slam.cpp")])
    c_src = tmp_path / "graph_c.c"
    c_src.write_text('#include "rgbd360_hip.h"\nint f(rgbd360_graph* g) { rgbd360_graph_params p; rgbd360_graph_result r; rgbd360_graph_iteration t; '
                     'rgbd360_graph_default_params(&p); t.accepted = 0; return rgbd360_graph_optimize(g, &p, &r) + rgbd360_graph_get_trace(g, 1, 0, &t) + t.accepted; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(c_src)])
