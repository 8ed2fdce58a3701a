"""GPU tests of the pose-graph optimiser (rgbd360_graph_*, csrc/pose_graph.h) against the float64 numpy restatement
tests/pose_graph_reference.py on the graphs of tests/pose_graph_cases.py.  Every tolerance is that of the definition: none is
taken from what the device gives."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(n, f) for n in cases.NAMES for f in cases.FORMS]
IDS = ["%s-%s" % nf for nf in ALL]


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    r.setNumPyr(3)
    yield r
    r.close()


def make(reg, c):
    from rgbd360_amd.pose_graph import PoseGraph
    g = PoseGraph(reg)
    assert g.add_vertices(c["poses"], fixed=c["fixed"]) == 0
    g.add_edges(c["ei"], c["ej"], c["Z"], c["Om"])
    return g


@pytest.fixture(scope="module")
def optimised(reg):
    """Every graph optimised once at the test settings: name, form -> (poses, result, trace)."""
    out = {}
    for name, form in ALL:
        with make(reg, cases.case(name, form)) as g:
            res = g.optimize(**cases.OPT)
            out[name, form] = (g.poses(), res, g.trace())
    return out


@pytest.mark.parametrize("name,form", ALL + [("far", "consistent"), ("far", "noisy")], ids=IDS + ["far-consistent", "far-noisy"])
def test_linearisation_apply_and_chi2(reg, name, form):
    """r within 1e-9 of the reference for |t| <= 100 m (float64 rounding times about 10^2 operations at magnitude 10^2, margin 10^3), A within
    1e-9 |A|; y = (H + lambda diag H) x within 1e-10 |H| |x| of the dense product at lambda = 0 and 1e-3; chi2 to 1e-10 relative, above the
    rounding floor of a residual that is itself zero up to rounding (cases.chi2_floor: a tree started from its own chained odometry)."""
    c = cases.case(name, form)
    ref = cases.reference_graph(c)
    assert np.abs(c["poses"][:, :3, 3]).max() <= 100.0
    r_ref, A_ref = ref.linearize()
    H, g_ref, chi2_ref = ref.normal_equations()
    chi2_ref, per_ref = ref.chi2(per_edge=True)
    with make(reg, c) as g:
        r, A = g.linearize()
        dr = np.abs(r - r_ref).max()
        dA = max(np.linalg.norm(A[e] - A_ref[e]) / np.linalg.norm(A_ref[e]) for e in range(len(r)))
        chi2, per = g.chi2(per_edge=True)
        print(name, form, "max |r - ref|", dr, "max |A - ref| / |A|", dA, "chi2", chi2, "ref", chi2_ref)
        assert dr <= 1e-9 and dA <= 1e-9
        floor = cases.chi2_floor(ref)
        assert abs(chi2 - chi2_ref) <= 1e-10 * chi2_ref + floor.sum()
        assert (np.abs(per - per_ref) <= 1e-10 * per_ref + floor).all()
        x = np.random.default_rng(11).normal(size=(ref.n, 6))
        for lam in (0.0, 1e-3):
            y = g.apply(x, lam)
            want = (H + lam * np.diag(np.diag(H))) @ x[ref.free].reshape(-1)
            dy = np.abs(y[ref.free].reshape(-1) - want).max()
            bound = 1e-10 * np.linalg.norm(H, 2) * np.linalg.norm(x[ref.free])
            print("   lambda", lam, "max |y - Hx|", dy, "bound", bound)
            assert dy <= bound
            assert not y[ref.fixed].any()
        assert np.array_equal(g.poses(), c["poses"])      # nothing of this moved the graph


@pytest.mark.parametrize("name,form", ALL, ids=IDS)
def test_optimum_matches_the_dense_reference(optimised, name, form):
    """Every pose entry within 4 * 2^-23 * max(1, |ref|) of the reference's dense-solve optimum: both stop at a stationary point that agrees to
    about 1e-10 in float64 (tests/test_pose_graph_cpu.py pins that for the reference's own two solvers); what remains is the float32 rounding
    of the output with a margin of 4 ulp.  chi2_initial to 1e-10 relative.  On the consistent graphs also the ground truth, at the bound the
    CPU test holds the reference to."""
    c = cases.case(name, form)
    poses, res, trace = optimised[name, form]
    T_ref, res_ref, _ = cases.reference_optimum(name, form)
    tol = 4 * 2.0 ** -23 * np.maximum(1.0, np.abs(T_ref))
    worst = (np.abs(poses.astype(np.float64) - T_ref) / tol).max()
    print(name, form, "status", res["status"], "iterations", res["iterations"], "(reference %d)" % res_ref["iterations"], "cg", res["cg_iterations"],
          "chi2", res["chi2_initial"], "->", res["chi2_final"], "(reference %.17g)" % res_ref["chi2_final"], "worst |T - ref| / tol", worst)
    assert res["status"] == 0
    assert abs(res["chi2_initial"] - res_ref["chi2_initial"]) <= 1e-10 * res_ref["chi2_initial"] + cases.chi2_floor(cases.reference_graph(c)).sum()
    assert res["chi2_final"] <= res["chi2_initial"]
    assert worst <= 1.0
    ref = cases.reference_graph(c)
    assert (res["n_fixed"], res["n_isolated"]) == (int(ref.user_fixed.sum()), int(ref.isolated.sum()))
    assert poses[ref.fixed].tobytes() == c["poses"][ref.fixed].tobytes()      # fixed and isolated vertices: bit for bit what went in
    if form == "consistent":
        err = np.abs(poses.astype(np.float64) - c["gt"])[~ref.isolated].max()
        print("   max |T - truth|", err, "bound", cases.truth_bound(c))
        assert err <= cases.truth_bound(c)


@pytest.mark.parametrize("name,form", ALL, ids=IDS)
def test_trace_invariants(optimised, name, form):
    poses, res, trace = optimised[name, form]
    assert res["iterations"] == len(trace) >= 1
    assert res["accepted"] == sum(t["accepted"] for t in trace)
    assert res["cg_iterations"] == sum(t["cg_iterations"] for t in trace)
    assert trace[0]["lambda_"] == 1e-3 and trace[0]["chi2"] == res["chi2_initial"]
    accepted = [t for t in trace if t["accepted"]]
    for t in accepted:
        assert t["chi2_trial"] < t["chi2"]
    for a, b in zip(accepted, accepted[1:]):
        assert b["chi2"] < a["chi2"]      # chi2 strictly decreases over the accepted records
    for a, b in zip(trace, trace[1:]):
        if a["accepted"]:
            assert b["chi2"] == a["chi2_trial"] and b["lambda_"] == max(a["lambda_"] / 10.0, 1e-9)
        else:
            assert b["chi2"] == a["chi2"] and b["lambda_"] == a["lambda_"] * 10.0      # a rejected step left the poses alone: the same bits
            assert not a["chi2_trial"] < a["chi2"]
    for t in trace:
        assert 0 <= t["cg_iterations"] <= cases.OPT["cg_max_iters"] and t["max_update"] >= 0.0
    last = trace[-1]
    assert res["chi2_final"] == (last["chi2_trial"] if last["accepted"] else last["chi2"])
    assert res["converged"] == int(bool(last["accepted"]) and last["max_update"] <= cases.OPT["tol_update"])
    assert res["converged"] or len(trace) == cases.OPT["max_iters"]


@pytest.mark.parametrize("name,form", [("n300", "noisy"), ("variant", "consistent")], ids=["n300-noisy", "variant-consistent"])
def test_two_runs_give_the_same_bits(reg, optimised, name, form):
    with make(reg, cases.case(name, form)) as g:
        res = g.optimize(**cases.OPT)
        poses, res1, trace = optimised[name, form]
        assert g.poses().tobytes() == poses.tobytes() and res == res1 and g.trace() == trace
        assert g.chi2() == res["chi2_final"]      # chi2 at the poses the loop left is the bits it reported


def test_errors_leave_the_graph_unchanged(reg):
    from rgbd360_amd.pose_graph import PoseGraph
    from rgbd360_amd.register import Rgbd360Error
    c = cases.case("ring5", "noisy")
    with PoseGraph(reg) as g:
        res = g.optimize()      # an empty graph
        assert (res["status"], res["iterations"], res["chi2_initial"], res["chi2_final"]) == (0, 0, 0.0, 0.0) and g.trace() == []
        g.add_vertices(c["poses"])
        g.add_edges(c["ei"], c["ej"], c["Z"], c["Om"])
        with pytest.raises(Rgbd360Error, match="no fixed vertex"):
            g.optimize()
        g.set_fixed(0, [1])
        before = (g.n_vertices, g.n_edges, g.poses().tobytes(), g.chi2())
        eye = np.eye(4, dtype=np.float32)
        bad = eye.copy()
        bad[1, 3] = np.nan
        with pytest.raises(Rgbd360Error, match="edge 1: to = 5"):
            g.add_edges([0, 1], [1, 5], [eye, eye])
        with pytest.raises(Rgbd360Error, match="edge 0: from = -1"):
            g.add_edges([-1], [1], [eye])
        with pytest.raises(Rgbd360Error, match="edge 1: from == to"):
            g.add_edges([0, 2], [1, 2], [eye, eye])
        with pytest.raises(Rgbd360Error, match="edge 0: the relative pose"):
            g.add_edges([0], [1], [bad])
        with pytest.raises(Rgbd360Error, match="non-positive diagonal"):
            g.add_edges([0], [1], [eye], [np.diag([1, 1, 0, 1, 1, 1])])
        with pytest.raises(Rgbd360Error, match="vertex 1: the pose"):
            g.add_vertices([eye, bad])
        with pytest.raises(Rgbd360Error, match="vertex 2: the pose"):
            g.set_poses(2, [bad])
        with pytest.raises(Rgbd360Error):
            g.optimize(max_iters=-1)
        assert (g.n_vertices, g.n_edges, g.poses().tobytes(), g.chi2()) == before
        # and the graph still optimises to what a fresh one gives
        res = g.optimize(**cases.OPT)
        with make(reg, c) as fresh:
            assert fresh.optimize(**cases.OPT) == res and fresh.poses().tobytes() == g.poses().tobytes()
        # all vertices fixed, no iterations allowed: chi2 only
        g.set_fixed(0, [1] * 5)
        res = g.optimize()
        assert (res["status"], res["iterations"], res["n_fixed"]) == (0, 0, 5) and res["chi2_initial"] == res["chi2_final"] == g.chi2()
        g.clear()
        assert (g.n_vertices, g.n_edges) == (0, 0)


@pytest.fixture(scope="module")
def ring(reg):
    """Eight 256 x 128 frames on a ring through FrameStore.align: the consecutive pairs from the identity, then the closing pair from the
    pose the chained odometry gives it (what a SLAM front end knows at that moment)."""
    from rgbd360_amd import synth
    from rgbd360_amd.store import FrameStore
    frames = [synth.render(synth.trajectory_pose(k, 7), 256, 128, 7) for k in range(8)]
    pairs = [(k, k + 1) for k in range(7)] + [(7, 0)]
    with FrameStore(reg, 8, 128, 256) as st:
        st.put(list(range(8)), frames)
        poses, status, iters, results = st.align(pairs[:7], method=2)
        chained = np.eye(4)
        for k in range(7):
            chained = chained @ poses[k].astype(np.float64)
        p7, s7, _, r7 = st.align(pairs[7:], guesses=[R.rigid_inv(chained).astype(np.float32)], method=2)
    return frames, pairs, np.concatenate([poses, p7]), np.concatenate([status, s7]), results + r7


def test_store_edges_to_optimised_map(reg, ring):
    """store.align -> add_alignments -> optimize -> VoxelMap.move: status OK, chi2 does not grow, the poses meet the tolerance of the other
    graphs against the numpy reference on the same edges, and the map moved to the optimised poses is, bit for bit, the map filled there."""
    from rgbd360_amd.pose_graph import PoseGraph
    from rgbd360_amd.voxel_map import VoxelMap
    frames, pairs, rel, status, results = ring
    odo = [np.eye(4, dtype=np.float32)]
    for k in range(7):
        odo.append((odo[-1].astype(np.float64) @ rel[k].astype(np.float64)).astype(np.float32))
    odo = np.stack(odo)
    trg, src = [p[0] for p in pairs], [p[1] for p in pairs]
    with PoseGraph(reg) as g:
        g.add_vertices(odo, fixed=[0])
        skipped = g.add_alignments(trg, src, rel, results)
        assert skipped == int((status != 0).sum()) and g.n_edges == 8 - skipped and skipped == 0
        res = g.optimize(**cases.OPT)
        opt = g.poses()
    Om = np.stack([np.array(r.hessian, np.float32).reshape(6, 6).T for r in results])
    T_ref, res_ref, _ = R.optimize(R.Graph(odo, [True] + [False] * 7, trg, src, rel, Om), **cases.OPT)
    worst = (np.abs(opt.astype(np.float64) - T_ref) / (4 * 2.0 ** -23 * np.maximum(1.0, np.abs(T_ref)))).max()
    print("ring of 8: status", res["status"], "iterations", res["iterations"], "chi2", res["chi2_initial"], "->", res["chi2_final"],
          "reference", res_ref["chi2_final"], "worst |T - ref| / tol", worst, "largest correction", np.abs(opt - odo).max())
    assert res["status"] == 0 and res["chi2_final"] <= res["chi2_initial"]
    assert worst <= 1.0
    with VoxelMap(reg, leaf=0.05, capacity=1 << 18) as moved, VoxelMap(reg, leaf=0.05, capacity=1 << 18) as fresh:
        for k, (rgb, depth) in enumerate(frames):
            moved.insert_sphere(rgb, depth, odo[k])
            fresh.insert_sphere(rgb, depth, opt[k])
        assert not moved.full and not fresh.full
        for k, (rgb, depth) in enumerate(frames):
            if not np.array_equal(odo[k], opt[k]):
                moved.move_sphere(rgb, depth, odo[k], opt[k])
                assert not moved.mismatch and not moved.full
        a, b = moved.extract(), fresh.extract()
        assert len(a[0]) > 1000
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_pose_graph_slam_example(hip_lib, tmp_path):
    """examples/pose_graph_slam.cpp on a dumped synthetic ring: every frame a keyframe, odometry and closure edges from the store, one
    optimisation, the map re-posed; exit 0 and one `keyframe` line per frame."""
    from rgbd360_amd import build
    lib = build.build()
    exe = os.path.join(str(tmp_path), "pose_graph_slam")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "pose_graph_slam.cpp"),
                           "-L" + os.path.dirname(lib), "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-pthread", "-o", exe])
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "8", "256", "128"])
    out = subprocess.run([exe, str(seq), "8", "256", "128", "0.0", "10.0"], text=True, capture_output=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    lines = out.stdout.splitlines()
    assert len([l for l in lines if l.startswith("keyframe ")]) == 8
    graph = [l.split() for l in lines if l.startswith("graph ")]
    assert len(graph) == 1 and int(graph[0][graph[0].index("status") + 1]) == 0
    assert int(graph[0][graph[0].index("edges") + 1]) > 7      # odometry edges and at least one closure
