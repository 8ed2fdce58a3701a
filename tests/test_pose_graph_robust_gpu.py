"""GPU tests of the robust and switchable edges of the pose-graph optimiser (rgbd360_graph_set_edge_robust / _enabled / edge_weights,
csrc/pose_graph.h) against the float64 numpy restatement tests/pose_graph_robust_reference.py.  The graphs are n70/noisy and n300/noisy of
tests/pose_graph_cases.py with some closures replaced by wrong ones; robust settings apply to the closure edges only, delta = 6.  Every
tolerance is that of the definition; tests/test_pose_graph_robust_cpu.py pins what they assume of the reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_reference as R
import pose_graph_robust_reference as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
COMBO_IDS = ["%s-%s" % (n, RR.KIND_NAMES[k]) for n, k in RR.COMBOS]
RUNS = RR.COMBOS + (("n70", RR.NONE), ("n300", RR.NONE))


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


def make_corrupted(reg, name, kind):
    """The corrupted graph with `kind` on its closure edges."""
    c, _ = RR.corrupted(name)
    g = make(reg, c)
    if kind != RR.NONE:
        first = RR.FIRST_CLOSURE[name]
        g.set_edge_robust(first, np.full(len(c["ei"]) - first, kind), RR.DELTA)
    return g


def tolerance(T_ref):
    return 4 * 2.0 ** -23 * np.maximum(1.0, np.abs(T_ref))


@pytest.fixture(scope="module")
def optimised(reg):
    """Every robust run once: (name, kind) -> (poses, result, trace, weights at the end)."""
    out = {}
    for name, kind in RUNS:
        with make_corrupted(reg, name, kind) as g:
            res = g.optimize(**RR.OPT)
            out[name, kind] = (g.poses(), res, g.trace(), g.edge_weights()[3])
    return out


# ---- 1: the bits of the commit before the kinds existed
def _all_none(g):
    g.set_edge_robust(0, np.zeros(g.n_edges, np.int32))
    g.set_edge_enabled(0, np.ones(g.n_edges, bool))


def _huge_huber(g):
    g.set_edge_robust(0, np.full(g.n_edges, RR.HUBER), 1e150)


@pytest.mark.parametrize("configure", [None, _all_none, _huge_huber], ids=["nothing_set", "all_none_enabled", "huber_1e150"])
def test_quadratic_graphs_keep_the_parents_bits(reg, configure):
    """tests/golden/pose_graph_bits.json was recorded with tests/golden/make_golden_pose_graph_bits.py from the library before k_pg_edges
    gained the weight.  A graph whose edges are all quadratic -- nothing set, NONE and enabled set explicitly, or Huber with a threshold
    delta^2 = 1e300 no s reaches -- gives those bits: poses, result and trace.  (w is an exact 1.0, rho is s itself.)"""
    import make_golden_pose_graph_bits as G
    want = json.load(open(G.OUT))
    got = G.compute(reg, configure)
    assert sorted(got) == sorted(want) == sorted("%s/%s" % nf for nf in G.CASES)
    for key in want:
        assert got[key]["result"] == want[key]["result"], key
        assert got[key]["trace"] == want[key]["trace"], key
        assert got[key]["poses_sha256"] == want[key]["poses_sha256"], key


# ---- 2: s, rho, w, the cost and the weighted operator at the start poses
@pytest.mark.parametrize("name", ["n70", "n300"])
@pytest.mark.parametrize("kind", RR.KINDS, ids=[RR.KIND_NAMES[k] for k in RR.KINDS])
def test_edge_weights_cost_and_apply_at_the_start(reg, name, kind):
    """s within the bound of the quadratic tests, 1e-10 s + cases.chi2_floor; rho within the same bound since d rho / d s <= 1; w within
    2 / delta^2 times it since |d w / d s| <= 2 / delta^2 for all three kinds; the cost is bit for bit what chi2() returns; y = (H + lambda
    diag H) x with the weighted H within 1e-10 |H| |x| of the reference's dense product at lambda = 0 and 1e-3."""
    c, bad = RR.corrupted(name)
    ref = RR.graph(name, kind)
    cost_ref, s_ref, rho_ref, w_ref = ref.edge_weights()
    H, _, _ = ref.normal_equations()
    bound = 1e-10 * np.abs(s_ref) + cases.chi2_floor(ref)
    with make_corrupted(reg, name, kind) as g:
        cost, s, rho, w = g.edge_weights()
        chi2, per = g.chi2(per_edge=True)
        print(name, RR.KIND_NAMES[kind], "max |s - ref| / bound", (np.abs(s - s_ref) / bound).max(), "|rho - ref| / bound", (np.abs(rho - rho_ref) / bound).max(),
              "|w - ref| / bound", (np.abs(w - w_ref) / (2.0 / RR.DELTA ** 2 * bound)).max(), "cost", cost, "ref", cost_ref, "w of the wrong edges", w[list(bad)])
        assert (np.abs(s - s_ref) <= bound).all() and np.array_equal(per, s)
        assert (np.abs(rho - rho_ref) <= bound).all()
        assert (np.abs(w - w_ref) <= 2.0 / RR.DELTA ** 2 * bound).all()
        assert (w[:RR.FIRST_CLOSURE[name]] == 1.0).all() and ((w > 0.0) & (w <= 1.0)).all()
        assert cost == chi2 and abs(cost - cost_ref) <= bound.sum()
        x = np.random.default_rng(11).normal(size=(ref.n, 6))
        for lam in (0.0, 1e-3):
            y = g.apply(x, lam)
            want = (H + lam * np.diag(np.diag(H))) @ x[ref.free].reshape(-1)
            dy = np.abs(y[ref.free].reshape(-1) - want).max()
            limit = 1e-10 * np.linalg.norm(H, 2) * np.linalg.norm(x[ref.free])
            print("   lambda", lam, "max |y - Hx|", dy, "bound", limit)
            assert dy <= limit
            assert not y[ref.fixed].any()
        r, A = g.linearize()      # still the unweighted r and A
        r_ref, A_ref = ref.linearize()
        assert np.abs(r - r_ref).max() <= 1e-9 and max(np.linalg.norm(A[e] - A_ref[e]) / np.linalg.norm(A_ref[e]) for e in range(len(r))) <= 1e-9
        assert np.array_equal(g.poses(), c["poses"])


# ---- 3: the optimum
@pytest.mark.parametrize("name,kind", RR.COMBOS, ids=COMBO_IDS)
def test_robust_optimum_matches_the_dense_reference(optimised, name, kind):
    """Every pose entry within 4 * 2^-23 * max(1, |ref|) of the robust reference's dense-solve optimum, status 0: the tolerance of the
    quadratic graphs, fair because the reference's own two solvers end within 0.01 of it of each other on these five combinations
    (tests/test_pose_graph_robust_cpu.py).  n300 with Geman-McClure is not a case: its cost is non-convex enough there for the two solvers of the
    reference to part by 1.2 tolerances."""
    poses, res, trace, _ = optimised[name, kind]
    T_ref = RR.stored_optimum(name, kind)
    worst = (np.abs(poses.astype(np.float64) - T_ref) / tolerance(T_ref)).max()
    print(name, RR.KIND_NAMES[kind], "status", res["status"], "iterations", res["iterations"], "converged", res["converged"], "cg", res["cg_iterations"],
          "cost", res["chi2_initial"], "->", res["chi2_final"], "worst |T - ref| / tol", worst)
    assert res["status"] == 0
    assert res["chi2_final"] <= res["chi2_initial"]
    assert worst <= 1.0


# ---- 4: recovery, on the device's own poses
def test_device_recovers_from_the_wrong_closures(optimised):
    """The quadratic optimiser is bent by more than 0.5 m on both graphs (reference: 0.906 and 0.682 m); Cauchy ends within 0.05 m of the
    optimum of the graph without the wrong edges on both (0.016, 0.018), Geman-McClure on n70 (0.004).  After Cauchy every wrong edge has
    w < 0.1 and every other edge w > 0.1 (reference: <= 2.6e-3 against >= 0.43)."""
    for name in ("n70", "n300"):
        clean = RR.stored_optimum(name, "clean")
        bad = list(RR.corrupted(name)[1])
        d_quad = RR.distance(optimised[name, RR.NONE][0], clean)
        d_cauchy = RR.distance(optimised[name, RR.CAUCHY][0], clean)
        w = optimised[name, RR.CAUCHY][3]
        others = np.setdiff1d(np.arange(len(w)), bad)
        print(name, "distance: quadratic", d_quad, "Cauchy", d_cauchy, "; Cauchy weights: wrong edges <=", w[bad].max(), ", the others >=", w[others].min())
        assert optimised[name, RR.NONE][1]["status"] == 0 and d_quad > 0.5
        assert d_cauchy < 0.05
        assert (w[bad] < 0.1).all() and (w[others] > 0.1).all()
    d_gm = RR.distance(optimised["n70", RR.GEMAN_MCCLURE][0], RR.stored_optimum("n70", "clean"))
    print("n70 distance: Geman-McClure", d_gm)
    assert d_gm < 0.05


# ---- 5: switching edges off and on again
@pytest.mark.parametrize("name", ["n70", "n300"])
def test_disabled_edges_are_absent_edges(reg, optimised, name):
    """With the wrong closures disabled (all kinds NONE) the optimum is within the tolerance of the reference on the graph BUILT without
    them; per_edge still reports their s; chi2 leaves them out.  Enabled again and back at the start poses, the run gives the bits of a graph
    that never had an edge disabled."""
    c, bad = RR.corrupted(name)
    bad = list(bad)
    E = len(c["ei"])
    en = np.ones(E, bool)
    en[bad] = False
    T_ref = RR.stored_optimum(name, "clean")
    with make_corrupted(reg, name, RR.NONE) as g:
        for e in bad:
            g.set_edge_enabled(e, [False])
        assert np.array_equal(g.edge_state()[2], en)
        res = g.optimize(**RR.OPT)
        poses = g.poses()
        worst = (np.abs(poses.astype(np.float64) - T_ref) / tolerance(T_ref)).max()
        chi2, per = g.chi2(per_edge=True)
        cost, s, rho, w = g.edge_weights()
        print(name, "status", res["status"], "iterations", res["iterations"], "worst |T - ref| / tol", worst, "cost", chi2, "s of the disabled edges", per[bad])
        assert res["status"] == 0 and (res["n_fixed"], res["n_isolated"]) == (1, 0)
        assert worst <= 1.0
        assert chi2 == res["chi2_final"] == cost
        assert np.array_equal(s, per) and not rho[bad].any() and not w[bad].any() and np.array_equal(rho[en], s[en]) and (w[en] == 1.0).all()
        # against the reference, at poses both can stand on: the float32 read-out put back (the loop's own poses are float64)
        g.set_poses(0, poses)
        chi2, per = g.chi2(per_edge=True)
        ref = RR.RobustGraph(poses, c["fixed"], c["ei"], c["ej"], c["Z"], c["Om"], enabled=en)
        cost_ref, s_ref, _, _ = ref.edge_weights()
        bound = 1e-10 * np.abs(s_ref) + cases.chi2_floor(ref)
        print("   at the float32 poses: cost", chi2, "ref", cost_ref, "with the disabled edges", s_ref.sum(), "max |s - ref| / bound", (np.abs(per - s_ref) / bound).max())
        assert (np.abs(per - s_ref) <= bound).all() and (per[bad] > 0.0).all()
        assert abs(chi2 - cost_ref) <= bound[en].sum()      # the reference's cost leaves the disabled edges out: their s is far above the bound
        assert per[bad].min() > 1e3 * bound[en].sum()
        g.set_edge_enabled(0, np.ones(E, bool))
        g.set_poses(0, c["poses"])
        res2 = g.optimize(**RR.OPT)
        never_poses, never_res, never_trace, _ = optimised[name, RR.NONE]
        assert g.poses().tobytes() == never_poses.tobytes() and res2 == never_res and g.trace() == never_trace


# ---- 6: a vertex whose edges are all disabled
def test_starved_vertex_is_isolated_and_keeps_its_pose(reg):
    c = cases.case("variant", "consistent")
    v = 77
    assert not c["fixed"][v]
    mine = np.flatnonzero((c["ei"] == v) | (c["ej"] == v))
    assert len(mine) >= 2
    with make(reg, c) as g:
        base = g.optimize(max_iters=0)
        for e in mine:
            g.set_edge_enabled(int(e), [0])
        res = g.optimize(**cases.OPT)
        poses = g.poses()
        print("variant: vertex", v, "edges", mine, "n_isolated", base["n_isolated"], "->", res["n_isolated"], "status", res["status"], "iterations", res["iterations"])
        assert res["n_isolated"] == base["n_isolated"] + 1 and res["n_fixed"] == base["n_fixed"]
        assert res["status"] == 0 and res["chi2_final"] < res["chi2_initial"]
        assert poses[v].tobytes() == c["poses"][v].tobytes()
        assert not np.array_equal(poses[v - 1], c["poses"][v - 1])      # its neighbours moved


# ---- 7: determinism and the trace
def test_two_cauchy_runs_give_the_same_bits(reg, optimised):
    with make_corrupted(reg, "n300", RR.CAUCHY) as g:
        res = g.optimize(**RR.OPT)
        poses, res1, trace, w = optimised["n300", RR.CAUCHY]
        assert g.poses().tobytes() == poses.tobytes() and res == res1 and g.trace() == trace
        assert g.chi2() == res["chi2_final"]      # the cost at the poses the loop left is the bits it reported
        assert np.array_equal(g.edge_weights()[3], w)


@pytest.mark.parametrize("name,kind", RR.COMBOS, ids=COMBO_IDS)
def test_robust_trace_invariants(optimised, name, kind):
    """The invariants of tests/test_pose_graph_gpu.py::test_trace_invariants, on the robust cost."""
    poses, res, trace, _ = optimised[name, kind]
    assert res["iterations"] == len(trace) >= 1
    assert res["accepted"] == sum(t["accepted"] for t in trace)
    assert res["cg_iterations"] == sum(t["cg_iterations"] for t in trace)
    assert trace[0]["lambda_"] == 1e-3 and trace[0]["chi2"] == res["chi2_initial"]
    accepted = [t for t in trace if t["accepted"]]
    for t in accepted:
        assert t["chi2_trial"] < t["chi2"]
    for a, b in zip(accepted, accepted[1:]):
        assert b["chi2"] < a["chi2"]
    for a, b in zip(trace, trace[1:]):
        if a["accepted"]:
            assert b["chi2"] == a["chi2_trial"] and b["lambda_"] == max(a["lambda_"] / 10.0, 1e-9)
        else:
            assert b["chi2"] == a["chi2"] and b["lambda_"] == a["lambda_"] * 10.0
            assert not a["chi2_trial"] < a["chi2"]
    for t in trace:
        assert 0 <= t["cg_iterations"] <= RR.OPT["cg_max_iters"] and t["max_update"] >= 0.0
    last = trace[-1]
    assert res["chi2_final"] == (last["chi2_trial"] if last["accepted"] else last["chi2"])
    assert res["converged"] == int(bool(last["accepted"]) and last["max_update"] <= RR.OPT["tol_update"])
    assert res["converged"] or len(trace) == RR.OPT["max_iters"]


# ---- 8: bad arguments
def test_bad_arguments_change_nothing(reg, optimised):
    from rgbd360_amd.register import Rgbd360Error
    name = "n70"
    c, _ = RR.corrupted(name)
    E = len(c["ei"])
    with make_corrupted(reg, name, RR.CAUCHY) as g:
        g.set_edge_enabled(75, [0])
        g.set_edge_enabled(75, [1])
        before = tuple(a.tobytes() for a in g.edge_state()) + (g.poses().tobytes(),)
        kinds0, deltas0, enabled0 = g.edge_state()
        assert (kinds0[:69] == RR.NONE).all() and (kinds0[69:] == RR.CAUCHY).all() and (deltas0[69:] == RR.DELTA).all() and (deltas0[:69] == 1.0).all() and enabled0.all()
        for first, kinds, deltas, match in (
                (E - 1, [1, 1], [1.0, 1.0], "edge range"), (-1, [0], None, "edge range"), (E, [0], None, "edge range"),
                (70, [1, 4, 7], [1.0, 1.0, 1.0], "edge 71: kind = 4"), (70, [-1], [1.0], "edge 70: kind = -1"),
                (10, [0, 2, 2], [1.0, np.nan, 0.0], "edge 11: delta"), (10, [3], [0.0], "edge 10: delta"), (10, [1], [-2.0], "edge 10: delta"),
                (10, [0, 0, 1], [1.0, 1.0, np.inf], "edge 12: delta"), (20, [0, 2], None, "edge 21: a robust kind needs a delta")):
            with pytest.raises(Rgbd360Error, match=match):
                g.set_edge_robust(first, np.array(kinds, np.int32), None if deltas is None else np.array(deltas))
        for first, flags in ((E - 1, [1, 1]), (-1, [1]), (E, [0])):
            with pytest.raises(Rgbd360Error, match="edge range"):
                g.set_edge_enabled(first, flags)
        g.set_edge_robust(10, [0, 0], [np.nan, -1.0])      # the delta of a NONE edge is not looked at ...
        g.set_edge_robust(10, [0, 0])                      # ... and may be absent
        assert tuple(a.tobytes() for a in g.edge_state()) + (g.poses().tobytes(),) == before
        res = g.optimize(**RR.OPT)
        poses, res1, trace, _ = optimised[name, RR.CAUCHY]
        assert g.poses().tobytes() == poses.tobytes() and res == res1 and g.trace() == trace
        g.clear()      # forgets the settings
        g.add_vertices(c["poses"], fixed=c["fixed"])
        g.add_edges(c["ei"], c["ej"], c["Z"], c["Om"])
        kinds, deltas, enabled = g.edge_state()
        assert not kinds.any() and (deltas == 1.0).all() and enabled.all()


# ---- 9: the example
def test_pose_graph_slam_example_with_a_robust_delta(hip_lib, tmp_path):
    """examples/pose_graph_slam.cpp: a 9th argument 0 prints byte for byte what 8 arguments print; with delta = 6 every closure gets one
    `weight` line after the last optimisation and the run still ends with status 0."""
    from rgbd360_amd import build
    lib = build.build()
    exe = os.path.join(str(tmp_path), "pose_graph_slam")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "pose_graph_slam.cpp"),
                           "-L" + os.path.dirname(lib), "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-pthread", "-o", exe])
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "8", "256", "128"])
    args = [exe, str(seq), "8", "256", "128", "0.0", "10.0", "3", "0"]
    plain = subprocess.run(args, capture_output=True)
    zero = subprocess.run(args + ["0"], capture_output=True)
    robust = subprocess.run(args + ["6"], text=True, capture_output=True)
    print(robust.stdout, robust.stderr)
    assert plain.returncode == zero.returncode == robust.returncode == 0
    assert plain.stdout == zero.stdout and b"weight" not in plain.stdout and plain.stdout.count(b"keyframe ") == 8
    lines = robust.stdout.splitlines()
    closures = [tuple(l.split()[1:3]) for l in lines if l.startswith("closure ") and l.split()[-1] == "0"]
    optimise = [k for k, l in enumerate(lines) if l.startswith("optimise ")]
    assert len(closures) >= 1 and len(optimise) >= 1
    start = optimise[-2] + 1 if len(optimise) > 1 else 0
    weights = [l.split() for l in lines[start:optimise[-1]] if l.startswith("weight ")]
    assert [tuple(t[1:3]) for t in weights] == closures
    assert all(0.0 <= float(t[3]) <= 1.0 for t in weights)
    graph = [l.split() for l in lines if l.startswith("graph ")]
    assert len(graph) == 1 and int(graph[0][graph[0].index("status") + 1]) == 0
    assert len([l for l in lines if l.startswith("keyframe ")]) == 8
