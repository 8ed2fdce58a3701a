"""The serial Gauss-Newton step of the spherical path (solve_waves / solve_finish / fs_write_state, qr_rank6_lanes /
lu_inverse6_lanes, photo_icp_kernels.h) driven from chosen states through rgbd360_debug_solve_state, against the float64 / float32 /
mpmath references of tests/gn_reference.py and the CPU oracle.  Every case runs through the three routes -- k_solve (0), the prologue
of the fused launch k_eval_fs (1), the same with the row late in the table (2) -- which must agree bit for bit.  The three routes
run the same solve code (route 0 had a form of its own once); the hand-made cases -- the pseudo-exponential's branches, the
bookkeeping, the rank and pivot edges -- are also compared, on every route, with the bits that old form of route 0 left in
tests/golden/solve_bits.json (tools/solve_bits.py; the cases live in tests/solve_cases.py).  The large sweeps are not in the file:
gn_reference.update_f32 pins their update bit for bit and the oracle their verdicts."""
import ctypes as C
import math

import numpy as np
import pytest

import gn_reference as R
import solve_cases as S
from rgbd360_amd import synth

pytestmark = pytest.mark.gpu

F = np.float32
ROUTES = (0, 1, 2)


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    (rgbA, dA), (rgbB, dB), _ = synth.make_pair(2048, 1024, seed=3)      # level 1 still has more than 40 block rows (route 2)
    r = RegisterPhotoICP()
    r.setTargetFrame(rgbA, dA)
    r.setSourceFrame(rgbB, dB)
    return r


def _bits(x):
    return np.asarray(x).view(np.uint32 if np.asarray(x).dtype == F else np.uint64)


def _same_float(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


KEYS_I = ("status", "done", "level_active", "it", "n_evals", "iters")
KEYS_F = ("lam", "error", "new_error", "diff_error")


@pytest.fixture(scope="module")
def recorded():
    return S.load_recorded()


def _run_case(reg, recorded, case):
    """_run on a case of tests/solve_cases.py, every route against the case's recorded bits."""
    return _run(reg, case["level"], case["row"], recorded=recorded[case["name"]], **case["kw"])


def _run(reg, level, row, recorded=None, **kw):
    """All three routes; asserts they agree bit for bit -- and with the recorded state, where there is one (pend_nb on route 0 only: a
    fused launch leaves its own pass pending, as many rows as its frame has) -- and returns route 0's state."""
    outs = [reg.debug_solve_state(level, row, route=r, **kw) for r in ROUTES]
    o0 = outs[0]
    if recorded is not None:
        for r, o in zip(ROUTES, outs):
            differ = S.differences(o, recorded, skip=("pend_nb",) if r else ())
            assert not differ, (r, differ)
    for o in outs[1:]:
        for k in KEYS_I:
            assert o[k] == o0[k], (k, o, o0)
        for k in KEYS_F:
            assert _same_float(o[k], o0[k]), (k, o[k], o0[k])
        for k in ("cand", "pose", "update"):
            assert np.array_equal(_bits(o[k]), _bits(o0[k])), (k, o[k], o0[k])
        # the fused launch leaves its own pass pending exactly when the new state runs one on this level
        assert (o["pend_nb"] > 0) == (o["done"] == 0 and o["level_active"] == level), o
    assert o0["pend_nb"] == 0
    return o0


def _step_row(H, g):
    return R.partial_row(H, g, e2=(3.0, 2.0), n=(1000, 800, 1500))


# -------------------------------------------------------------------------------------------------------------------------------
# 1. the update against float64
# -------------------------------------------------------------------------------------------------------------------------------
def test_update_within_the_float64_bound(reg, oracle_mod):
    """300 dense SPD systems (condition 1 .. 1e5, every pivoting case: row swaps at every LU step, QR column swaps): each entry of the
    device update lies within
        64 u (|H^-1| P^T|L||U| |H^-1| |g|) + 8 u (|H^-1| |g|)
    of the float64 solution of the float32 system (constants derived in gn_reference.update_bound), and so does the oracle's gn_step
    update.  The device update is also the float32 restatement of the reciprocal-form LU (gn_reference.update_f32) bit for bit."""
    rng = np.random.default_rng(101)
    cases = R.cond_sweep(rng, 240, cond_max=1e5) + R.pivot_sweep(rng, 30) + R.qr_swap_sweep(rng, 30)
    worst_dev = worst_ora = 0.0
    tight = 0
    for H, g in cases:
        b, u64 = R.update_bound(H, g)
        out = _run(reg, 0, _step_row(H, g))
        assert out["status"] == 0 and out["done"] == 0, out
        u = out["update"].astype(np.float64)
        assert np.array_equal(_bits(out["update"]), _bits(R.update_f32(H, g, "rcp"))), (out["update"], R.update_f32(H, g, "rcp"))
        st, _, uo = oracle_mod.gn_step(H, g, 1.0, np.eye(4))
        assert st == 0
        worst_dev = max(worst_dev, float((np.abs(u - u64) / b).max()))
        worst_ora = max(worst_ora, float((np.abs(uo.astype(np.float64) - u64) / b).max()))
        assert np.all(np.abs(u - u64) <= b), (np.abs(u - u64) / b)
        assert np.all(np.abs(uo.astype(np.float64) - u64) <= b)
        tight += bool(b.max() < 1e-3 * np.linalg.norm(u64))
    print(f"update vs float64: worst error / bound device {worst_dev:.4f} oracle {worst_ora:.4f}; {tight} of {len(cases)} systems "
          f"with a bound below 1e-3 |u|")
    assert tight >= 20


# -------------------------------------------------------------------------------------------------------------------------------
# 2. the rank verdict against the oracle
# -------------------------------------------------------------------------------------------------------------------------------
def _oracle_rank(L, M):
    return L.oracle_rank6(np.ascontiguousarray(np.asarray(M, F).T.reshape(36)).ctypes.data_as(C.c_void_p))


def test_rank_verdict_equals_the_oracle_on_the_near_threshold_sweep(reg, oracle_mod):
    """(H + lambda diag H).rank() != 6 decides ILL-POSED (RPI.h:4682).  Over the near-threshold sweep (sigma_min / sigma_max in
    [1e-8, 1e-5], lambda = 5^-k formed as the device forms it, k = 0..11) the device says ILL-POSED exactly where the oracle's
    rank is not 6 -- including the matrices on which a reciprocal form of the Householder quotients would decide otherwise."""
    L = oracle_mod.lib()
    sweep = R.near_threshold_sweep()
    n_ill = n_full = 0
    bad = []
    for H, g, k, lam in sweep:
        M = R.damped(H, F(lam))
        want_ill = _oracle_rank(L, M) != 6
        out = _run(reg, 0, _step_row(H, g), lam=lam)
        got_ill = out["status"] == 1
        assert out["status"] in (0, 1)
        if got_ill != want_ill:
            bad.append((k, lam, R.rank6_f32(M, "div"), R.rank6_f32(M, "rcp"), out["status"]))
        n_ill += want_ill
        n_full += not want_ill
    print(f"rank verdicts: {len(sweep)} matrices, {n_full} full rank, {n_ill} ILL-POSED; {len(bad)} device verdicts differ")
    assert not bad, bad[:10]


def test_rank_and_pivot_edges_agree_with_the_oracle(reg, oracle_mod, recorded):
    """An exact zero LU pivot, an exactly singular matrix, and entries scaled by 2^j so that squared column norms overflow or
    underflow float32: the device's verdict is the oracle gn_step's (rank test, then the inverse's zero-pivot test), whatever it is."""
    cases = S.rank_edge_cases()
    assert len(cases) == 2 * len(R.rank_edge_cases())
    for c in cases:
        st, _, upd = oracle_mod.gn_step(c["H"], c["g"], F(c["lam"]), np.eye(4))
        out = _run_case(reg, recorded, c)
        assert out["status"] == st, (c["label"], c["k"], out["status"], st)


# -------------------------------------------------------------------------------------------------------------------------------
# 3. scale invariance
# -------------------------------------------------------------------------------------------------------------------------------
def test_update_is_invariant_under_power_of_two_scaling(reg):
    """H, g -> 2^j H, 2^j g leaves the update unchanged bit for bit wherever the reference proves every value of the inverse and the
    update stays a normal float32 and every pivot stays where the device reciprocal is exact (gn_reference.scale_safe)."""
    rng = np.random.default_rng(33)
    n_checked = 0
    for H, g in R.cond_sweep(rng, 4, cond_max=1e4) + R.pivot_sweep(rng, 2):
        u0 = _run(reg, 0, _step_row(H, g))["update"]
        for j in range(-40, 41, 5):
            if not R.scale_safe(H, g, j):
                continue
            s = 2.0 ** j
            out = _run(reg, 0, _step_row(H.astype(np.float64) * s, g.astype(np.float64) * s))
            assert out["status"] == 0
            assert np.array_equal(_bits(out["update"]), _bits(u0)), (j, out["update"], u0)
            n_checked += 1
    assert n_checked >= 80


# -------------------------------------------------------------------------------------------------------------------------------
# 4. the pseudo-exponential's branches
# -------------------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    def key(x):
        i = np.asarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _oracle_pexp(L, v):
    E = np.zeros(16)
    L.oracle_se3_pseudo_exp(np.ascontiguousarray(v, np.float64).ctypes.data_as(C.c_void_p), E.ctypes.data_as(C.c_void_p))
    return E.reshape(4, 4).T.copy()


def test_pseudo_exponential_branches(reg, oracle_mod, recorded):
    """H = 2^k I makes the update exactly -2^-k g.  Rotation angles 0, 2^-45 (the threshold of gn::se3_pseudo_exp) and one float32
    step on either side, 1e-8, 0.49 / 0.5 / 0.51 (theta^2 = 0.25: series against sin / cos), 1, 2, 3.1, pi, 3.5.  At the identity
    pose the candidate is within 1 ulp of float32(Rodrigues(update)) evaluated in mpmath, its translation column is the update bit
    for bit, and around the threshold the branch is gn::se3_pseudo_exp's; at another pose the candidate is within
    8 u (|E||P|) of the float64 product."""
    L = oracle_mod.lib()
    thr = R.ROT_THRESHOLD
    cases = S.pseudo_exp_cases()
    assert len(cases) == 26
    for c in cases:
        w, u, P = c["w"], c["u"], c["P"]
        out = _run_case(reg, recorded, c)
        assert out["status"] == 0 and np.array_equal(_bits(out["update"]), _bits(u)), (out["update"], u)
        cand = out["cand"]
        v = u.astype(np.float64)
        if c["at_P"]:
            E = R.pseudo_exp_mp(v)
            want = E @ P.astype(np.float64)
            bound = 8 * R.U32 * (np.abs(E) @ np.abs(P.astype(np.float64)))
            assert np.all(np.abs(cand - want) <= bound), (np.linalg.norm(w), np.abs(cand - want) / np.maximum(bound, 1e-300))
            continue
        assert np.array_equal(_bits(cand[:3, 3]), _bits(u[:3]))
        assert np.array_equal(cand[3], F([0, 0, 0, 1]))
        wn = float(np.linalg.norm(v[3:]))
        if abs(wn - thr) <= thr * 1e-6 or wn == 0.0:
            E_o = _oracle_pexp(L, v).astype(F)
            assert np.array_equal(cand[:3, :3] != np.eye(3, dtype=F), E_o[:3, :3] != np.eye(3, dtype=F)), (wn, cand, E_o)
            assert np.array_equal(cand[:3, :3], E_o[:3, :3]), (wn, cand, E_o)
        else:
            want = R.pseudo_exp_f32_mp(v)
            assert _ulps(cand, want).max() <= 1, (wn, _ulps(cand, want))


# -------------------------------------------------------------------------------------------------------------------------------
# 5. the bookkeeping against the restatement
# -------------------------------------------------------------------------------------------------------------------------------
def test_bookkeeping_matches_the_restatement(reg, recorded):
    """Accept when diff > tol_residual (diff equal: no), it against max_iters, |update| against tol_update, forced, the occlusion
    error sqrt(E2P / NP) + sqrt(E2D / ND) with a modality empty, NaN totals, no residuals, and the hand-over of a finished level to
    the next finer one: every field of the state equals gn_reference.solve_step's."""
    H, g, cases = S.bookkeeping_cases()
    assert len(cases) == 23
    H32, g32 = H.astype(F), g.astype(F)
    for case in cases:
        name, c = case["label"], case["c"]
        out = _run_case(reg, recorded, case)
        st = R.SolveState(level=c["level"], pose=c["pose"], update=c["update"], lam=c["lam"], error=c["error"], first=c["first"],
                          it=c["it"])
        want = R.solve_step(st, H32, g32, c["e2"][0], c["e2"][1], c["n"][0], c["n"][1], occ=c["occlusion"], max_iters=c["max_iters"],
                            tol_residual=c["tol_residual"], tol_update=c["tol_update"], forced=c["forced"])
        for k in ("status", "done", "level_active", "it", "n_evals"):
            assert out[k] == getattr(want, k), (name, k, out[k], getattr(want, k))
        assert out["iters"] == want.iters, (name, out["iters"], want.iters)
        for k, wk in (("lam", "lam"), ("error", "error"), ("new_error", "new_error"), ("diff_error", "diff_error")):
            assert _same_float(out[k], getattr(want, wk)), (name, k, out[k], getattr(want, wk))
        for k in ("pose", "cand", "update"):
            assert np.array_equal(_bits(out[k]), _bits(getattr(want, k))), (name, k, out[k], getattr(want, k))
