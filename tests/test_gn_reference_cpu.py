"""tests/gn_reference.py against the CPU oracle (oracle/photo_icp_ref.cpp: gn::rank6 / gn::inverse6 / se3_pseudo_exp restated the
way Eigen / MRPT compute them) -- the references the GPU solve tests (test_gn_solve_exact.py) hold the device to.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import gn_reference as R

F = np.float32


def _cm(M):
    return np.ascontiguousarray(np.asarray(M, F).T.reshape(36))


def _oracle_rank(L, M):
    return L.oracle_rank6(_cm(M).ctypes.data_as(C.c_void_p))


def _oracle_inverse(L, M):
    inv = np.zeros(36, F)
    st = L.oracle_inverse6(_cm(M).ctypes.data_as(C.c_void_p), inv.ctypes.data_as(C.c_void_p))
    return st, inv.reshape(6, 6).T.copy()


def _all_sweeps():
    rng = np.random.default_rng(11)
    out = [(H, g) for H, g in R.cond_sweep(rng, 120)]
    out += R.pivot_sweep(rng, 20)
    out += R.qr_swap_sweep(rng, 20)
    base = R.cond_sweep(np.random.default_rng(12), 6, cond_max=1e3)
    for j in range(-40, 41, 8):
        out += [((H.astype(np.float64) * 2.0 ** j).astype(F), g) for H, g in base]
    out += [(H, g) for H, g, _ in R.rank_edge_cases()]
    return out


@pytest.fixture(scope="module")
def near():
    return R.near_threshold_sweep()


def test_rank6_div_equals_the_oracle_on_every_sweep_matrix(oracle_mod, near):
    L = oracle_mod.lib()
    mats = [R.damped(H, F(lam)) for H, _, _, lam in near]
    for k in (0, 3, 6):
        mats += [R.damped(H, F(R.device_lambda(k))) for H, _ in _all_sweeps()]
    M = np.stack(mats)
    got = R.rank6_f32(M, "div")
    want = np.array([_oracle_rank(L, m) for m in M])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])


def test_float64_lu_and_inverse_reproduce_the_oracle(oracle_mod):
    """The oracle's float32 inverse (gn::inverse6, the division form) lies within the first-order bound of the float64 LU:
    |X - H^-1| <= 21 u |H^-1| P^T|L||U| |H^-1| (the column bound of update_bound's docstring, the update's rounding left out)."""
    L = oracle_mod.lib()
    rng = np.random.default_rng(3)
    cases = R.cond_sweep(rng, 150, cond_max=1e5) + R.pivot_sweep(rng, 20)
    worst = 0.0
    for H, _ in cases:
        st, X = _oracle_inverse(L, H)
        assert st == 0
        H64 = H.astype(np.float64)
        Lf, Uf, perm, _ = R.lu64(H64)
        P = np.eye(6)[perm]
        assert np.allclose(P @ H64, Lf @ Uf, rtol=0, atol=1e-12 * np.abs(H64).max())
        Hi = np.linalg.inv(H64)
        bound = 21 * R.U32 * (np.abs(Hi) @ (P.T @ (np.abs(Lf) @ np.abs(Uf))) @ np.abs(Hi))
        err = np.abs(X.astype(np.float64) - Hi)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= 3 * bound), float((err / bound).max())
        # the float32 restatement of the division form is the oracle bit for bit
        Xr, ok = R.inverse6_f32(H, "div")
        assert ok and np.array_equal(Xr.view(np.uint32), X.view(np.uint32))
    print(f"inverse: worst error / first-order bound {worst:.3f}")


def test_pivot_sweep_swaps_rows_at_every_step():
    for H, _ in R.pivot_sweep(np.random.default_rng(5), 10):
        _, _, _, piv = R.lu64(H)
        assert all(piv[k] != k for k in range(5)), piv
        assert np.array_equal(H, H.T)
        assert np.all(np.linalg.eigvalsh(H.astype(np.float64)) > 0)


def test_mpmath_rodrigues_matches_the_oracle(oracle_mod):
    L = oracle_mod.lib()
    rng = np.random.default_rng(9)
    angles = [0.0, R.ROT_THRESHOLD * (1 - 2 ** -20), R.ROT_THRESHOLD, R.ROT_THRESHOLD * (1 + 2 ** -20), 1e-8, 1e-3, 0.49, 0.5,
              0.51, 1.0, 2.0, 3.1, math.pi, 3.5]
    for a in angles:
        for _ in range(4):
            d = rng.normal(size=3)
            w = d / np.linalg.norm(d) * a
            v = np.concatenate([rng.normal(size=3), w]).astype(F).astype(np.float64)
            E = np.zeros(16)
            L.oracle_se3_pseudo_exp(np.ascontiguousarray(v).ctypes.data_as(C.c_void_p), E.ctypes.data_as(C.c_void_p))
            E = E.reshape(4, 4).T
            wn = float(np.linalg.norm(v[3:]))
            if wn < R.ROT_THRESHOLD:      # below the threshold the oracle (and the device) apply no rotation at all
                assert np.array_equal(E[:3, :3], np.eye(3))
                assert np.abs(R.pseudo_exp_mp(v) - E).max() <= 2 * wn
                continue
            assert np.abs(R.pseudo_exp_mp(v) - E).max() <= 1e-15, (a, np.abs(R.pseudo_exp_mp(v) - E).max())
            assert np.array_equal(E[:3, 3], v[:3])


def test_mat4_mul_f32_is_the_oracle_gn_step_product(oracle_mod):
    """gn_step's candidate pose is mat4_mul(float(E), pose): for a zero rotation E is exact, and the emulation equals it bit for bit."""
    rng = np.random.default_rng(4)
    for _ in range(20):
        pose = np.eye(4, dtype=F)
        pose[:3, :3] = np.asarray(R.pseudo_exp_mp(np.concatenate([[0, 0, 0], rng.normal(size=3)]))[:3, :3], F)
        pose[:3, 3] = rng.normal(size=3).astype(F)
        g = rng.normal(size=6).astype(F)
        g[3:] = 0
        H = np.diag([4.0, 0.5, 2.0, 8.0, 1.0, 0.25]).astype(F)
        st, cand, upd = oracle_mod.gn_step(H, g, 1.0, pose)
        assert st == 0
        E = np.eye(4, dtype=F)
        E[:3, 3] = upd[:3]
        assert np.array_equal(cand, R.mat4_mul_f32(E, pose))


def test_update_emulation_matches_the_oracle_step(oracle_mod):
    """update_f32(., "div") is the oracle's gn_step update bit for bit (same operations, same order)."""
    rng = np.random.default_rng(21)
    for H, g in R.cond_sweep(rng, 40, cond_max=1e5) + R.pivot_sweep(rng, 10):
        st, _, upd = oracle_mod.gn_step(H, g, 1.0, np.eye(4))
        assert st == 0
        assert np.array_equal(R.update_f32(H, g, "div").view(np.uint32), upd.view(np.uint32))


@pytest.mark.parametrize("method", [0, 1, 2])
def test_bookkeeping_restatement_reproduces_the_oracle_trace(oracle_mod, small_pair, method):
    """Replays ora.trace() (the errors every pass produced and the updates every step took) through decide(): the same passes are
    accepted, the same step is the last of its level."""
    (rgbA, dA), (rgbB, dB), _ = small_pair
    ora = oracle_mod.Oracle(n_pyr=3, math_mode=1, reduce_mode=1)
    ora.set_target(rgbA, dA)
    ora.set_source(rgbB, dB)
    st_o, _ = ora.align360(np.eye(4), method)
    assert st_o == 0
    tr = ora.trace()
    i = 0
    n_acc = 0
    while i < len(tr):
        level = tr[i]["level"]
        assert tr[i]["it"] == -1
        st = R.SolveState(level=level)
        take, go, _ = R.decide(st, tr[i]["error"], float(tr[i]["n_valid"]), 10, 1e-3, 1e-4, 0)
        assert take == 1
        i += 1
        while go:
            assert i < len(tr) and tr[i]["level"] == level and tr[i]["it"] == st.it, (i, level, st.it)
            st.update = tr[i]["update"]
            take, go, _ = R.decide(st, tr[i]["new_error"], float(tr[i]["n_valid"]), 10, 1e-3, 1e-4, 0)
            assert (take == 2) == bool(tr[i]["accepted"]), (i, take, tr[i])
            n_acc += take == 2
            i += 1
        assert i == len(tr) or tr[i]["it"] == -1, (i, tr[i])
        assert st.iters == ora.result.iters[level]
    assert n_acc == sum(ora.result.iters[:3])


def test_sweep_is_sensitive_to_the_quotient_form(near):
    """The committed seed holds matrices on which the division and the reciprocal form of the rank test disagree, and enough of
    each verdict for the device comparison to mean something."""
    M = np.stack([R.damped(H, F(lam)) for H, _, _, lam in near])
    rd, rr = R.rank6_f32(M, "div"), R.rank6_f32(M, "rcp")
    n_dis = int(((rd == 6) != (rr == 6)).sum())
    print(f"near-threshold sweep: {len(near)} matrices, {int((rd == 6).sum())} full rank, {int((rd != 6).sum())} rank-deficient, "
          f"{n_dis} on which div and rcp disagree")
    assert len(near) >= 4000
    assert n_dis >= 1
    assert (rd == 6).sum() >= 50 and (rd != 6).sum() >= 50


def test_scale_safe_range_is_wide_and_proven_by_emulation():
    rng = np.random.default_rng(13)
    for H, g in R.cond_sweep(rng, 10, cond_max=1e3):
        safe = [j for j in range(-40, 41) if R.scale_safe(H, g, j)]
        assert len(safe) >= 41, safe
