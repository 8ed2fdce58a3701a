"""CPU references for the serial Gauss-Newton step of the spherical path (RPI.h:4599-4722; gn_math.h, photo_icp_kernels.h
qr_rank6_lanes / lu_inverse6_lanes / solve_waves / solve_finish: one form, run by k_solve / k_solve_b and by the fused launches alike;
the bits of the form k_solve ran before it are recorded in tests/golden/solve_bits.json, cases in tests/solve_cases.py).  No GPU needed.

- rank6_f32: (H + lambda diag H).rank() restated operation for operation in float32 (batched numpy, IEEE per element, no
  contraction), with the Householder quotients as divisions ("div": gn::rank6, the oracle, Eigen) or as products with a correctly
  rounded reciprocal ("rcp").
- inverse6_f32 / update_f32: the 6x6 partial-pivot LU inverse and update = (-H^-1) g in float32, in the same two quotient forms.
- lu64: float64 partial-pivot LU (scipy) with the pivot sequence; update_bound: the a-priori error bound of the float32 update.
- rodrigues_mp: Rodrigues' rotation in mpmath; mat4_mul_f32: the ((a0 + a1) + a2) + a3 product of gn::mat4_mul.
- SolveState / solve_step: the accept / stop bookkeeping of one solve launch.
- Seeded sweep generators of float32 normal equations (H32 = (float) of a float64 total, like the device's cast of its sums).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace

import mpmath
import numpy as np
import scipy.linalg

F = np.float32
EPS32 = F(1.1920929e-07)          # gn::kEpsF
U32 = 2.0 ** -24                  # unit roundoff of float32
ROT_THRESHOLD = 128 * 2.220446049250313e-16      # gn::se3_pseudo_exp: a rotation is applied when |w| >= 2^-45


def _seq_sum(terms, start=None):
    s = F(0) if start is None else start
    for t in terms:
        s = s + t
    return s


# ------------------------------------------------------------------------------------------------------------------------
# rank test (ColPivHouseholderQR::rank() with Eigen's thresholds)
# ------------------------------------------------------------------------------------------------------------------------
def rank6_f32(M, quotient: str = "div", with_swaps: bool = False):
    """Rank of each 6x6 float32 matrix M[..., r, c] as gn::rank6 computes it ("div") or with the two Householder quotients
    v[r] = A[r][k] / (c0 - beta) and tau = (beta - c0) / beta formed through a correctly rounded reciprocal ("rcp").
    with_swaps: also return, per matrix, whether a column swap ran."""
    assert quotient in ("div", "rcp")
    A = np.array(M, dtype=F, copy=True)
    single = A.ndim == 2
    if single:
        A = A[None]
    N = A.shape[0]
    idx = np.arange(N)
    with np.errstate(all="ignore"):
        colsq = np.zeros((N, 6), F)
        for c in range(6):
            colsq[:, c] = _seq_sum(A[:, r, c] * A[:, r, c] for r in range(6))
        maxcol = np.zeros(N, F)
        for c in range(6):
            maxcol = np.where(colsq[:, c] > maxcol, colsq[:, c], maxcol)
        helper = (maxcol * (EPS32 * EPS32)) / F(6)
        pivots = np.zeros((N, 6), F)
        maxpivot = np.zeros(N, F)
        nonzero = np.full(N, 6)
        stopped = np.zeros(N, bool)
        swapped = np.zeros(N, bool)
        for k in range(6):
            best = np.full(N, k)
            bestsq = np.full(N, F(-1))
            for c in range(k, 6):
                s = _seq_sum(A[:, r, c] * A[:, r, c] for r in range(k, 6))
                better = s > bestsq
                bestsq = np.where(better, s, bestsq)
                best = np.where(better, c, best)
            stop_now = ~stopped & (bestsq < helper * F(6 - k))
            nonzero = np.where(stop_now, k, nonzero)
            stopped |= stop_now
            act = ~stopped
            sw = act & (best != k)
            swapped |= sw
            if sw.any():
                n = idx[sw]
                colk, colb = A[n, :, k].copy(), A[n, :, best[sw]].copy()
                A[n, :, k], A[n, :, best[sw]] = colb, colk
            tail = _seq_sum((A[:, r, k] * A[:, r, k] for r in range(k + 1, 6)), np.zeros(N, F))
            c0 = A[:, k, k]
            zero = tail == F(0)
            beta = np.sqrt(c0 * c0 + tail)
            beta = np.where(c0 >= F(0), -beta, beta)
            beta = np.where(zero, c0, beta)
            den = c0 - beta
            v = np.zeros((N, 6), F)
            if quotient == "div":
                for r in range(k + 1, 6):
                    v[:, r] = A[:, r, k] / den
                tau = (beta - c0) / beta
            else:
                rden = F(1) / den
                for r in range(k + 1, 6):
                    v[:, r] = A[:, r, k] * rden
                tau = (beta - c0) * (F(1) / beta)
            v = np.where(zero[:, None], F(0), v)
            tau = np.where(zero, F(0), tau)
            v[:, k] = F(1)
            for c in range(k + 1, 6):
                dot = _seq_sum(v[:, r] * A[:, r, c] for r in range(k, 6))
                dot = dot * tau
                for r in range(k, 6):
                    A[:, r, c] = np.where(act, A[:, r, c] - dot * v[:, r], A[:, r, c])
            pivots[:, k] = np.where(act, beta, F(0))
            ab = np.abs(beta)
            maxpivot = np.where(act & (ab > maxpivot), ab, maxpivot)
        thr = maxpivot * (EPS32 * F(6))
        ks = np.arange(6)[None, :]
        rank = ((ks < nonzero[:, None]) & (np.abs(pivots) > thr[:, None])).sum(axis=1)
    if single:
        return (int(rank[0]), bool(swapped[0])) if with_swaps else int(rank[0])
    return (rank, swapped) if with_swaps else rank


def damped(H32, lam32):
    """H + lambda diag(H) as the device forms it: (float) entries, the diagonal as h + lambda * h in float32."""
    M = np.array(H32, dtype=F, copy=True)
    d = np.arange(6)
    with np.errstate(all="ignore"):
        M[..., d, d] = M[..., d, d] + F(lam32) * M[..., d, d]
    return M


def device_lambda(k: int, first: bool = True) -> float:
    """lambda after k accepted steps as the state holds it (double, repeated / 5.0); the rank test uses (float) of it (of
    lambda / 5.0 on a pass that follows an accepted step)."""
    lam = 1.0
    for _ in range(k):
        lam = lam / 5.0
    return lam


# ------------------------------------------------------------------------------------------------------------------------
# LU inverse and update
# ------------------------------------------------------------------------------------------------------------------------
def inverse6_f32(H, quotient: str = "div", track: bool = False):
    """M^-1 of one float32 6x6 matrix by partial-pivot LU as gn::inverse6 ("div") or lu_inverse6_lanes ("rcp": multipliers
    c_r * (1 / p) and back-substitution x = s * (1 / p), one correctly rounded reciprocal per pivot).  Returns (inv, ok[, (lo, hi,
    pivots)]): lo / hi = smallest non-zero / largest magnitude of any value formed, pivots = the six pivots."""
    LU = np.array(H, dtype=F, copy=True)
    perm = list(range(6))
    mags = []
    piv_vals = []
    with np.errstate(all="ignore"):
        for k in range(6):
            p, best = k, abs(LU[k, k])
            for r in range(k + 1, 6):
                if abs(LU[r, k]) > best:
                    best, p = abs(LU[r, k]), r
            if best == F(0):
                return (None, False, None) if track else (None, False)
            if p != k:
                LU[[k, p]] = LU[[p, k]]
                perm[k], perm[p] = perm[p], perm[k]
            piv_vals.append(LU[k, k])
            rk = F(1) / LU[k, k]
            mags.append(rk)
            for r in range(k + 1, 6):
                LU[r, k] = LU[r, k] / LU[k, k] if quotient == "div" else LU[r, k] * rk
                mags.append(LU[r, k])
                for c in range(k + 1, 6):
                    t = LU[r, k] * LU[k, c]
                    LU[r, c] = LU[r, c] - t
                    mags += [t, LU[r, c]]
        inv = np.zeros((6, 6), F)
        for col in range(6):
            y = np.zeros(6, F)
            for r in range(6):
                s = F(1) if perm[r] == col else F(0)
                for c in range(r):
                    t = LU[r, c] * y[c]
                    s = s - t
                    mags += [t, s]
                y[r] = s
            for r in range(5, -1, -1):
                s = y[r]
                for c in range(r + 1, 6):
                    t = LU[r, c] * y[c]
                    s = s - t
                    mags += [t, s]
                y[r] = s / LU[r, r] if quotient == "div" else s * (F(1) / LU[r, r])
                mags.append(y[r])
            inv[:, col] = y
    if not track:
        return inv, True
    a = np.abs(np.array(mags + list(np.ravel(H)), np.float64))
    nz = a[a > 0]
    return inv, True, (float(nz.min()) if nz.size else 0.0, float(a.max()), np.array(piv_vals, F))


def update_f32(H, g, quotient: str = "rcp"):
    """update = (-H^-1) g, row r summed in column order from 0 (RPI.h:4693; solve_wave1 / gn::step)."""
    inv, ok = inverse6_f32(H, quotient)
    if not ok:
        return None
    g = np.asarray(g, F)
    with np.errstate(all="ignore"):
        return np.array([_seq_sum((-inv[r, c]) * g[c] for c in range(6)) for r in range(6)], F)


def lu64(H):
    """Partial-pivot LU of H (float64): P H = L U.  Returns (L, U, perm, pivot_rows) with pivot_rows[k] = the row chosen at step
    k (LAPACK's sequence of interchanges)."""
    lu, piv = scipy.linalg.lu_factor(np.asarray(H, np.float64), check_finite=True)
    L = np.tril(lu, -1) + np.eye(6)
    U = np.triu(lu)
    perm = list(range(6))
    for k, p in enumerate(piv):
        perm[k], perm[p] = perm[p], perm[k]
    return L, U, perm, [int(p) for p in piv]


def update_bound(H32, g32):
    """Per-entry bound of |u_computed - u64| for the float32 update of a reciprocal-form (or division-form) LU inverse:
        64 u (|H^-1| P^T |L||U| |H^-1| |g|) + 8 u (|H^-1| |g|),     u = 2^-24,
    all in float64 from the LU of the float32 H.  Constants (first order in u; the test cases keep cond(H) u below 1e-2):
    the computed LU satisfies L^ U^ = P(H + dH0), |dH0| <= gamma_n |L^||U^| (n = 6; a reciprocal multiplier c * fl(1/p) adds one
    rounding, absorbed as gamma_2 |l||p|); each column of the inverse solves (L^ + dL)(U^ + dU) x = P e with |dL| <= gamma_n |L^| and
    |dU| <= gamma_{n+1} |U^| (one more rounding per row for s * fl(1/p)).  So x = (H + dH)^-1 e, |dH| <= (3n + 3) u P^T|L||U| = 21 u
    P^T|L||U|, and |X - H^-1| <= 21 u |H^-1| P^T|L||U| |H^-1| to first order.  update = fl(-X g) in column order adds gamma_6
    |X||g| <= 6.01 u |H^-1||g|.  64 and 8 leave a factor 3 (1.3) for the second-order terms and for |L^||U^| versus the float64
    factors."""
    H = np.asarray(H32, np.float64)
    g = np.asarray(g32, np.float64)
    Hi = np.linalg.inv(H)
    L, U, perm, _ = lu64(H)
    P = np.eye(6)[perm]
    LU_abs = P.T @ (np.abs(L) @ np.abs(U))
    aHi = np.abs(Hi)
    b = 64 * U32 * (aHi @ LU_abs @ aHi @ np.abs(g)) + 8 * U32 * (aHi @ np.abs(g))
    return b, Hi @ g * -1.0


def scale_safe(H32, g32, j: int) -> bool:
    """True when 2^j H, 2^j g give the same update bit for bit on the device: every value the reciprocal-form inverse and the update
    form stays a normal float32 after scaling by 2^j (products and sums scale exactly then), every pivot stays inside
    [2^-60, 2^60] (the range over which the device reciprocal is proven correctly rounded), and the float32 emulation confirms it."""
    inv, ok, (lo, hi, piv) = inverse6_f32(H32, "rcp", track=True)
    if not ok:
        return False
    g = np.abs(np.asarray(g32, np.float64))
    gnz = g[g > 0]
    # scale factors: H, U, pivots 2^j; multipliers and y 1; reciprocals, x, inverse 2^-j; products inv * g and the update 1
    s = 2.0 ** j
    lo_s, hi_s = min(lo * min(s, 1 / s), gnz.min() * min(s, 1.0) if gnz.size else 1.0), max(hi * max(s, 1 / s), g.max() * max(s, 1.0))
    if lo_s < 2.0 ** -126 or hi_s >= 2.0 ** 127:
        return False
    if np.any(np.abs(piv.astype(np.float64)) * s < 2.0 ** -60) or np.any(np.abs(piv.astype(np.float64)) * s > 2.0 ** 60):
        return False
    u0 = update_f32(H32, g32, "rcp")
    uj = update_f32(np.asarray(H32, F) * F(s), np.asarray(g32, F) * F(s), "rcp")
    return uj is not None and np.array_equal(u0.view(np.uint32), uj.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------
# SE(3) pseudo-exponential and the pose product
# ------------------------------------------------------------------------------------------------------------------------
def rodrigues_mp(w, dps: int = 40):
    """R = I + sin(a)/a W + (1 - cos a)/a^2 W^2 (W = skew(w), a = |w|) in mpmath at `dps` digits, w taken as float64 (the float32
    update cast to double, RPI.h:4696).  Returns a 3x3 list of mpf."""
    with mpmath.workdps(dps):
        wx, wy, wz = (mpmath.mpf(float(x)) for x in w)
        a2 = wx * wx + wy * wy + wz * wz
        W = [[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]]
        R = [[mpmath.mpf(1 if i == j else 0) for j in range(3)] for i in range(3)]
        if a2 == 0:
            return R
        a = mpmath.sqrt(a2)
        sa, cb = mpmath.sin(a) / a, (1 - mpmath.cos(a)) / a2
        for i in range(3):
            for j in range(3):
                w2 = sum(W[i][k] * W[k][j] for k in range(3))
                R[i][j] = R[i][j] + sa * W[i][j] + cb * w2
        return R


def pseudo_exp_mp(v, dps: int = 40):
    """4x4 [Rodrigues(v[3:6]) v[0:3]; 0 0 0 1] as float64 (entries of the mpmath result rounded once)."""
    R = rodrigues_mp(v[3:6], dps)
    E = np.eye(4)
    for i in range(3):
        for j in range(3):
            E[i, j] = float(R[i][j])
        E[i, 3] = float(v[i])
    return E


def pseudo_exp_f32_mp(v, dps: int = 40):
    """float32 of the exact pseudo-exponential (each entry rounded once from the mpmath value)."""
    R = rodrigues_mp(v[3:6], dps)
    E = np.eye(4, dtype=F)
    for i in range(3):
        for j in range(3):
            with mpmath.workdps(dps):
                E[i, j] = F(float(R[i][j]))     # double first: one rounding to 53 bits cannot move a float32 rounding but at a tie
        E[i, 3] = F(v[i])
    return E


def mat4_mul_f32(A, B):
    """gn::mat4_mul: C[r, c] = ((A[r,0] B[0,c] + A[r,1] B[1,c]) + A[r,2] B[2,c]) + A[r,3] B[3,c] in float32 (row-major 4x4 in)."""
    A = np.asarray(A, F)
    B = np.asarray(B, F)
    C = np.zeros((4, 4), F)
    for c in range(4):
        for r in range(4):
            C[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return C


# ------------------------------------------------------------------------------------------------------------------------
# bookkeeping of one solve launch (RPI.h:4599-4722 as solve_waves / solve_finish implement it)
# ------------------------------------------------------------------------------------------------------------------------
@dataclass
class SolveState:
    level: int
    pose: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=F))
    cand: np.ndarray = None
    update: np.ndarray = field(default_factory=lambda: np.ones(6, F))
    lam: float = 1.0
    error: float = 0.0
    new_error: float = 0.0
    diff_error: float = 0.0
    first: int = 1
    it: int = 0
    iters: int = 0
    status: int = 0
    done: int = 0
    n_evals: int = 0

    def __post_init__(self):
        self.pose = np.asarray(self.pose, F).copy()
        self.cand = self.pose.copy() if self.cand is None else np.asarray(self.cand, F).copy()
        self.update = np.asarray(self.update, F).copy()
        self.level_active = self.level


def error_of(e2p, e2d, n_p, n_d, occ: int) -> float:
    """sqrt((E2P + E2D) / (NP + ND)) (RPI.h:2738), or sqrt(E2P / NP) + sqrt(E2D / ND) in the occlusion modes; 0/0 -> NaN."""
    with np.errstate(all="ignore"):
        if occ == 0:
            return float(np.sqrt(np.float64(e2p + e2d) / np.float64(n_p + n_d)))
        return float(np.sqrt(np.float64(e2p) / np.float64(n_p)) + np.sqrt(np.float64(e2d) / np.float64(n_d)))


def decide(st: SolveState, new_error: float, nvalid: float, max_iters: int, tol_residual: float, tol_update: float, forced: int):
    """The scalar decisions of one pass (solve_bookkeeping_wave, wave 0 of solve_waves).  Mutates st; returns (take, go, lam32) -- take 2: the candidate
    was accepted (pose := cand), go: a step is computed, lam32: the damping of its rank test."""
    lam32 = F(st.lam if st.first else st.lam / 5.0)
    st.n_evals += 1
    st.new_error = new_error
    take, go, stop = 0, False, False
    if st.first:
        st.first = 0
        if nvalid == 0.0 or new_error != new_error:
            st.status, st.done, stop = 2, 1, True
        else:
            st.error = st.diff_error = new_error
            take = 1
    else:
        diff = st.error - new_error
        st.diff_error = diff
        if forced or diff > tol_residual:
            st.lam = st.lam / 5.0
            st.error = new_error
            st.it += 1
            st.iters = st.it
            take = 2
    if not stop:
        un = float(np.sqrt(_seq_sum(st.update[i] * st.update[i] for i in range(6))))
        go = bool(forced or (st.it < max_iters and un > tol_update and st.diff_error > tol_residual))
        if not go:
            st.done = 1
    if take == 2:
        st.pose = st.cand.copy()
    return take, go, lam32


def finish(st: SolveState, go: bool, ill: bool, cand_new, update_new, forced: int):
    """solve_finish: commit the step or ILL-POSED; a finished level > 0 hands over to the next finer one."""
    if go:
        if ill:
            st.status, st.done = 1, 1
        else:
            st.cand = np.asarray(cand_new, F).copy()
            st.update = np.asarray(update_new, F).copy()
    if not forced and st.level_active > 0 and st.done and st.status == 0:
        st.cand = st.pose.copy()
        st.update = np.ones(6, F)
        st.level_active -= 1
        st.lam, st.it, st.first, st.done = 1.0, 0, 1, 0
        st.error = st.new_error = st.diff_error = 0.0


def solve_step(st: SolveState, H32, g32, e2p, e2d, n_p, n_d, *, occ=0, max_iters=10, tol_residual=1e-3, tol_update=1e-4, forced=0):
    """One whole solve launch on the normal equations H32, g32 and the error sums, with the step in the device's arithmetic where
    it can be stated exactly: the rank test and the reciprocal-form update in float32, the exponential exact for a zero rotation
    (cases with a rotation compare the candidate pose separately).  Returns a new state."""
    st = replace(st, pose=st.pose.copy(), cand=st.cand.copy(), update=st.update.copy())
    st.level_active = st.level
    take, go, lam32 = decide(st, error_of(e2p, e2d, n_p, n_d, occ), float(n_p + n_d), max_iters, tol_residual, tol_update, forced)
    cand_new = upd = None
    ill = False
    if go:
        ill = rank6_f32(damped(H32, lam32), "div") != 6
        upd = update_f32(H32, g32, "rcp")
        ill = ill or upd is None
        if not ill:
            assert not np.any(upd[3:]), "solve_step states the exponential exactly only for a zero rotation"
            E = np.eye(4, dtype=F)
            E[:3, 3] = upd[:3]
            cand_new = mat4_mul_f32(E, st.cand)
    finish(st, go, ill, cand_new, upd, forced)
    return st


# ------------------------------------------------------------------------------------------------------------------------
# the partial row the device sums (rgbd360_debug_solve_partials / _state)
# ------------------------------------------------------------------------------------------------------------------------
def partial_row(H, g, e2=(3.0, 2.0), n=(1000, 800, 1500)) -> np.ndarray:
    """32 float64: the 21 upper-triangle terms of H (slot a*(13-a)/2 + (b-a)), g, E2 photo / depth, N photo / depth / visible."""
    H = np.asarray(H, np.float64)
    row = np.zeros(32)
    for a in range(6):
        for b in range(a, 6):
            row[(a * (13 - a)) // 2 + (b - a)] = H[a, b]
    row[21:27] = np.asarray(g, np.float64)
    row[27:29] = e2
    row[29:32] = n
    return row


# ------------------------------------------------------------------------------------------------------------------------
# seeded sweeps
# ------------------------------------------------------------------------------------------------------------------------
def _orth(rng):
    q, r = np.linalg.qr(rng.normal(size=(6, 6)))
    return q * np.sign(np.diag(r))


def spd(rng, s, scale=1.0):
    """float32 (the device's (float) of a float64 total) of scale * Q diag(s) Q^T; symmetric by construction."""
    Q = _orth(rng)
    H = (Q * np.asarray(s, np.float64)) @ Q.T
    H = 0.5 * (H + H.T) * scale
    return H.astype(F)


def rhs_for(rng, H32, mag=1e-3):
    """g = (float)(H u) for a random u of norm ~mag: the update stays near -u, a pose a pass can be evaluated at."""
    u = rng.normal(size=6)
    u *= mag / np.linalg.norm(u)
    return (np.asarray(H32, np.float64) @ u).astype(F)


def cond_sweep(rng, n, cond_max=1e7):
    out = []
    for _ in range(n):
        c = 10.0 ** rng.uniform(0, math.log10(cond_max))
        s = np.sort(10.0 ** rng.uniform(-math.log10(c), 0, size=6))[::-1]
        s[0], s[-1] = 1.0, 1.0 / c
        H = spd(rng, s, scale=10.0 ** rng.uniform(-3, 4))
        out.append((H, rhs_for(rng, H)))
    return out


def pivot_sweep(rng, n):
    """SPD matrices on which partial pivoting swaps rows at every step k = 0..4 (D B D: B a correlation-heavy SPD matrix, D growing
    down the diagonal, so that a lower row outweighs the diagonal in every column).  Asserted from the float64 pivot sequence."""
    out = []
    while len(out) < n:
        s = np.sort(10.0 ** rng.uniform(-4, 0, size=6))[::-1]
        B = spd(rng, s).astype(np.float64)
        d = 10.0 ** np.sort(rng.uniform(-1, 1, size=6))[rng.permutation(6)]
        H = (B * d[:, None] * d[None, :]).astype(F)
        H = np.triu(H) + np.triu(H, 1).T
        _, _, _, piv = lu64(H)
        if all(piv[k] != k for k in range(5)) and np.linalg.cond(H.astype(np.float64)) < 1e5:
            out.append((H, rhs_for(rng, H)))
    return out


def qr_swap_sweep(rng, n):
    """Matrices on which the rank test's column pivoting swaps columns (a large column behind a small one)."""
    out = []
    while len(out) < n:
        s = 10.0 ** rng.uniform(-3, 0, size=6)
        H = spd(rng, s, scale=10.0 ** rng.uniform(-2, 2))
        if rank6_f32(damped(H, F(1.0)), with_swaps=True)[1]:
            out.append((H, rhs_for(rng, H)))
    return out


def near_threshold_sweep(seed=20261016, n_per_k=400, ks=range(12)):
    """(H32, g32, k, lambda_double) with sigma_min / sigma_max in [1e-8, 1e-5] (log-uniform) and lambda = 5^-k as the device forms it:
    the matrices on which (H + lambda diag H).rank() hangs on a pivot near Eigen's threshold."""
    rng = np.random.default_rng(seed)
    out = []
    for k in ks:
        for _ in range(n_per_k):
            r = 10.0 ** rng.uniform(-8, -5)
            s = np.concatenate([[1.0], 10.0 ** rng.uniform(-3, 0, size=4), [r]])
            H = spd(rng, s, scale=10.0 ** rng.uniform(-1, 3))
            out.append((H, rhs_for(rng, H, 1e-4), k, device_lambda(k)))
    return out


def rank_edge_cases():
    """An exact zero LU pivot, and entries whose squared column norms overflow / underflow float32 (2^j scaling)."""
    rng = np.random.default_rng(7)
    out = []
    H = np.diag([1.0, 1.0, 1.0, 0.0, 1.0, 1.0]).astype(F)              # zero pivot, rank 5
    out.append((H, np.array([0.3, -0.2, 0.1, 0.05, -0.04, 0.02], F), "zero pivot"))
    B = spd(rng, [1, 0.5, 0.3, 0.2, 0.1, 0.05])
    B2 = np.array(B, F)
    B2[:, 5] = B2[:, 4]
    B2[5, :] = B2[4, :]                                                  # exactly singular, every LU pivot but the last non-zero
    out.append((B2, rhs_for(rng, B2), "duplicate row"))
    for j in (-90, -80, -76, -70, 62, 64, 66, 70):
        for base in (B, spd(rng, [1, 1e-3, 1e-5, 1e-6, 1e-7, 1e-8])):
            Hs = (base.astype(np.float64) * 2.0 ** j).astype(F)
            out.append((Hs, (rhs_for(rng, base).astype(np.float64) * 2.0 ** j).astype(F), f"2^{j}"))
    return out
