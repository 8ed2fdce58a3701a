"""The hand-made solve cases of tests/test_fused_solve_shape.py and tests/test_gn_solve_exact.py in one place, and the recorded bits
of their states: tests/golden/solve_bits.json (tools/solve_bits.py records it, the two tests compare with it).

A case is a dict: `name`, `level`, `row` (the 32 float64 of gn_reference.partial_row) and `kw` (the further arguments of
RegisterPhotoICP.debug_solve_state), plus whatever the test that owns the group asserts on (H, g, u, ...).  Everything comes from
seeds and constants.  No GPU needed here."""
from __future__ import annotations

import json
import math
import os

import numpy as np

import gn_reference as R

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_bits.json")
KEYS_I = ("status", "done", "level_active", "it", "n_evals", "pend_nb", "iters")
KEYS_F64 = ("lam", "error", "new_error", "diff_error")
KEYS_F32 = ("cand", "pose", "update")


def step_row(H, g):
    return R.partial_row(H, g, e2=(3.0, 2.0), n=(1000, 800, 1500))


def _case(name, row, level=0, kw=None, **more):
    return dict(name=name, level=level, row=row, kw=dict(kw or {}), **more)


# ------------------------------------------------------------------------------------------------------------------------
# tests/test_fused_solve_shape.py
# ------------------------------------------------------------------------------------------------------------------------
def dominant(rng):
    """symmetric, strictly diagonally dominant float32: no step of the elimination swaps"""
    A = rng.uniform(-0.1, 0.1, size=(6, 6))
    H = 0.5 * (A + A.T) + np.diag(rng.uniform(4.0, 8.0, size=6))
    return H.astype(F)


def pivot_cases():
    """21 cases (k, p): a symmetric H on which steps 0 .. k-1 take their diagonal entry and step k takes row p (p = k: no swap at all)."""
    rng = np.random.default_rng(20261020)
    hs = []
    for k in range(6):
        for p in range(k, 6):
            H = dominant(rng)
            if p != k:
                H[k, p] = H[p, k] = F(3.0) * H[k, k]      # column k below the diagonal: row p outweighs the diagonal entry
            hs.append((k, p, H))
    rng = np.random.default_rng(7)
    out = []
    for k, p, H in hs:
        g = R.rhs_for(rng, H, mag=1e-3)
        out.append(_case("shape/pivot: step %d takes row %d" % (k, p), step_row(H, g), k=k, p=p, H=H, g=g))
    return out


def deficient_cases():
    """A zero pivot (ILL-POSED by the inverse) and a rank-3 matrix, on its first pass and undamped (ILL-POSED by the rank test alone)."""
    rng = np.random.default_rng(11)
    H = dominant(rng)
    H[2, :] = 0
    H[:, 2] = 0                                    # column 2 is zero when step 2 looks for its pivot
    g = R.rhs_for(rng, dominant(rng))
    B = rng.normal(size=(6, 3))
    H3 = (B @ B.T).astype(F)                        # rank 3: the pivots behind the third are rounding noise, none is zero
    H3 = np.triu(H3) + np.triu(H3, 1).T
    return [_case("shape/zero pivot", step_row(H, g)),
            _case("shape/rank 3, first pass", step_row(H3, g)),
            _case("shape/rank 3, undamped", step_row(H3, g), kw=dict(first=0, it=1, error=10.0, lam=0.0, update=(1e-2,) * 6))]


def exponential_arm_cases():
    """H = I: the inverse is exact and the update is -g, so g = -u hands the exponential exactly u.  11 rotation vectors: angle^2 just
    below, at and just above 0.25, around the no-rotation threshold, none, and an everyday one."""
    half = F(0.5)
    thr = R.ROT_THRESHOLD
    below, above = np.nextafter(half, F(0)), np.nextafter(half, F(1))
    out = []
    for n, w in enumerate(([below, 0, 0], [half, 0, 0], [above, 0, 0],                         # angle^2 just below, at and just above 0.25
                           [0.3, -0.3, 0.26], [0.2, 0.3, -0.35],                               # ... with all three components (0.2476, 0.2525)
                           [thr * 0.5, 0, 0], [0, thr * 0.99, 0], [0, 0, thr * 1.01], [thr * 2, thr, 0],      # around the no-rotation threshold
                           [0, 0, 0], [0.01, -0.02, 0.03])):
        u = np.array([1e-3, -2e-3, 3e-3] + list(w), np.float64).astype(F)
        out.append(_case("shape/exponential arm %d" % n, step_row(np.eye(6, dtype=F), -u), w=w, u=u))
    return out


STATE_TURN_ERROR = math.sqrt(5.0 / 1800.0)      # the error of step_row's sums


def state_turn_cases():
    """The state machine's six turns, in the order test_state_machine_turns asserts on them."""
    rng = np.random.default_rng(5)
    H = dominant(rng)
    g = R.rhs_for(rng, H, mag=1e-3)
    row = step_row(H, g)
    e = STATE_TURN_ERROR
    pose = np.eye(4)
    pose[:3, 3] = (0.01, -0.02, 0.03)
    small = (1e-2,) * 6
    return [_case("shape/turn: first pass", row, kw=dict(pose=pose, first=1)),
            _case("shape/turn: accepted", row, kw=dict(pose=pose, first=0, it=2, error=e + 0.5, lam=0.2, update=small)),
            _case("shape/turn: accepted, budget spent", row, kw=dict(pose=pose, first=0, it=9, error=e + 0.5, max_iters=10, update=small)),
            _case("shape/turn: rejected", row, kw=dict(pose=pose, first=0, it=2, error=e - 1e-3, update=small)),
            _case("shape/turn: rejected on level 1", row, level=1, kw=dict(pose=pose, first=0, it=2, error=e - 1e-3, update=small)),
            _case("shape/turn: accepted, small update", row, kw=dict(pose=pose, first=0, it=2, error=e + 0.5, update=(1e-6,) * 6))]


# ------------------------------------------------------------------------------------------------------------------------
# tests/test_gn_solve_exact.py
# ------------------------------------------------------------------------------------------------------------------------
def pseudo_exp_cases():
    """H = 2^3 I makes the update exactly -g / 8.  Thirteen rotation vectors (ten angles on seeded axes, three at the threshold of
    gn::se3_pseudo_exp and one float32 step on either side), each from the identity and from another pose `P`."""
    rng = np.random.default_rng(44)
    thr = R.ROT_THRESHOLD
    angles = [0.0, 1e-8, 0.49, 0.5, 0.51, 1.0, 2.0, 3.1, math.pi, 3.5]
    axis_cases = [np.array([thr, 0, 0]), np.array([0, np.nextafter(F(thr), F(0)), 0]), np.array([0, 0, np.nextafter(F(thr), F(1))])]
    P = np.eye(4, dtype=F)
    P[:3, :3] = np.asarray(R.pseudo_exp_mp(np.array([0, 0, 0, 0.3, -0.2, 0.5]))[:3, :3], F)
    P[:3, 3] = F([0.4, -1.5, 2.25])
    ws = []
    for a in angles:
        d = rng.normal(size=3)
        ws.append(d / np.linalg.norm(d) * a)
    ws += axis_cases
    kexp = 3
    H = np.eye(6) * 2.0 ** kexp
    out = []
    for n, w in enumerate(ws):
        u = np.concatenate([rng.normal(size=3) * 0.1, w]).astype(F)
        g = (-u.astype(np.float64) * 2.0 ** kexp)
        for at, pose in (("identity", np.eye(4, dtype=F)), ("P", P)):
            out.append(_case("exact/pseudo-exponential %d at %s" % (n, at), step_row(H, g), kw=dict(pose=pose), w=w, u=u, at_P=at == "P", P=P))
    return out


def bookkeeping_settings():
    """(H, g, {name: settings}) of the bookkeeping cases: the state, the termination settings, the error form and the row's sums."""
    H = np.diag([4.0, 5.0, 6.0, 7.0, 8.0, 9.0])
    g = np.array([0.3, -0.2, 0.1, 0.0, 0.0, 0.0])
    P = np.eye(4, dtype=F)
    P[:3, :3] = np.asarray(R.pseudo_exp_mp(np.array([0, 0, 0, -0.1, 0.25, 0.05]))[:3, :3], F)
    P[:3, 3] = F([0.2, 0.1, -0.3])
    tol = 2.0 ** -10
    ok_sums = dict(e2=(3000.0, 5000.0), n=(1200, 800, 1500))      # error sqrt(8000 / 2000) = 2 exactly
    upd = F([0.01, -0.02, 0.005, 0.001, 0.0, 0.002])
    base = dict(pose=P, update=upd, lam=0.04, error=2.0 + 0.5, first=0, it=3, max_iters=10, tol_residual=tol, tol_update=1e-4,
                forced=0, occlusion=0, level=0, **ok_sums)
    cases = {
        "first pass": dict(base, first=1, lam=1.0, it=0, error=0.0),
        "accept": base,
        "diff equals tol": dict(base, error=2.0 + tol),
        "diff one ulp above tol": dict(base, error=np.nextafter(2.0 + tol, 3.0)),
        "reject": dict(base, error=2.0 - 0.25),
        "it = max_iters - 1": dict(base, it=9),
        "it = max_iters - 2": dict(base, it=8),
        "it = max_iters": dict(base, it=10),
        "|update| = tol_update": dict(base, update=F([2.0 ** -12, 0, 0, 0, 0, 0]), tol_update=2.0 ** -12),
        "|update| one ulp above": dict(base, update=F([np.nextafter(F(2.0 ** -12), F(1)), 0, 0, 0, 0, 0]), tol_update=2.0 ** -12),
        "forced, rejected diff": dict(base, error=1.0, forced=1),
        "occ 1, depth empty, first": dict(base, first=1, lam=1.0, it=0, occlusion=1, e2=(3000.0, 0.0), n=(1200, 0, 1500)),
        "occ 2, photo empty, first": dict(base, first=1, lam=1.0, it=0, occlusion=2, e2=(0.0, 5000.0), n=(0, 800, 1500)),
        "occ 1, depth sum without count, first": dict(base, first=1, lam=1.0, it=0, occlusion=1, e2=(3000.0, 7.0), n=(1200, 0, 1500)),
        "occ 2, depth empty, later": dict(base, occlusion=2, e2=(3000.0, 0.0), n=(1200, 0, 1500)),
        "occ 1, both present": dict(base, occlusion=1, error=9.0),
        "NaN, first": dict(base, first=1, lam=1.0, it=0, e2=(float("nan"), 5000.0)),
        "NaN, later": dict(base, e2=(float("nan"), 5000.0)),
        "no residuals, first": dict(base, first=1, lam=1.0, it=0, n=(0, 0, 0), e2=(0.0, 0.0)),
        "level 1 finished: handover": dict(base, level=1, error=2.0 - 0.25),
        "level 1 accepted": dict(base, level=1),
        "level 1 at the iteration limit: handover": dict(base, level=1, it=9),
        "level 1 forced at the limit": dict(base, level=1, it=9, forced=1),
    }
    return H, g, cases


def bookkeeping_cases():
    H, g, cases = bookkeeping_settings()
    out = []
    for name, c in cases.items():
        kw = {k: c[k] for k in ("pose", "update", "lam", "error", "first", "it", "max_iters", "tol_residual", "tol_update", "forced", "occlusion")}
        out.append(_case("exact/bookkeeping: " + name, R.partial_row(H, g, e2=c["e2"], n=c["n"]), level=c["level"], kw=kw, label=name, c=c))
    return H, g, out


def rank_edge_cases():
    """gn_reference.rank_edge_cases() at the damping of a level's first pass (k = 0) and behind six accepted steps (k = 6)."""
    out = []
    for n, (H, g, label) in enumerate(R.rank_edge_cases()):
        for k in (0, 6):
            lam = R.device_lambda(k)
            out.append(_case("exact/rank edge %d (%s), lambda 5^-%d" % (n, label, k), step_row(H, g), kw=dict(lam=lam), H=H, g=g, label=label, k=k, lam=lam))
    return out


def all_cases():
    """Every case the fixture holds, in recording order."""
    return (pivot_cases() + deficient_cases() + exponential_arm_cases() + state_turn_cases() + pseudo_exp_cases() + bookkeeping_cases()[2] +
            rank_edge_cases())


# ------------------------------------------------------------------------------------------------------------------------
# the recorded form of a state
# ------------------------------------------------------------------------------------------------------------------------
def encode(state):
    """What debug_solve_state returns, every key of it, in the fixture's form: integers as they are, floats as the hex of their bytes."""
    rec = {k: int(state[k]) for k in KEYS_I}
    rec.update({k: np.float64(state[k]).tobytes().hex() for k in KEYS_F64})
    rec.update({k: np.ascontiguousarray(state[k], F).tobytes().hex() for k in KEYS_F32})
    assert sorted(rec) == sorted(state), sorted(state)
    return rec


def load_recorded():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def differences(state, recorded, skip=()):
    """The keys on which a state differs from its recorded bits."""
    got = encode(state)
    return ["%s: recorded %s, computed %s" % (k, recorded.get(k), got.get(k)) for k in sorted(set(got) | set(recorded))
            if k not in skip and got.get(k) != recorded.get(k)]
