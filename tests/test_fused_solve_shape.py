"""The fused launches' solve path (solve_waves_ft: wave 1's common case as fall-through code) against the two-launch route's
(k_solve keeps solve_waves as it was): the same hand-made partial row and state through rgbd360_debug_solve_state on route 0 (k_solve, the
old code) and on routes 1 and 2 (the prologue of k_eval_fs, the new code), and every word the solve decides -- candidate pose, pose,
update, status, done, iteration counts, level, damping, errors -- compared BIT FOR BIT.  The cases are the paths the reshaped code lays
out differently: every pivot choice at every elimination step (the swap arms lie behind the path now, taken by a second elimination),
a zero pivot, a rank-deficient H, the exponential's arms on both sides of angle^2 = 0.25 and of the no-rotation threshold, and the
state machine's turns (first pass of a level, accepted and rejected step, level hand-over).

Frames: 256 x 128 for routes 0 and 1.  Route 2 places the row at block row 40 of the table and needs a level with more than 40 block
rows; 256 x 128 has 32 at most, so route 2 runs on a 1024 x 512 pair (whose level 1, for the hand-over, still has 128).  Route 0 is run
on both pairs and must agree with itself."""
import math

import numpy as np
import pytest

import gn_reference as R
from rgbd360_amd import synth

pytestmark = pytest.mark.gpu

F = np.float32
KEYS_I = ("status", "done", "level_active", "it", "n_evals", "iters")
KEYS_F = ("lam", "error", "new_error", "diff_error")
KEYS_A = ("cand", "pose", "update")


def _reg(cols, rows):
    from rgbd360_amd.register import RegisterPhotoICP
    (rgbA, dA), (rgbB, dB), _ = synth.make_pair(cols, rows, seed=3)
    r = RegisterPhotoICP()
    r.setNumPyr(3)
    r.setTargetFrame(rgbA, dA)
    r.setSourceFrame(rgbB, dB)
    return r


@pytest.fixture(scope="module")
def regs(hip_lib):
    return _reg(256, 128), _reg(1024, 512)


def _bits(x):
    x = np.asarray(x)
    return x.view(np.uint32 if x.dtype == F else np.uint64)


def _same_state(a, b, what):
    for k in KEYS_I:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in KEYS_F:
        assert np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64), (what, k, a[k], b[k])
    for k in KEYS_A:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, a[k], b[k])


def _run(regs, row, level=0, **kw):
    """Route 0 and 1 on the small pair, 0 and 2 on the larger one: all four states equal bit for bit; returns route 0's."""
    small, large = regs
    old = small.debug_solve_state(level, row, route=0, **kw)
    _same_state(small.debug_solve_state(level, row, route=1, **kw), old, "route 1")
    _same_state(large.debug_solve_state(level, row, route=0, **kw), old, "route 0, larger pair")
    _same_state(large.debug_solve_state(level, row, route=2, **kw), old, "route 2")
    return old


def _row(H, g):
    return R.partial_row(H, g, e2=(3.0, 2.0), n=(1000, 800, 1500))


def _dominant(rng):
    """symmetric, strictly diagonally dominant float32: no step of the elimination swaps"""
    A = rng.uniform(-0.1, 0.1, size=(6, 6))
    H = 0.5 * (A + A.T) + np.diag(rng.uniform(4.0, 8.0, size=6))
    return H.astype(F)


def _pivot_cases():
    """(k, p, H): a symmetric H on which steps 0 .. k-1 take their diagonal entry and step k takes row p (p = k: no swap at all)."""
    rng = np.random.default_rng(20261020)
    out = []
    for k in range(6):
        for p in range(k, 6):
            H = _dominant(rng)
            if p != k:
                H[k, p] = H[p, k] = F(3.0) * H[k, k]      # column k below the diagonal: row p outweighs the diagonal entry
            out.append((k, p, H))
    return out


def test_every_pivot_choice_at_every_step(regs):
    cases = _pivot_cases()
    assert len(cases) == 21
    rng = np.random.default_rng(7)
    for k, p, H in cases:
        piv = R.lu64(H)[3]
        assert piv[:k] == list(range(k)) and piv[k] == p, (k, p, piv)      # the case is what it says (float64 pivot sequence)
        g = R.rhs_for(rng, H, mag=1e-3)
        o = _run(regs, _row(H, g))
        assert o["status"] == 0 and o["done"] == 0, (k, p, o)                # the step was taken: cand and update are the new ones
        u64 = -np.linalg.solve(H.astype(np.float64), g.astype(np.float64))
        assert np.allclose(o["update"], u64, rtol=1e-3, atol=1e-7), (k, p, o["update"], u64)      # (a sanity check; the exact pin is test_gn_solve_exact's)


def test_zero_pivot_and_rank_deficient(regs):
    rng = np.random.default_rng(11)
    H = _dominant(rng)
    H[2, :] = 0
    H[:, 2] = 0                                    # column 2 is zero when step 2 looks for its pivot
    g = R.rhs_for(rng, _dominant(rng))
    o = _run(regs, _row(H, g))
    assert o["status"] == 1 and o["done"] == 1, o          # ILL-POSED; candidate and update stay as they were
    assert np.array_equal(o["update"], np.ones(6, F))
    B = rng.normal(size=(6, 3))
    H3 = (B @ B.T).astype(F)                        # rank 3: the pivots behind the third are rounding noise, none is zero
    H3 = np.triu(H3) + np.triu(H3, 1).T
    _run(regs, _row(H3, g))                        # first pass: the rank test sees H + diag(H) -- whatever it says, every route says it
    o = _run(regs, _row(H3, g), first=0, it=1, error=10.0, lam=0.0, update=(1e-2,) * 6)      # undamped: ILL-POSED by the rank test alone
    assert o["status"] == 1 and o["done"] == 1, o


def _update_case(u):
    """H = I: the inverse is exact and the update is -g, so g = -u hands the exponential exactly u"""
    return _row(np.eye(6, dtype=F), -np.asarray(u, F))


def test_exponential_arms(regs):
    half = F(0.5)
    thr = R.ROT_THRESHOLD
    below, above = np.nextafter(half, F(0)), np.nextafter(half, F(1))
    for w in ([below, 0, 0], [half, 0, 0], [above, 0, 0],                         # angle^2 just below, at and just above 0.25
              [0.3, -0.3, 0.26], [0.2, 0.3, -0.35],                               # ... with all three components (0.2476, 0.2525)
              [thr * 0.5, 0, 0], [0, thr * 0.99, 0], [0, 0, thr * 1.01], [thr * 2, thr, 0],      # around the no-rotation threshold
              [0, 0, 0], [0.01, -0.02, 0.03]):
        u = np.array([1e-3, -2e-3, 3e-3] + list(w), np.float64).astype(F)
        o = _run(regs, _update_case(u))
        assert o["status"] == 0 and o["done"] == 0, (w, o)
        assert np.array_equal(_bits(o["update"]), _bits(u)), (w, o["update"])
        tsq = float(np.sum(np.asarray(u[3:], np.float64) ** 2))
        if tsq < thr * thr:                            # no rotation: the candidate is the translation alone
            assert np.array_equal(o["cand"][:3, :3], np.eye(3, dtype=F)), (w, o["cand"])
        assert np.array_equal(_bits(o["cand"][:3, 3]), _bits(u[:3]))


def test_state_machine_turns(regs):
    rng = np.random.default_rng(5)
    H = _dominant(rng)
    g = R.rhs_for(rng, H, mag=1e-3)
    row = _row(H, g)
    new_error = math.sqrt(5.0 / 1800.0)
    pose = np.eye(4)
    pose[:3, 3] = (0.01, -0.02, 0.03)
    # first pass of a level: the error is recorded, the step is taken from `pose`
    o = _run(regs, row, pose=pose, first=1)
    assert (o["status"], o["done"], o["it"]) == (0, 0, 0) and o["error"] == pytest.approx(new_error, rel=1e-14)
    # an accepted step: lambda / 5, it + 1, cand promoted, the next step computed
    o = _run(regs, row, pose=pose, first=0, it=2, error=new_error + 0.5, lam=0.2, update=(1e-2,) * 6)
    assert (o["status"], o["done"], o["it"]) == (0, 0, 3) and o["lam"] == 0.2 / 5.0
    # ... the last one the iteration budget allows: accepted, and the level is done
    o = _run(regs, row, pose=pose, first=0, it=9, error=new_error + 0.5, max_iters=10, update=(1e-2,) * 6)
    assert (o["status"], o["done"], o["it"]) == (0, 1, 10)
    # a rejected step (the error grew): nothing is taken, the level ends where it was
    o = _run(regs, row, pose=pose, first=0, it=2, error=new_error - 1e-3, update=(1e-2,) * 6)
    assert (o["status"], o["done"], o["it"], o["level_active"]) == (0, 1, 2, 0)
    assert np.array_equal(o["update"], np.full(6, 1e-2, F))
    # the same on level 1: the finished level hands over to level 0 (it = 0, update = 1, lambda = 1, first pass at the pose reached)
    o = _run(regs, row, level=1, pose=pose, first=0, it=2, error=new_error - 1e-3, update=(1e-2,) * 6)
    assert (o["status"], o["done"], o["it"], o["level_active"], o["lam"]) == (0, 0, 0, 0, 1.0)
    assert np.array_equal(o["update"], np.ones(6, F)) and np.array_equal(o["cand"], o["pose"])
    # a small update ends the loop although the step was accepted
    o = _run(regs, row, pose=pose, first=0, it=2, error=new_error + 0.5, update=(1e-6,) * 6)
    assert (o["status"], o["done"], o["it"]) == (0, 1, 3)
