"""The solve path (solve_waves: wave 1's common case as fall-through code) on the three routes of rgbd360_debug_solve_state, against
each other and against recorded bits.  The same hand-made partial row and state go through route 0 (k_solve) and routes 1 and 2 (the
prologue of k_eval_fs), and every word the solve decides -- candidate pose, pose, update, status, done, iteration counts, level,
damping, errors -- is compared BIT FOR BIT: between the routes, and with tests/golden/solve_bits.json.  All routes run the same
solve code now; the recorded bits are those of the form k_solve ran until it moved to this one (lane-masked regions, a row swap
under a branch at every elimination step, a second copy of wave 0's bookkeeping), recorded from the last commit that had it
(tools/solve_bits.py, cases in tests/solve_cases.py) -- so the comparison still is "the old code and the new code agree".  The
cases are the paths the fall-through form lays out differently: every pivot choice at every elimination step (the swap arms lie
behind the path, taken by a second elimination), a zero pivot, a rank-deficient H, the exponential's arms on both sides of
angle^2 = 0.25 and of the no-rotation threshold, and the state machine's turns (first pass of a level, accepted and rejected step,
level hand-over).

Frames: 256 x 128 for routes 0 and 1.  Route 2 places the row at block row 40 of the table and needs a level with more than 40 block
rows; 256 x 128 has 32 at most, so route 2 runs on a 1024 x 512 pair (whose level 1, for the hand-over, still has 128).  Route 0 is run
on both pairs and must agree with itself."""
import numpy as np
import pytest

import gn_reference as R
import solve_cases as S
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


@pytest.fixture(scope="module")
def recorded():
    return S.load_recorded()


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


def _run(regs, recorded, case):
    """Route 0 and 1 on the small pair, 0 and 2 on the larger one: all four states equal bit for bit, and equal to the recorded one
    (pend_nb on route 0 only: a fused launch leaves its own pass pending, as many rows as its frame has); returns route 0's."""
    small, large = regs
    level, row, kw = case["level"], case["row"], case["kw"]
    old = small.debug_solve_state(level, row, route=0, **kw)
    runs = [("route 0", old, ()),
            ("route 1", small.debug_solve_state(level, row, route=1, **kw), ("pend_nb",)),
            ("route 0, larger pair", large.debug_solve_state(level, row, route=0, **kw), ()),
            ("route 2", large.debug_solve_state(level, row, route=2, **kw), ("pend_nb",))]
    for what, state, _ in runs[1:]:
        _same_state(state, old, what)
    for what, state, skip in runs:
        differ = S.differences(state, recorded[case["name"]], skip=skip)
        assert not differ, (case["name"], what, differ)
    return old


def test_every_pivot_choice_at_every_step(regs, recorded):
    cases = S.pivot_cases()
    assert len(cases) == 21
    for c in cases:
        k, p, H, g = c["k"], c["p"], c["H"], c["g"]
        piv = R.lu64(H)[3]
        assert piv[:k] == list(range(k)) and piv[k] == p, (k, p, piv)      # the case is what it says (float64 pivot sequence)
        o = _run(regs, recorded, c)
        assert o["status"] == 0 and o["done"] == 0, (k, p, o)                # the step was taken: cand and update are the new ones
        u64 = -np.linalg.solve(H.astype(np.float64), g.astype(np.float64))
        assert np.allclose(o["update"], u64, rtol=1e-3, atol=1e-7), (k, p, o["update"], u64)      # (a sanity check; the exact pin is test_gn_solve_exact's)


def test_zero_pivot_and_rank_deficient(regs, recorded):
    zero, rank3_first, rank3_undamped = S.deficient_cases()
    o = _run(regs, recorded, zero)
    assert o["status"] == 1 and o["done"] == 1, o          # ILL-POSED; candidate and update stay as they were
    assert np.array_equal(o["update"], np.ones(6, F))
    _run(regs, recorded, rank3_first)              # first pass: the rank test sees H + diag(H) -- whatever it says, every route says it
    o = _run(regs, recorded, rank3_undamped)       # undamped: ILL-POSED by the rank test alone
    assert o["status"] == 1 and o["done"] == 1, o


def test_exponential_arms(regs, recorded):
    thr = R.ROT_THRESHOLD
    cases = S.exponential_arm_cases()
    assert len(cases) == 11
    for c in cases:
        w, u = c["w"], c["u"]
        o = _run(regs, recorded, c)
        assert o["status"] == 0 and o["done"] == 0, (w, o)
        assert np.array_equal(_bits(o["update"]), _bits(u)), (w, o["update"])
        tsq = float(np.sum(np.asarray(u[3:], np.float64) ** 2))
        if tsq < thr * thr:                            # no rotation: the candidate is the translation alone
            assert np.array_equal(o["cand"][:3, :3], np.eye(3, dtype=F)), (w, o["cand"])
        assert np.array_equal(_bits(o["cand"][:3, 3]), _bits(u[:3]))


def test_state_machine_turns(regs, recorded):
    first, accepted, last_allowed, rejected, rejected_l1, small_update = S.state_turn_cases()
    new_error = S.STATE_TURN_ERROR
    # first pass of a level: the error is recorded, the step is taken from `pose`
    o = _run(regs, recorded, first)
    assert (o["status"], o["done"], o["it"]) == (0, 0, 0) and o["error"] == pytest.approx(new_error, rel=1e-14)
    # an accepted step: lambda / 5, it + 1, cand promoted, the next step computed
    o = _run(regs, recorded, accepted)
    assert (o["status"], o["done"], o["it"]) == (0, 0, 3) and o["lam"] == 0.2 / 5.0
    # ... the last one the iteration budget allows: accepted, and the level is done
    o = _run(regs, recorded, last_allowed)
    assert (o["status"], o["done"], o["it"]) == (0, 1, 10)
    # a rejected step (the error grew): nothing is taken, the level ends where it was
    o = _run(regs, recorded, rejected)
    assert (o["status"], o["done"], o["it"], o["level_active"]) == (0, 1, 2, 0)
    assert np.array_equal(o["update"], np.full(6, 1e-2, F))
    # the same on level 1: the finished level hands over to level 0 (it = 0, update = 1, lambda = 1, first pass at the pose reached)
    o = _run(regs, recorded, rejected_l1)
    assert (o["status"], o["done"], o["it"], o["level_active"], o["lam"]) == (0, 0, 0, 0, 1.0)
    assert np.array_equal(o["update"], np.ones(6, F)) and np.array_equal(o["cand"], o["pose"])
    # a small update ends the loop although the step was accepted
    o = _run(regs, recorded, small_update)
    assert (o["status"], o["done"], o["it"]) == (0, 1, 3)
