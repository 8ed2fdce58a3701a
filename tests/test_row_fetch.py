"""The fused launches fetch the pending pass's partial table in 16-byte pieces on eight waves (stage_pending, photo_icp_kernels.h); the
two-launch solve (k_solve, solve_block) keeps the 8-byte form on sixteen, for any row count.  The row fetch is all that differs between
the routes: behind it k_solve runs the same solve code as the fused launches (solve_staged; it had a form of its own once, whose bits
tests/golden/solve_bits.json holds).  Both fetches must form every column total in the same association:

    s[q]   = 0.0 + x[q] + x[q + 32] + ... + x[q + 224]          q = 0 ... 31, rows >= n_rows count as explicit 0.0 terms
    red[w] = s[2 w] + s[2 w + 1]                                w = 0 ... 15
    tot    = 0.0 + red[0] + red[1] + ... + red[15]

A hand-made single row (rgbd360_debug_solve_partials) cannot see a row summed in the wrong group or order; a whole table can
(rgbd360_debug_solve_table).  The table test compares `tot` bit for bit between k_solve (route 0), the prologue of k_eval_fs (1) and
k_solve_pending (2) and against a numpy float64 restatement of the order above -- and shows, for the same seeded tables, that two other
plausible orders (j split 0-3 / 4-7; plain row by row) do NOT give the same bits, so that agreement means something.  The schedule
test compares the fused schedule with the two-launch schedule bit for bit at the level-0 block counts where the fetch changes shape.
The last case needs no GPU: the machine code in front of k_eval_fs<0,0>'s first barrier."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import build as B  # noqa: E402
from rgbd360_amd import synth  # noqa: E402

gpu = pytest.mark.gpu

Q, J, V = 32, 8, 32
N_ROWS = [1, 31, 32, 33, 64, 200, 255, 256]
LATE = (40, 1)              # n_rows, rows_hint: the host's bound is too small, the device fetches the rest


def make_rows(n_rows, seed):
    """+-2^e * u, e in [-20, 20], u in [1, 2)"""
    rng = np.random.default_rng(seed)
    e = rng.integers(-20, 21, size=(n_rows, V))
    u = rng.uniform(1.0, 2.0, size=(n_rows, V))
    sign = np.where(rng.integers(0, 2, size=(n_rows, V)) == 0, -1.0, 1.0)
    return sign * np.ldexp(u, e)


def _table(rows):
    x = np.zeros((Q * J, V), np.float64)
    x[:len(rows)] = rows
    return x


def _totals(s):
    red = s[0::2] + s[1::2]
    tot = np.zeros(V, np.float64)
    for k in range(Q // 2):
        tot = tot + red[k]
    return tot


def tot_shipped(rows):
    x, nb = _table(rows), len(rows)
    q = np.arange(Q)[:, None]
    s = np.zeros((Q, V), np.float64)
    for j in range(J):
        s = s + np.where(q + Q * j < nb, x[j * Q:(j + 1) * Q], 0.0)
    return _totals(s)


def tot_split_j(rows):
    """the same row groups, j = 0 ... 3 and 4 ... 7 summed apart"""
    x = _table(rows)
    lo, hi = np.zeros((Q, V), np.float64), np.zeros((Q, V), np.float64)
    for j in range(J // 2):
        lo = lo + x[j * Q:(j + 1) * Q]
        hi = hi + x[(j + J // 2) * Q:(j + J // 2 + 1) * Q]
    return _totals(lo + hi)


def tot_row_by_row(rows):
    tot = np.zeros(V, np.float64)
    for r in rows:
        tot = tot + r
    return tot


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _other_orders_differ(rows):
    n = len(rows)
    want = tot_shipped(rows)
    d_split = int((_bits(tot_split_j(rows)) != _bits(want)).sum())
    d_plain = int((_bits(tot_row_by_row(rows)) != _bits(want)).sum())
    print("n_rows %d: columns that differ from the shipped order: j split %d, row by row %d of %d" % (n, d_split, d_plain, V))
    if n >= 200:
        assert d_split > 0, n
    if n >= 31:
        assert d_plain > 0, n
    return want


@pytest.mark.parametrize("n_rows", N_ROWS + [LATE[0]])
def test_other_orders_give_other_bits(n_rows):
    """No GPU: the tables of the table test tell the shipped order from its neighbours."""
    _other_orders_differ(make_rows(n_rows, 1000 + n_rows))


@pytest.fixture(scope="module")
def table_reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    (rgbA, dA), (rgbB, dB), _ = synth.make_pair(256, 128, seed=3)
    r = RegisterPhotoICP()
    r.setNumPyr(1)
    r.setTargetFrame(rgbA, dA)
    r.setSourceFrame(rgbB, dB)
    return r


@gpu
@pytest.mark.parametrize("n_rows,hint", [(n, n) for n in N_ROWS] + [LATE])
def test_table_totals(table_reg, n_rows, hint):
    rows = make_rows(n_rows, 1000 + n_rows)
    want = _other_orders_differ(rows)
    outs = [table_reg.debug_solve_table(0, rows, rows_hint=hint, method=0, route=route) for route in (0, 1, 2)]
    for route, o in enumerate(outs):
        differ = int((_bits(o["tot"]) != _bits(want)).sum())
        print("route %d: %d of %d totals differ from the restatement" % (route, differ, V))
    for route, o in enumerate(outs):
        assert np.array_equal(_bits(o["tot"]), _bits(outs[0]["tot"])), (n_rows, hint, route, o["tot"], outs[0]["tot"])
        assert np.array_equal(_bits(o["tot"]), _bits(want)), (n_rows, hint, route, o["tot"], want)
    # the solve behind the totals ran on the same numbers: the same verdict and candidate pose on every route
    for route in (1, 2):
        assert outs[route]["status"] == outs[0]["status"] and outs[route]["n_evals"] == outs[0]["n_evals"], (n_rows, hint, route)
        assert np.array_equal(_bits(outs[route]["cand"]), _bits(outs[0]["cand"])), (n_rows, hint, route)


# ---- fused against two-launch ----
# cols, rows: level-0 block count 1 (a single row), 32 (the short form's upper edge), 33 (the first long-form size), 200 (the last batch
# partly filled)
SIZES = {"32x16": (32, 16), "256x128": (256, 128), "264x128": (264, 128), "1280x640": (1280, 640)}


class Pair:
    """One synthetic pair in two contexts: the fused schedule (the library's default) and the two-launch schedule."""

    def __init__(self, cols, rows, n_pyr):
        from rgbd360_amd.register import RegisterPhotoICP
        (rgbA, dA), (rgbB, dB), self.truth = synth.make_pair(cols, rows, seed=3)
        self.regs = []
        for fused in (True, False):
            r = RegisterPhotoICP()
            r.setNumPyr(n_pyr)
            r.debug_set_schedule(fused_solve=fused, fused_occ=fused)
            r.setTargetFrame(rgbA, dA)
            r.setSourceFrame(rgbB, dB)
            self.regs.append(r)

    def forced(self, method, k):
        return [r.forced_iters(0, np.eye(4), method, k) for r in self.regs]

    def align(self, method):
        out = []
        for r in self.regs:
            rc = r.alignFrames360(np.eye(4), method)
            out.append(dict(status=rc, pose=r.getOptimalPose().copy(), iters=list(r.num_iterations), H=r.getHessian().copy(), g=r.getGradient().copy()))
        return out


def _same_forced(a, b, what):
    assert a["status"] == b["status"], (what, a["status"], b["status"])
    assert np.array_equal(_bits(a["pose"]), _bits(b["pose"])), (what, a["pose"], b["pose"])
    assert np.float64(a["rms"]).view(np.uint64) == np.float64(b["rms"]).view(np.uint64), (what, a["rms"], b["rms"])


def _same_align(a, b, what):
    assert a["status"] == b["status"], (what, a["status"], b["status"])
    assert a["iters"] == b["iters"], (what, a["iters"], b["iters"])
    for k in ("pose", "H", "g"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, a[k], b[k])


@pytest.fixture(scope="module")
def pairs(hip_lib):
    return {name: Pair(cols, rows, 1) for name, (cols, rows) in SIZES.items()}


@gpu
@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("size", list(SIZES))
def test_fused_schedule_same_bits(pairs, size, method):
    p = pairs[size]
    a, b = p.forced(method, 4)
    _same_forced(a, b, (size, method, "forced"))
    a, b = p.align(method)
    _same_align(a, b, (size, method, "alignment"))


@gpu
@pytest.mark.parametrize("method", [0, 2])
def test_three_levels_same_bits(hip_lib, method):
    """1280 x 640, three levels: a launch of one level fetches the rows of another."""
    p = Pair(1280, 640, 3)
    a, b = p.align(method)
    _same_align(a, b, ("1280x640, 3 levels", method))


# ---- the machine code (no GPU) ----
KERNEL = "_ZN4r3609k_eval_fsILi0ELi0EEE"


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def _instr(line):
    t = line.split(";")[0].strip()
    return t if t and not t.endswith(":") and not t.startswith(".") else ""


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is absent: no ISA to read")
def test_rows_are_requested_in_16_byte_loads(tmp_path):
    out = str(tmp_path / "api.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-pthread")]
    subprocess.check_call([_hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, B.SRC], stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    st = [i for i, l in enumerate(lines) if l.startswith(KERNEL) and l.split(";")[0].strip().endswith(":")][0]
    end = [i for i in range(st, len(lines)) if lines[i].startswith(".Lfunc_end")][0]
    ins = [t for t in (_instr(l) for l in lines[st:end]) if t]
    first_barrier = [k for k, t in enumerate(ins) if t.startswith("s_barrier")][0]
    front = ins[:first_barrier]
    x2 = sum(t.startswith("global_load_dwordx2") for t in front)
    x4 = sum(t.startswith("global_load_dwordx4") for t in front)
    tail = "\n".join(lines[end:end + 200])
    scratch = int(re.search(r"ScratchSize:\s*(\d+)", tail).group(1))
    vgprs = int(re.search(r"NumVgprs:\s*(\d+)", tail).group(1))
    print("in front of the first barrier: %d instructions, %d global_load_dwordx2, %d global_load_dwordx4; NumVgprs %d, ScratchSize %d"
          % (len(front), x2, x4, vgprs, scratch))
    assert x2 == 0
    assert 1 <= x4 <= 16
    assert vgprs <= 83
    assert scratch == 0
