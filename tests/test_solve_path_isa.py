"""The machine code of the fused launch's solve path (k_eval_fs<0,0>): wave 1's common case -- the diagonal entry is every step's pivot,
a rotation with angle^2 < 0.25 -- is fall-through code from the barrier behind solve_totals to the store of shCand.  No GPU needed:
the unit is compiled to ISA with the library's own flags (as tools/isa_loop_stats.py documents); skipped where hipcc is absent.

The path is read off the text: from the barrier on, every conditional branch counts as not taken (the scalar-uniform ones are laid out
that way on purpose) and the instructions are followed in textual order up to the last LDS store in front of the next barrier (shCand;
the diagnostic stamps are compiled out).  On that path there may be no branch on EXEC and no unconditional branch."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import build as B  # noqa: E402

KERNEL = "_ZN4r3609k_eval_fsILi0ELi0EEE"
VGPRS_AT_PARENT = 83


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


pytestmark = pytest.mark.skipif(_hipcc() is None, reason="hipcc is absent: no ISA to read")


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "api.s")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-pthread")]
    subprocess.check_call([_hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, B.SRC], stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    st = [i for i, l in enumerate(lines) if l.startswith(KERNEL) and l.split(";")[0].strip().endswith(":")][0]
    end = [i for i in range(st, len(lines)) if lines[i].startswith(".Lfunc_end")][0]
    return lines[st:end], lines[end:end + 200]


def _instr(line):
    t = line.split(";")[0].strip()
    return t if t and not t.endswith(":") and not t.startswith(".") else ""


def fall_through_path(body):
    """The instructions between the barrier behind solve_totals and the store of shCand, conditional branches not taken.
    The barrier is the last one in front of the kernel's first v_readlane_b32: the elimination's broadcasts are the first in the text
    (the tests below check that the path found is indeed the solve's)."""
    ins = [(i, _instr(l)) for i, l in enumerate(body)]
    ins = [(i, t) for i, t in ins if t]
    bars = [k for k, (_, t) in enumerate(ins) if t.startswith("s_barrier")]
    lanes = [k for k, (_, t) in enumerate(ins) if t.startswith("v_readlane_b32")]
    assert lanes, "no broadcast through the scalar unit in the kernel"
    first = max(b for b in bars if b < lanes[0])
    after = [b for b in bars if b > first]
    assert after, "no barrier behind the solve"
    path = []
    for _, t in ins[first + 1:after[0]]:
        path.append(t)
        if re.match(r"s_branch\b|s_setpc|s_endpgm", t):      # where the textual order stops being the executed one
            break
    stores = [k for k, t in enumerate(path) if t.startswith("ds_write")]
    assert stores, "no LDS store on the fall-through path"
    return path[:stores[-1] + 1]


def test_common_case_is_fall_through_code(kernel):
    body, _ = kernel
    path = fall_through_path(body)
    # the whole chain lies on it: the six broadcasts per elimination step, the reciprocals, the float64 series, five results stored
    assert sum(t.startswith("v_readlane_b32") for t in path) >= 30, "the path found is not wave 1's"
    assert sum(t.startswith("ds_write") for t in path) >= 5
    assert sum(bool(re.match(r"v_(mul|add|fma)_f64", t)) for t in path) >= 40
    exec_branches = [t for t in path if t.startswith("s_cbranch_exec")]
    jumps = [t for t in path if re.match(r"s_branch\b", t)]
    print("fall-through path: %d instructions, %d conditional branches (none taken)" % (len(path), sum(t.startswith("s_cbranch") for t in path)))
    assert exec_branches == []
    assert jumps == []
    assert not any(t.startswith("v_swap_b32") for t in path), "a pivot arm lies on the path"
    assert not any(t.startswith("v_sqrt_f64") or t.startswith("v_rsq_f64") or t.startswith("v_div_") for t in path), "the general arm of the exponential lies on the path"


def test_no_scratch_and_no_more_registers(kernel):
    _, tail = kernel
    text = "\n".join(tail)
    scratch = int(re.search(r"ScratchSize:\s*(\d+)", text).group(1))
    vgprs = int(re.search(r"NumVgprs:\s*(\d+)", text).group(1))
    print("ScratchSize", scratch, "NumVgprs", vgprs)
    assert scratch == 0
    assert vgprs <= VGPRS_AT_PARENT
