"""Diagnostic: phase timestamps inside the solve (k_solve, or the prologue of the fused launch k_eval_fs).
Needs the RGBD360_SOLVE_STAMPS builds of the library:  python tools/solve_stamps.py build   (cross-compiles, no GPU needed),
then on the GPU box:
    python tools/solve_stamps.py                      phase ends of one launch, levels 0 and 3, methods 0 and 2 (2048x1024)
    python tools/solve_stamps.py chain [RUNS] [LIB]   "totals -> candidate pose done" of RUNS launches (default 5), 2048x1024 and 256x128;
                                                      LIB: another stamps build of the library (A/B against another commit's)
    python tools/solve_stamps.py fetch [RUNS] [LIB]   the row fetch of stage_pending: "loads issued", "row sums in LDS" (behind the barrier), totals
                                                      and candidate pose, mean over RUNS launches, 2048x1024 and 256x128
    python tools/solve_stamps.py twice [RUNS]         the RGBD360_SOLVE_TWICE build: wave 1 of every block walks its path a first time into
                                                      spare LDS slots and then for real -- the cold and the warm price of the same code,
                                                      per phase (inverse done / update + exponential + candidate done)"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbd360_amd import _lib, build as B
STAMPS_LIB = os.path.join(os.path.dirname(B.LIB), "librgbd360_hip_stamps.so")
TWICE_LIB = os.path.join(os.path.dirname(B.LIB), "librgbd360_hip_stamps2x.so")
args = sys.argv[1:]
mode = args.pop(0) if args else "phases"
if mode == "build":
    for lib, flags in ((STAMPS_LIB, ["-DRGBD360_SOLVE_STAMPS"]), (TWICE_LIB, ["-DRGBD360_SOLVE_STAMPS", "-DRGBD360_SOLVE_TWICE"])):
        print(B.compile_library(lib, flags, selects_vop3=False))
    sys.exit(0)
import numpy as np
runs = int(args.pop(0)) if args and args[0].isdigit() else 5
_lib.LIB_PATH = TWICE_LIB if mode == "twice" else (args.pop(0) if args else STAMPS_LIB)
from rgbd360_amd import synth
from rgbd360_amd.register import RegisterPhotoICP


def make_reg(cols, rows, n_pyr):
    (rgbA, dA), (rgbB, dB), T = synth.make_pair(cols, rows, seed=1234)
    reg = RegisterPhotoICP(); reg.setNumPyr(n_pyr)
    reg.setTargetFrame(rgbA, dA); reg.setSourceFrame(rgbB, dB)
    return reg


def stamps_of(reg, level, method):
    """the stamps (us from kernel start) the last launch of a 20-iteration schedule left"""
    reg.forced_iters(level, np.eye(4), method, 20)
    out = np.zeros(8, np.uint64)
    reg._L.rgbd360_debug_solve_stamps.argtypes = [C.c_void_p, C.c_void_p]
    reg._L.rgbd360_debug_solve_stamps(reg._ctx(), out.ctypes.data_as(C.c_void_p))
    return out.astype(np.float64) / 100.0


if mode == "phases":
    reg = make_reg(2048, 1024, 4)
    names = ["staged+row sums", "totals", "bookkeeping (wave 0)", "loads issued", "end", "inverse (wave 1)", "update+exp+cand (wave 1)", "rank (wave 2)"]
    for level in (0, 3):
        for method in (0, 2):
            out = stamps_of(reg, level, method)
            print("level", level, "method", method, "| phase ends, us from kernel start:", "; ".join("%s %.2f" % (n, v) for n, v in zip(names, out)))
    sys.exit(0)
print("library", os.path.basename(_lib.LIB_PATH))
for cols, rows, n_pyr in ((2048, 1024, 4), (256, 128, 2)):
    reg = make_reg(cols, rows, n_pyr)
    stamps_of(reg, 0, 0)       # (the first schedule of a context pays for allocations)
    if mode == "fetch":
        a = np.array([stamps_of(reg, 0, 0) for _ in range(runs)])
        m = a.mean(axis=0)
        print("%dx%d | loads issued %.3f | row sums in LDS %.3f (min %.2f max %.2f) | totals %.3f | candidate pose %.3f | state written %.3f us  (mean of %d launches)"
              % (cols, rows, m[3], m[0], a[:, 0].min(), a[:, 0].max(), m[1], m[6], m[4], runs), flush=True)
        continue
    for run in range(runs):
        s = stamps_of(reg, 0, 0)
        if mode == "twice":      # stamps 7 / 2: the first walk's inverse / candidate; 5 / 6: the second's
            print("%dx%d run %d | first walk: inverse %.2f us, exp+cand %.2f us | second walk: inverse %.2f us, exp+cand %.2f us | first - second %.2f us"
                  % (cols, rows, run, s[7] - s[1], s[2] - s[7], s[5] - s[2], s[6] - s[5], (s[2] - s[1]) - (s[6] - s[2])), flush=True)
        else:
            print("%dx%d run %d | totals %.2f -> inverse %.2f -> candidate pose %.2f us | totals -> candidate pose done %.2f us"
                  % (cols, rows, run, s[1], s[5], s[6], s[6] - s[1]), flush=True)
