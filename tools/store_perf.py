"""Throughput of the resident frame store (rgbd360_store_align) next to the same pairs through the one-pair entry points, in ONE run on
one device: python tools/store_perf.py [W=2048] [reps=30] > profiles/frame_store_perf.txt
Workloads, PHOTO_DEPTH, frames resident in HBM, guess = identity:
  keyframe      1 target entry x 64 source entries                 (OdometryKeyFrame360.cpp:244-253)
  loop closure  8 x 8 entries, all 64 ordered pairs                (LoopClosure360.h:309-312, 348-351, both roles)
Baselines from the entry points that existed before the store: (1) one context, rgbd360_set_source_dev (+ rgbd360_set_target_dev when the
target changes) + rgbd360_align360 per pair; (2) the same through rgbd360_align360_begin / _finish on three contexts.
Every figure is a host clock around calls that end in a device synchronisation; `reps` repetitions of the 64-pair list per timed window,
three windows each (all three printed), one untimed warm-up.  9 distinct rendered frames are cycled through the entries."""
import ctypes as C, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rgbd360_amd import synth
from rgbd360_amd.register import RegisterPhotoICP
from rgbd360_amd.store import FrameStore

W = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
H = W // 2
hip = C.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]


def to_device(a):
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
    return p.value


def sh(cmd):
    try:
        return subprocess.run(cmd, shell=True, capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception:
        return "?"


print("box: %s | ROCm %s | GPU_MAX_HW_QUEUES seen: %s" % (sh("rocminfo | grep -m1 'Marketing Name.*MI' | sed 's/.*: *//'") or "?",
                                                       sh("cat /opt/rocm/.info/version") or "?", os.environ.get("GPU_MAX_HW_QUEUES", "(unset)")))
print("size %d x %d, 4 levels, PHOTO_DEPTH, %d x 64 pairs per timed window, 3 windows" % (W, H, reps), flush=True)
uniq = [synth.render(synth.trajectory_pose(k, 7), W, H, 7) for k in range(9)]
rgb_u = [to_device(f[0]) for f in uniq]
dep_u = [to_device(f[1]) for f in uniq]


def windows(f, n_per_call):
    f()
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            r = f()
        out.append(reps * n_per_call / (time.perf_counter() - t0))
    return out, r


def fmt(v):
    return "[" + ", ".join("%.0f" % x for x in v) + "] median %.0f" % sorted(v)[1]


def one_context(pairs, frame_of):
    reg = RegisterPhotoICP(); reg.setNumPyr(4)

    def f():
        cur, poses = None, []
        for t, s in pairs:
            if t != cur:
                reg.setTargetFrameDev(rgb_u[frame_of[t]], W * 3, dep_u[frame_of[t]], W * 2, 0, H, W); cur = t
            reg.setSourceFrameDev(rgb_u[frame_of[s]], W * 3, dep_u[frame_of[s]], W * 2, 0, H, W)
            reg.alignFrames360(None, 2)
            poses.append(reg.getOptimalPose())
        return np.stack(poses)
    r = windows(f, len(pairs))
    reg.close()
    return r


def three_contexts(pairs, frame_of):
    regs = [RegisterPhotoICP() for _ in range(3)]
    for r_ in regs:
        r_.setNumPyr(4)

    def f():
        cur, poses = [None] * 3, []
        for k in range(0, len(pairs), 3):
            grp = pairs[k:k + 3]
            for c, (t, s) in enumerate(grp):
                if t != cur[c]:
                    regs[c].setTargetFrameDev(rgb_u[frame_of[t]], W * 3, dep_u[frame_of[t]], W * 2, 0, H, W); cur[c] = t
                regs[c].setSourceFrameDev(rgb_u[frame_of[s]], W * 3, dep_u[frame_of[s]], W * 2, 0, H, W)
                regs[c].alignFrames360_begin(None, 2)
            for c in range(len(grp)):
                regs[c].alignFrames360_finish()
                poses.append(regs[c].getOptimalPose())
        return np.stack(poses)
    r = windows(f, len(pairs))
    for r_ in regs:
        r_.close()
    return r


def store_run(pairs, frame_of, n_entries):
    reg = RegisterPhotoICP(); reg.setNumPyr(4)
    st = FrameStore(reg, n_entries, H, W)
    ents = list(range(n_entries))
    put = lambda: st.put_dev(ents, [rgb_u[frame_of[e]] for e in ents], [dep_u[frame_of[e]] for e in ents], 0)
    put()
    pt = []
    for _ in range(3):
        t0 = time.perf_counter(); put(); pt.append((time.perf_counter() - t0) / n_entries * 1e6)
    print("  store: %d entries x %.1f MB (rgbd360_store_entry_bytes %d); put_dev of all entries: %s us per frame"
          % (n_entries, st.entry_bytes / 1e6, st.entry_bytes, "[" + ", ".join("%.1f" % x for x in pt) + "]"), flush=True)
    out = {}
    for ni in (16, 32):
        out[ni] = windows(lambda: st.align(pairs, method=2, n_inflight=ni)[0], len(pairs))
    st.close(); reg.close()
    return out


for name, pairs, frame_of, n_entries in (
        ("keyframe: 1 target x 64 sources", [(0, 1 + k) for k in range(64)], [4] + [(0, 1, 2, 3, 5, 6, 7, 8)[k % 8] for k in range(64)], 65),
        ("loop closure: 8 x 8 entries, 64 ordered pairs", [(t, s) for t in range(8) for s in range(8)], list(range(8)), 8)):
    print("\n== " + name, flush=True)
    st = store_run(pairs, frame_of, n_entries)
    b1, p1 = one_context(pairs, frame_of)
    b3, p3 = three_contexts(pairs, frame_of)
    base = max(sorted(b1)[1], sorted(b3)[1])
    for ni in (16, 32):
        v, p = st[ni]
        print("  rgbd360_store_align n_inflight %2d : %s alignments/s  (x %.2f of the better baseline; poses bit-equal to one context: %s)"
              % (ni, fmt(v), sorted(v)[1] / base, bool(np.array_equal(p, p1))), flush=True)
    print("  baseline, one context            : %s alignments/s" % fmt(b1))
    print("  baseline, 3 contexts begin/finish: %s alignments/s  (poses bit-equal to one context: %s)" % (fmt(b3), bool(np.array_equal(p3, p1))), flush=True)
