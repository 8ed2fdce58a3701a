"""The bytes the four alignments against the voxel map produce on the device, recorded as a fixture: tests/golden/map_align_bits.json.

    python tools/map_align_bits.py [--out tests/golden/map_align_bits.json]       (RGBD360_LIB: the build of the library to record from)

tests/test_map_align_bits_gpu.py recomputes every case with compute() below and compares it with the file, byte for byte: a change of
the evaluation kernels (csrc/map_align.h and the methods' headers) that moves one bit of a sum, of a per-point output or of an aligned
pose fails it.  Record from the library the change is measured against, BEFORE the kernels change.  Every case is computed twice in the
process and nothing is written if the two differ.

Inputs, all from seeds (nothing large is stored), every map at voxel_map_reference.general_pose() with capacity 1 << 16 and the default box,
fed with the colour image synth returns with the depth (a cloud takes the bytes of its pixels):
  frame    frame 0 of synth.make_pair(256, 128, seed=1234), uint16 depth, convention 2, the sphere route; maps of leaf 0.05 and 0.1
  cloud    reg.sphere_cloud of that frame (32 768 points, 32 workgroups), the cloud route against the same two maps
  ragged   2 * 1024 + 37 of its valid points, evenly spaced (tests/test_map_align_plane_gpu.py, test_ragged_cloud_sizes), leaf 0.1
  strip    synth.render(synth.trajectory_pose(0, 7), 1100, 24, 7) in a map of its own, leaf 0.1: a full tile and a ragged second tile of
           76 columns per row, the smallest shape in which all four point slots of a thread and a second blockIdx.x of the sphere route
           hold pixels (at 256 and 200 columns only the first slot ever does)
Per input, method and pose (the map's, and map_align_reference.perturbed(P, 0.01, 0.003, 8)); the methods are point, plane, gicp (no source
normals), colour and, on the three cloud inputs, gicp_normals (a unit normal per point from seed 5):
  eval     the diag evaluation entry: the 17 / 30 / 30 / 31 float64 sums as hex, the counters, a SHA-256 of each per-point array
  align    the public entry from that pose with default parameters: status, iterations, converged, pose, hessian, gradient and the
           fitness fields as hex, the counters, every trace record as hex
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rgbd360_amd import synth                                        # noqa: E402
from rgbd360_amd.register import RegisterPhotoICP, pose_to_cm, _ptr  # noqa: E402
from rgbd360_amd.voxel_map import VoxelMap                           # noqa: E402
import map_align_reference as A                                      # noqa: E402
import voxel_map_reference as R                                      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "map_align_bits.json")
# per method: the diag entry, its parameter maker, sums, counters, the per-point arrays (name, dtype, values per point)
_KEY_D2 = (("key3", np.int32, 3), ("d2", np.float32, 1))
_GICP = ("rgbd360_map_align_gicp_eval", "align_gicp_params", 30, 6, _KEY_D2 + (("weight_cost", np.float64, 7), ("class", np.uint8, 1)))
METHODS = {
    "point": ("rgbd360_map_align_eval", "align_params", 17, 3, _KEY_D2),
    "plane": ("rgbd360_map_align_plane_eval", "align_plane_params", 30, 5, _KEY_D2 + (("normal_r", np.float64, 4), ("class", np.uint8, 1))),
    "gicp": _GICP,
    "gicp_normals": _GICP,           # (cloud inputs only)
    "colour": ("rgbd360_map_align_colour_eval", "align_colour_params", 31, 5, _KEY_D2 + (("residuals", np.float64, 2), ("class", np.uint8, 1))),
}


def _hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


class Source:
    """An input of the alignments: the sphere route's images, or the cloud route's points with their colours and seeded normals."""

    def __init__(self, rgb=None, depth=None, xyz=None, rgb3=None):
        self.rgb, self.depth = rgb, depth
        self.xyz = None if xyz is None else np.ascontiguousarray(xyz, np.float32)
        self.rgb3 = None if rgb3 is None else np.ascontiguousarray(rgb3, np.uint8)
        self.n = depth.size if depth is not None else len(self.xyz)
        self.normals = None
        if xyz is not None:
            v = np.random.default_rng(5).standard_normal((self.n, 3))
            self.normals = np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True), np.float32)

    def methods(self):
        return [k for k in METHODS if k != "gicp_normals" or self.xyz is not None]


def inputs(reg):
    """[(name, leaf, (rgb, depth) of the map, Source)]"""
    rgb, depth = (np.ascontiguousarray(a) for a in synth.make_pair(256, 128, seed=1234)[0])
    assert depth.dtype == np.uint16 and rgb.shape == depth.shape + (3,)
    cloud, rgb3 = reg.sphere_cloud(depth, 2), rgb.reshape(-1, 3)
    valid = np.nonzero(np.isfinite(cloud).all(axis=1))[0]
    pick = valid[np.linspace(0, len(valid) - 1, 2 * 1024 + 37).astype(np.int64)]
    srgb, strip = (np.ascontiguousarray(a) for a in synth.render(synth.trajectory_pose(0, 7), 1100, 24, 7))
    assert strip.shape == (24, 1100) and strip.dtype == np.uint16
    frame, whole = Source(rgb=rgb, depth=depth), Source(xyz=cloud, rgb3=rgb3)
    return [("frame", 0.05, (rgb, depth), frame), ("frame", 0.1, (rgb, depth), frame), ("cloud", 0.05, (rgb, depth), whole), ("cloud", 0.1, (rgb, depth), whole),
            ("ragged", 0.1, (rgb, depth), Source(xyz=cloud[pick], rgb3=rgb3[pick])), ("strip", 0.1, (srgb, strip), Source(rgb=srgb, depth=strip))]


def evaluate(hip, m, method, pose, s):
    entry, params, n_sums, n_counters, arrays = METHODS[method]
    host = [np.zeros((s.n, k), dt) for _, dt, k in arrays]
    dev = [C.c_void_p() for _ in arrays]
    for d, a in zip(dev, host):
        assert hip.hipMalloc(C.byref(d), a.nbytes) == 0
    sums, counters = np.zeros(n_sums, np.float64), np.zeros(n_counters, np.int64)
    p = getattr(m, params)()
    image = (_ptr(s.depth), s.depth.strides[0], 0, s.depth.shape[0], s.depth.shape[1], 2) if s.depth is not None else (None, 0, 0, 0, 0, 0)
    xyz = None if s.xyz is None else _ptr(s.xyz)
    n = 0 if s.xyz is None else s.n
    if method == "colour":
        src = ((_ptr(s.rgb), s.rgb.strides[0]) if s.depth is not None else (None, 0)) + image + (xyz, None if s.xyz is None else _ptr(s.rgb3), n)
    elif method.startswith("gicp"):
        src = image + (xyz, _ptr(s.normals) if method == "gicp_normals" else None, n)
    else:
        src = image + (xyz, n)
    tail = (0, None, None) if method == "point" else ()
    rc = getattr(m._L, entry)(m._handle(), *src, _ptr(pose_to_cm(pose)), 0, C.byref(p), _ptr(sums), _ptr(counters), *dev, *tail)
    assert rc == 0, (rc, m._L.rgbd360_map_last_error(m._handle()))
    out = {"sums": sums.tobytes().hex(), "counters": counters.tolist()}
    for (name, _, _), d, a in zip(arrays, dev, host):
        assert hip.hipMemcpy(_ptr(a), d, a.nbytes, 2) == 0
        hip.hipFree(d)
        out[name] = hashlib.sha256(a.tobytes()).hexdigest()
    return out


def align(m, method, pose, s):
    suffix = {"point": "", "gicp_normals": "_gicp"}.get(method, "_" + method)
    extra = {"normals": s.normals} if method == "gicp_normals" else {}
    if s.depth is not None:
        head = (s.rgb, s.depth) if method == "colour" else (s.depth,)
        out, res = getattr(m, "align_sphere" + suffix)(*head, pose, convention=2)
    else:
        head = (s.xyz, s.rgb3) if method == "colour" else (s.xyz,)
        out, res = getattr(m, "align_cloud" + suffix)(*head, pose, **extra)
    rec = {k: (np.asarray(v).tobytes().hex() if isinstance(v, (float, np.ndarray)) else int(v)) for k, v in res.items()}
    rec["pose"] = out.tobytes().hex()
    rec["trace"] = [np.int64(n).tobytes().hex() + np.float64(ss).tobytes().hex() + u.tobytes().hex() for n, ss, u in m.align_trace()]
    return rec


def compute(reg):
    """{case: {"eval": ..., "align": ...}} of every case on the device."""
    hip = _hip()
    P = R.general_pose()
    poses = (("map_pose", P), ("perturbed", A.perturbed(P, 0.01, 0.003, 8)))
    cases = {}
    for name, leaf, (rgb, depth), source in inputs(reg):
        with VoxelMap(reg, leaf, 1 << 16) as m:
            m.insert_sphere(rgb, depth, P, convention=2)
            for method in source.methods():
                for at, pose in poses:
                    cases["%s/leaf%g/%s/%s" % (name, leaf, method, at)] = {"eval": evaluate(hip, m, method, pose, source),
                                                                          "align": align(m, method, pose, source)}
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    reg = RegisterPhotoICP()
    first, second = compute(reg), compute(reg)
    reg.close()
    differ = [k for k in first if first[k] != second[k]]
    if differ:
        sys.exit("two runs in one process differ, nothing written: %s" % ", ".join(differ))
    with open(a.out, "w") as f:
        json.dump({"cases": first}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s (%d bytes)" % (len(first), a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
