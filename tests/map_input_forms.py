"""One frame in every form a rgbd360_map_* entry takes it in, each form once in host and once in device memory, and the same call made
on both: host-input and on_device = 1 calls must not differ in a bit (the statistics, the map read out, the pose, the result struct).
The frame is the 1100 x 24 strip, the smallest image that fills all four point slots of a thread and a second tile per row
(tests/test_voxel_map_gpu.py); the forms:
    f32_padded   float32 depth, its row step 64 bytes longer than a row; colour, its row step 5 bytes longer than a row
    u16          uint16 depth, no colour
    cloud        the same points as a cloud of 1100 x 24 points with their colours (the entries that change the map only)
Device memory comes from hipMalloc of the HIP runtime the library is linked to, as everywhere in these suites."""
import ctypes as C

import numpy as np

import map_align_reference as A
import voxel_map_reference as R

LEAF = 0.1
POSE_A = R.general_pose()


def pose_b():
    T = np.array(POSE_A, np.float64)
    T[:3, 3] += (0.04, -0.03, 0.02)
    return T.astype(np.float32)


def cm(pose):
    return np.ascontiguousarray(np.asarray(pose, np.float32).T.reshape(16))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def hip_runtime():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def padded_rows(a, pad):
    """The rows of `a` (H x W [x 3]) as bytes, `pad` unused bytes behind each."""
    rows = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
    buf = np.full((rows.shape[0], rows.shape[1] + pad), 0xEE, np.uint8)
    buf[:, :rows.shape[1]] = rows
    return buf


class Forms:
    """forms[name] = (kind, args of a host call, args of a device call): for a sphere (rgb, rgb_step, depth, depth_step, depth_type, rows,
    cols, convention), for a cloud (xyz, rgb3, n).  close() frees the device copies."""

    def __init__(self, reg):
        from rgbd360_amd import synth
        self.hip, self.keep, self.dev, self.forms = hip_runtime(), [], [], {}
        rgb, depth = synth.render(synth.trajectory_pose(0, 7), 1100, 24, 7)
        metres = depth.astype(np.float32) * 0.001 if depth.dtype == np.uint16 else depth.astype(np.float32)
        mm = depth if depth.dtype == np.uint16 else np.round(depth * 1000).astype(np.uint16)
        rows, cols = depth.shape
        d32, c8, d16 = padded_rows(metres, 64), padded_rows(rgb, 5), padded_rows(mm, 0)
        xyz, rgb3 = np.ascontiguousarray(reg.sphere_cloud(metres, 2)), np.ascontiguousarray(rgb.reshape(-1, 3))
        for where in (self.host, self.device):
            sphere = lambda c, d, t: (None if c is None else where(c), 0 if c is None else c.shape[1], where(d), d.shape[1], t, rows, cols, 2)
            self.forms.setdefault("f32_padded", ["sphere"]).append(sphere(c8, d32, 1))
            self.forms.setdefault("u16", ["sphere"]).append(sphere(None, d16, 0))
            self.forms.setdefault("cloud", ["cloud"]).append((where(xyz), where(rgb3), rows * cols))

    def host(self, a):
        self.keep.append(a)
        return vp(a)

    def device(self, a):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), a.nbytes) == 0 and self.hip.hipMemcpy(p, vp(a), a.nbytes, 1) == 0
        self.dev.append(p)
        return p

    def close(self):
        for p in self.dev:
            self.hip.hipFree(p)
        self.dev = []


def edit_on_both(L, reg, forms, name, op):
    """`op` (insert, remove or move) of form `name` into a fresh map that holds the form at POSE_A and at pose_b() (an empty one for
    insert), once from host and once from device memory: [(return code, the statistics' bytes, the map read out as bytes)] x 2."""
    from rgbd360_amd import _lib
    from rgbd360_amd.voxel_map import VoxelMap
    kind, host, dev = forms.forms[name]
    a, b = cm(POSE_A), cm(pose_b())
    out = []
    for on_device, args in ((0, host), (1, dev)):
        with VoxelMap(reg, LEAF, 1 << 14) as m:
            H, st, est = m._handle(), _lib.MapStats(), _lib.MapEditStats()
            ins = getattr(L, "rgbd360_map_insert_" + kind)
            if op == "insert":
                rc = ins(H, *args, vp(a), on_device, C.byref(st))
            else:
                assert ins(H, *host, vp(a), 0, C.byref(st)) == 0 and ins(H, *host, vp(b), 0, C.byref(st)) == 0
                if op == "remove":
                    rc = getattr(L, "rgbd360_map_remove_" + kind)(H, *args, vp(a), on_device, C.byref(est))
                else:
                    rc = getattr(L, "rgbd360_map_move_" + kind)(H, *args, vp(a), vp(cm(np.eye(4))), on_device, C.byref(est), C.byref(st))
            assert rc == 0 and len(m) > 200, (rc, L.rgbd360_map_last_error(H))
            out.append((rc, bytes(st) + bytes(est), b"".join(x.tobytes() for x in m.extract())))
    return out


def align_on_both(L, reg, forms, name, entry, params, result_type):
    """The align entry `entry` of sphere form `name` against a map that holds the form at POSE_A, from a guess 1 cm and 3 mrad off, once
    from host and once from device memory: [(return code, the pose's bytes, the result struct's bytes)] x 2."""
    from rgbd360_amd import _lib
    from rgbd360_amd.voxel_map import VoxelMap
    guess = cm(A.perturbed(POSE_A, 0.01, 0.003, 7))
    kind, host, dev = forms.forms[name]
    out = []
    with VoxelMap(reg, LEAF, 1 << 14) as m:
        H, st = m._handle(), _lib.MapStats()
        assert L.rgbd360_map_insert_sphere(H, *host, vp(cm(POSE_A)), 0, C.byref(st)) == 0
        for on_device, args in ((0, host), (1, dev)):
            pose, res = np.zeros(16, np.float32), result_type()
            rc = entry(H, *args[2:], vp(guess), on_device, C.byref(params), vp(pose), C.byref(res))
            assert rc == 0 and res.iterations >= 1 and res.n_matched > 1000, (rc, res.iterations, res.n_matched, L.rgbd360_map_last_error(H))
            out.append((rc, pose.tobytes(), bytes(res)))
    return out
