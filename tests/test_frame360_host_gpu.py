"""The host code in front of the Frame360 kernels (rgbd360_frame360.hip): every route of the normal-map dispatch -- the tiled kernel alone
for windows under 3 px, one sweep instantiation per window size 3 .. 9 -- and the lifetime of a context's scratch buffers when the
frame size grows, shrinks and other stages run in between."""
import ctypes as C

import numpy as np
import pytest

from rgbd360_amd import synth

pytestmark = pytest.mark.gpu

W_RAGGED, H_RAGGED = 250, 101       # partial 32 x 16 tiles (250 = 7 x 32 + 26, 101 = 6 x 16 + 5), partial sweep strips (63 - R columns each)

# normal_smoothing_size -> components of valid normals that differ from the oracle's, of how many (depth_mode 1; (size, 0): depth_mode 0).
# Measured on the build before the host dispatch was rewritten (docs/HISTORY.md); the result is deterministic, so the count is asserted
# without a margin: at this size every component is equal at every window size.
MISMATCHES = {
    (1.0, 1): (0, 67212), (2.0, 1): (0, 65142), (3.0, 1): (0, 63096), (4.0, 1): (0, 61074), (4.5, 1): (0, 61074), (5.0, 1): (0, 59076),
    (6.0, 1): (0, 57102), (7.0, 1): (0, 55152), (9.0, 1): (0, 51414), (9.5, 1): (0, 51414), (3.0, 0): (0, 64104), (9.5, 0): (0, 52422),
}


def _ragged_room(oracle_mod, far=1):
    """tests/test_gpu_parity.py's _room_cloud at 250 x 101: a hole and a box in front of the wall (the box moved up into the 101 rows).
    far: the room scaled -- PCL's window is min(distance to a depth change, smoothing size + depth / 10) and must exceed 2 px, so a
    smoothing size of 1.0 leaves normals only beyond 10 m."""
    (_, dA), _, _ = synth.make_pair(W_RAGGED, H_RAGGED, seed=5)
    d = (dA.astype(np.uint32) * far).astype(np.uint16)
    d[60:90, 200:230] = 0
    d[15:40, 60:110] = (d[15:40, 60:110] * 0.7).astype(np.uint16)
    return oracle_mod.sphere_cloud(d, 2)


_clouds, _refs = {}, {}


def _case(oracle_mod, size, depth_mode):
    """(cloud, oracle normals) of one case, computed once"""
    far = 8 if size < 2.0 else 1
    if far not in _clouds:
        _clouds[far] = _ragged_room(oracle_mod, far)
    key = (size, depth_mode)
    if key not in _refs:
        _refs[key] = oracle_mod.f360_normals(_clouds[far], H_RAGGED, W_RAGGED, 0.05, size, depth_mode)[0]
    return _clouds[far], _refs[key]


def _stages(hip_lib):
    from rgbd360_amd.register import Frame360Stages, RegisterPhotoICP
    reg = RegisterPhotoICP()
    reg.setNumPyr(2)
    return Frame360Stages(reg)


WINDOW_CASES = [(s, 1) for s in (1.0, 2.0, 3.0, 4.0, 4.5, 5.0, 6.0, 7.0, 9.0, 9.5)] + [(3.0, 0), (9.5, 0)]


@pytest.mark.parametrize("size,depth_mode", WINDOW_CASES)
def test_normal_map_every_window_size(hip_lib, oracle_mod, size, depth_mode):
    """test_normal_map_matches_oracle's assertions at every window size the launcher tells apart (that test runs 8.0 alone)."""
    xyz, ref = _case(oracle_mod, size, depth_mode)
    ok = ~np.isnan(ref[:, 0])
    assert ok.mean() > 0.3                          # (of the oracle alone: the input is worth comparing)
    nrm = _stages(hip_lib).normals(xyz, H_RAGGED, W_RAGGED, 0.05, size, depth_mode)
    assert np.array_equal(np.isnan(nrm[:, 0]), ~ok)
    diff = np.abs(nrm[ok] - ref[ok]).max()
    n_diff, n_all = int((nrm[ok] != ref[ok]).sum()), int(ok.sum()) * 3
    print("normal_smoothing_size %.1f depth_mode %d: valid share %.4f, max |diff| %.3g, %d of %d components differ"
          % (size, depth_mode, ok.mean(), diff, n_diff, n_all))
    assert diff <= 1.2e-7                           # two float32 ulps of a unit-vector component
    want_diff, want_all = MISMATCHES[(size, depth_mode)]
    assert n_all == want_all and n_diff <= want_diff


@pytest.mark.parametrize("size", [10.0, 0.5])
def test_normal_map_refuses_windows_out_of_range(hip_lib, oracle_mod, size):
    from rgbd360_amd.register import Rgbd360Error
    xyz, _ = _case(oracle_mod, 3.0, 1)
    with pytest.raises(Rgbd360Error, match=r"\(-1\): normal_smoothing_size out of range"):
        _stages(hip_lib).normals(xyz, H_RAGGED, W_RAGGED, 0.05, size, 1)


# ---- one context across frame sizes and stages ---------------------------------------------------------------------------------------
def _frame_planes_raw(st, depth, rgb):
    """rgbd360_frame_planes with `rgb` registered: (plane records as raw bytes, labels, normals, xyz)"""
    from rgbd360_amd import _lib
    from rgbd360_amd.register import _ptr
    st.set_color_image(rgb)
    d = np.ascontiguousarray(depth, np.uint16)
    rows, cols = d.shape
    xyz, nrm = np.empty((rows * cols, 3), np.float32), np.empty((rows * cols, 3), np.float32)
    labels = np.empty(rows * cols, np.int32)
    arr, n = (_lib.Plane * 256)(), C.c_int()
    st._reg._check(st._L.rgbd360_frame_planes(st._reg._ctx(), _ptr(d), d.strides[0], 0, rows, cols, 2, 0.05, 8.0, 40, 0.03, 0.05, 0.001, 1,
                                              _ptr(xyz), _ptr(nrm), _ptr(labels), C.cast(arr, C.c_void_p), 256, C.byref(n)))
    return bytes(arr)[: n.value * C.sizeof(_lib.Plane)], labels, nrm, xyz


def _sensor_planes_raw(st, depth, rgb):
    from rgbd360_amd import _lib
    from rgbd360_amd.register import _ptr
    st.set_color_image(rgb, step=2)
    d = np.ascontiguousarray(depth, np.uint16)
    rows, cols = d.shape
    arr, n = (_lib.Plane * 256)(), C.c_int()
    st._reg._check(st._L.rgbd360_sensor_planes(st._reg._ctx(), _ptr(d), d.strides[0], rows, cols, 2, 0.3, 10.0, 10.0, 0.05, 0.02, 8.0, 40, 0.0398,
                                               0.02, 0.0013, None, C.cast(arr, C.c_void_p), 256, C.byref(n)))
    return (bytes(arr)[: n.value * C.sizeof(_lib.Plane)],)


def _same_bytes(a, b):
    return len(a) == len(b) and all(x == y if isinstance(x, bytes) else np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_context_regrows_and_is_reused(hip_lib):
    """One context (refinement on, a colour image per frame) through 256 x 128 -> 512 x 256 -> 256 x 128 frames with the bilateral filter,
    a sensor's planes and the stitcher in between: every output equals, byte for byte, that of the same call on a context of its own."""
    from rgbd360_amd import _lib
    from rgbd360_amd.register import Rgbd360Error, RegisterPhotoICP, stitch_sphere
    from tests.test_gpu_parity import _fake_rig
    from tests.test_oracle_cpu import _noisy_pinhole_cloud
    (rgb_s, d_s), _, _ = synth.make_pair(256, 128, seed=31)
    (rgb_l, d_l), _, _ = synth.make_pair(512, 256, seed=31)
    (rgb_p, d_p), _, _, _ = synth.make_pinhole_pair(128, 96, seed=3)
    cloud, _ = _noisy_pinhole_cloud(97, 131, seed=97 + 131)
    rig = _fake_rig()

    def fresh():
        st = _stages(hip_lib)
        st.set_refinement(True, 0.02)
        return st

    steps = [lambda st: _frame_planes_raw(st, d_s, rgb_s),
             lambda st: (st.bilateral_filter(cloud, 97, 131, 7.0, 0.03),),
             lambda st: _frame_planes_raw(st, d_l, rgb_l),
             lambda st: _sensor_planes_raw(st, d_p, rgb_p),
             lambda st: stitch_sphere(st._reg, *rig),
             lambda st: _frame_planes_raw(st, d_s, rgb_s)]
    one = fresh()
    got = [step(one) for step in steps]
    for k, step in enumerate(steps):
        alone = fresh()
        assert _same_bytes(got[k], step(alone)), k
        alone._reg.close()
    one._reg.close()
    assert _same_bytes(got[0], got[5])
    n_planes = [len(got[k][0]) // C.sizeof(_lib.Plane) for k in (0, 2, 3)]
    print("planes: 256 x 128: %d, 512 x 256: %d, sensor 96 x 128 / 2: %d" % tuple(n_planes))
    assert n_planes[0] >= 2 and n_planes[1] >= 5 and n_planes[2] >= 1                      # the records compared are not empty lists
    assert np.isfinite(got[1][0]).any() and (got[4][1] > 0).any()
    # a context that never made a Frame360 call, and one whose only call was refused, are destroyed like any other
    reg = RegisterPhotoICP()
    reg._ctx()
    reg.close()
    st = _stages(hip_lib)
    with pytest.raises(Rgbd360Error, match=r"\(-1\): bad image size"):
        st.normals(np.zeros((4, 3), np.float32), 2, 2)
    st._reg.close()
