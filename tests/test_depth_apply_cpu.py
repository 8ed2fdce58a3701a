"""Applying the depth models without a GPU (rgbd360_depth_models_pack / _repack / _undistort_packed_host, rgbd360_hip_diag.h;
csrc/depth_apply.h): the scalar numpy restatement (tests/depth_apply_reference.py) equals rgbd360_depth_model_undistort byte for byte, and
so does the per-pixel text the kernels call, run on the host over the packed blob; sets with their sensors in another order agree per
sensor; a repacked blob is the freshly packed one; the two millimetre conversions differ and each is pinned; the evaluation's sums on a
hand-computed case; what the host entries refuse.

Models: the trainer's own shapes from rgbd360_depth_model_from_sums (slices below and at or above 50 examples alternate; smoothing 0 with
empty slices: multipliers of exactly 1), a written file whose frustums differ in num_bins and bin_depth, and the reference's
distortion_model1 after downsample 2 (320 x 240).  Images: tests/depth_apply_reference.depth_image."""
import ctypes as C

import numpy as np
import pytest

import depth_apply_reference as A
from rgbd360_amd import _lib
from rgbd360_amd.register import DepthModel

F = np.float32


def loaded(tmp_path, name, raw, downsample=1):
    """(DepthModel, the restatement's model) of a file's bytes."""
    path = tmp_path / name
    path.write_bytes(raw)
    return DepthModel(path, downsample), A.read_model(path, downsample)


def from_sums(tmp_path, shape, smoothing, seed, spread=0.1):
    m = DepthModel.from_sums(*shape, 2.0, smoothing, *A.sums_for(shape, smoothing, seed, spread))
    path = tmp_path / ("sums_%d_%d_%d_%g" % (shape[0], smoothing, seed, spread))
    m.save(path)
    return m, A.read_model(path)


def pack(models):
    """The blob of a list of DepthModel-or-None, as a uint8 array."""
    L = _lib.load()
    arr = (C.c_void_p * len(models))(*[None if m is None else m._h for m in models])
    n = C.c_size_t()
    assert L.rgbd360_depth_models_pack(arr, len(models), None, C.byref(n)) == 0
    blob = np.zeros(n.value, np.uint8)
    room = C.c_size_t(n.value)
    assert L.rgbd360_depth_models_pack(arr, len(models), blob.ctypes.data, C.byref(room)) == 0 and room.value == n.value
    return blob


def packed_undistort(blob, sensor, depth):
    z = np.ascontiguousarray(depth, F).copy()
    assert _lib.load().rgbd360_depth_models_undistort_packed_host(blob.ctypes.data, sensor, z.ctypes.data, z.strides[0], z.shape[0], z.shape[1]) == 0
    return z


def all_models(tmp_path):
    """[(name, DepthModel, restatement model)] of every model the tests use."""
    out = []
    for shape in A.SHAPES:
        for smoothing in (1, 0):
            out.append(("sums %s smoothing %d" % (shape, smoothing),) + from_sums(tmp_path, shape, smoothing, 3))
    out.append(("varied",) + loaded(tmp_path, "varied", A.varied_model_bytes(A.SHAPES[1], 9)))
    out.append(("distortion_model1",) + loaded(tmp_path, "golden1", A.golden_model_bytes(1), 2))
    return out


def test_restatement_host_and_packed_text_agree_byte_for_byte(tmp_path):
    for name, model, ref in all_models(tmp_path):
        depth = A.depth_image(ref, 17)
        want = A.undistort(ref, depth)
        host = model.undistort(depth)
        assert host.tobytes() == want.tobytes(), name
        blob = pack([None, model])
        assert packed_undistort(blob, 1, depth).tobytes() == want.tobytes(), name
        assert packed_undistort(blob, 0, depth).tobytes() == depth.tobytes(), name          # a NULL model: identity, payloads included
        changed = (host.view(np.uint32) != depth.view(np.uint32)).mean()
        print("%-36s %3d x %3d: %.0f %% of the pixels corrected, blob %d bytes" % (name, ref["width"], ref["height"], 100 * changed, blob.size))
        assert changed > 0.3 or "smoothing 0" in name
        # the specials: 0, -1 and the NaN keep their bits, +Inf takes the fall-back branch
        tail = slice(depth.size - 9, depth.size)
        assert host.ravel()[tail][4:7].tobytes() == depth.ravel()[tail][4:7].tobytes() and np.isnan(depth.ravel()[tail][6])
        assert host.ravel()[tail][7] == np.inf or np.isnan(host.ravel()[tail][7])
    # both branches and the D == 0 multipliers are there
    _, ref = from_sums(tmp_path, A.SHAPES[0], 0, 3)
    counts = np.concatenate([f[2] for f in ref["frustums"]])
    mult = np.concatenate([f[3] for f in ref["frustums"]])
    assert (counts < 50).mean() > 0.3 and (counts >= 50).mean() > 0.3 and (mult[counts == 0] == 1).all() and (counts == 0).any()
    _, ref = loaded(tmp_path, "varied2", A.varied_model_bytes(A.SHAPES[1], 9))
    assert len({f[1] for f in ref["frustums"]}) >= 5 and len({f[0] for f in ref["frustums"]}) >= 4


def test_sets_in_another_order_agree_per_sensor(tmp_path):
    shape = A.SHAPES[1]
    models = [from_sums(tmp_path, shape, 1, 5), from_sums(tmp_path, shape, 0, 6), loaded(tmp_path, "v", A.varied_model_bytes(shape, 9))]
    order_a, order_b = [0, 1, None, 2], [2, None, 0, 1]
    blob_a = pack([None if k is None else models[k][0] for k in order_a])
    blob_b = pack([None if k is None else models[k][0] for k in order_b])
    assert blob_a.size == blob_b.size and blob_a.tobytes() != blob_b.tobytes()
    depth = A.depth_image(models[0][1], 23)
    for k in (0, 1, 2, None):
        a, b = packed_undistort(blob_a, order_a.index(k), depth), packed_undistort(blob_b, order_b.index(k), depth)
        want = depth if k is None else A.undistort(models[k][1], depth)
        assert a.tobytes() == b.tobytes() == want.tobytes(), k


def test_a_repacked_blob_is_the_freshly_packed_one(tmp_path):
    L = _lib.load()
    shape = A.SHAPES[0]
    a, b, c = (from_sums(tmp_path, shape, 1, s)[0] for s in (1, 2, 3))
    v = loaded(tmp_path, "v", A.varied_model_bytes(shape, 4))[0]         # another section size
    blob = pack([a, None, b])
    for sensor, new, want in ((1, c, [a, c, b]), (0, None, [None, None, b]), (2, v, [a, None, v]), (0, v, [v, None, b])):
        n = C.c_size_t()
        assert L.rgbd360_depth_models_repack(blob.ctypes.data, sensor, None if new is None else new._h, None, C.byref(n)) == 0
        out = np.zeros(n.value, np.uint8)
        assert L.rgbd360_depth_models_repack(blob.ctypes.data, sensor, None if new is None else new._h, out.ctypes.data, C.byref(n)) == 0
        assert out.tobytes() == pack(want).tobytes(), sensor


def test_the_two_millimetre_conversions_differ_and_each_is_pinned():
    raw = np.arange(1, 65536, dtype=np.uint16)
    a, b = A.metres_convert_to(raw), A.metres_map_entries(raw)
    differ = raw[a != b]
    print("the conversions differ for %d of 65535 raw values; the first: %s" % (len(differ), differ[:4].tolist()))
    assert len(differ) == 38850 and differ[:4].tolist() == [5, 9, 10, 11]
    # the first is correctly rounded (half a float32 step); the second carries 0.001f's error (2^-24 relative: a step at the most) and its
    # own rounding (half a step): two steps of 2^-17, the step below 128 m, at the most
    assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= 2.0 ** -16
    # pinned: (float)(0.001 * (double)raw) for the stand-alone undistort, 0.001f * (float)raw for the cloud and map entries
    assert A.metres_convert_to([5])[0] == F(0.005) and A.metres_map_entries([5])[0] == F(0.001) * F(5) != F(0.005)
    assert A.metres_convert_to([65535])[0] == F(65.535) and A.metres_convert_to([0])[0] == 0 and A.metres_map_entries([0])[0] == 0


def test_the_evaluation_sums_on_a_hand_computed_case():
    """gt 1, 2, 4; meas 1.5, 2, 3.75; corrected 1.25, 2.5, 4: e_raw 0.5, 0, -0.25 and e_cor 0.25, 0.5, 0, all exact in binary."""
    got = A.eval_terms([1.0, 2.0, 4.0], [1.5, 2.0, 3.75], [1.25, 2.5, 4.0])
    assert got == dict(n=3, raw_e=1 << 28, raw_ee=(1 << 28) + (1 << 26), cor_e=3 << 28, cor_ee=(1 << 26) + (1 << 28))
    # rounding to nearest, ties to even, per term: 2^-31 -> 0, 3 2^-31 -> 2
    assert A.eval_terms([0.0], [2.0 ** -31], [3 * 2.0 ** -31]) == dict(n=1, raw_e=0, raw_ee=0, cor_e=2, cor_ee=0)
    a, b = A.eval_terms([1.0], [1.5], [1.25]), A.eval_terms([2.0, 4.0], [2.0, 3.75], [2.5, 4.0])
    assert A.add_sums(a, b) == got


def test_refusals(tmp_path):
    L = _lib.load()
    small, _ = from_sums(tmp_path, A.SHAPES[2], 1, 1)
    big, ref = from_sums(tmp_path, A.SHAPES[0], 1, 1)
    n = C.c_size_t(12345)
    arr = lambda ms: (C.c_void_p * max(len(ms), 1))(*[None if m is None else m._h for m in ms])
    assert L.rgbd360_depth_models_pack(arr([small, big]), 2, None, C.byref(n)) == -1          # two widths x heights
    assert L.rgbd360_depth_models_pack(arr([]), 0, None, C.byref(n)) == -1
    assert L.rgbd360_depth_models_pack(arr([None] * 17), 17, None, C.byref(n)) == -1
    assert L.rgbd360_depth_models_pack(None, 1, None, C.byref(n)) == -1 and L.rgbd360_depth_models_pack(arr([big]), 1, None, None) == -1
    assert n.value == 12345
    assert L.rgbd360_depth_models_pack(arr([None] * 16), 16, None, C.byref(n)) == 0 and n.value > 0      # sixteen identities: a set
    blob = pack([big, None])
    short = np.zeros(blob.size - 1, np.uint8)
    room = C.c_size_t(short.size)
    assert L.rgbd360_depth_models_pack(arr([big, None]), 2, short.ctypes.data, C.byref(room)) == -1 and not short.any()
    for sensor, model in ((2, big), (-1, big), (1, small)):
        assert L.rgbd360_depth_models_repack(blob.ctypes.data, sensor, model._h, None, C.byref(n)) == -1
    assert L.rgbd360_depth_models_repack(None, 0, big._h, None, C.byref(n)) == -1
    junk = np.zeros(blob.size, np.uint8)
    assert L.rgbd360_depth_models_repack(junk.ctypes.data, 0, big._h, None, C.byref(n)) == -1
    depth = A.depth_image(ref, 1)
    z = depth.copy()
    call = lambda b, s, a, step, rows, cols: L.rgbd360_depth_models_undistort_packed_host(None if b is None else b.ctypes.data, s, None if a is None else a.ctypes.data,
                                                                                           step, rows, cols)
    assert call(None, 0, z, z.strides[0], *z.shape) == -1 and call(junk, 0, z, z.strides[0], *z.shape) == -1
    assert call(blob, 2, z, z.strides[0], *z.shape) == -1 and call(blob, -1, z, z.strides[0], *z.shape) == -1
    assert call(blob, 0, None, z.strides[0], *z.shape) == -1 and call(blob, 0, z, z.strides[0] - 4, *z.shape) == -1
    assert call(blob, 0, z, z.strides[0], z.shape[0] - 1, z.shape[1]) == -1              # not the set's size
    assert z.tobytes() == depth.tobytes()
    assert call(blob, 1, z, z.strides[0], z.shape[0] - 1, z.shape[1]) == 0 and z.tobytes() == depth.tobytes()      # identity: any size
