"""Free-space observation and carving of the voxel map (rgbd360_map_observe_* / _votes / _carve, csrc/map_carve.h) on the device against
the numpy restatement of its definition (tests/map_carve_reference.py), bit for bit: the votes (keys, through, end, count), every statistic
(n_lookups for both forms of the walk), and the map after carving (extract, size, census); then what follows a carve -- the ordering of
the calls, the derived layers, rehash, the contract with exact removal -- the refusals, and the C++ adapter.

Shapes: lists of 1 .. 2 000 segments against a blob of ~5 000 voxels in a 2^14-slot table; 64 x 32 and 256 x 128 frames of the synthetic
room under SMALL_BOX (the observation does not apply the box: most of its measurements end outside the map) in 2^15-slot tables."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_carve_reference as V
import map_normals_reference as N
import map_raycast_reference as M
import voxel_map_reference as R
from test_map_carve_cpu import blob, segments

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
F = np.float32
LEAF = 0.05
SMALL_BOX = (np.array([-2.0, -1.3, -1.3], F), np.array([2.0, 1.3, 1.3], F))
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def new_map(reg, capacity=1 << 14, box=None):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, LEAF, capacity)
    m.set_box(*(box if box is not None else (None, None)))
    return m


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def blob_map(reg):
    """The blob of tests/test_map_carve_cpu.py in a 2^14-slot table, with the restatement's map; shared and never written."""
    pts, ref = blob()
    assert 4000 < len(ref) < 6000 and ref.key.min() < -15 and ref.key.max() > 15
    m = new_map(reg)
    m.insert_cloud(pts, None, EYE)
    assert not m.full and len(m) == len(ref)
    yield m, ref, pts
    m.close()


def with_invalid(o, w):
    """Every seventh segment made invalid, one way after the other."""
    o, w = o.copy(), w.copy()
    for j in range(3, len(o), 7):
        which = (j // 7) % 5
        if which == 0:
            w[j] = o[j]
        elif which == 1:
            w[j, 1] = np.nan
        elif which == 2:
            o[j, 2] = np.inf
        elif which == 3:
            w[j, 0] = 5000.0
        else:
            o[j, 0] = -np.nan
    return o, w


@pytest.mark.parametrize("n", [1, 63, 65, 257, 2000])
def test_ray_lists_equal_the_restatement(hip_lib, hip, blob_map, n):
    from rgbd360_amd import _lib
    m, ref, pts = blob_map
    o, w = with_invalid(*segments(n, pts, seed=20 + n))
    for params in ({}, dict(margin_leaves=1.0, margin_rel=0.05, max_offset=0.8, near=0.2, min_count=2, max_steps=30)):
        want = V.observe_rays(ref, LEAF, o, w, **params)
        stats = m.observe_rays(o, w, **params)
        print(n, params, stats)
        V.assert_observation_equals(stats, m.votes(), ref, want, "%d %s" % (n, params))
    if n == 2000:          # many segments share voxels (the atomics contend), some are invalid, some end on the step limit
        assert want["through"].max() > 3 and want["stats"]["n_skipped"] > 200 and want["stats"]["n_max_steps"] > 100 and want["stats"]["n_end"] > 100
    # device arrays give what host arrays give
    want = V.observe_rays(ref, LEAF, o, w)
    dev = [C.c_void_p(), C.c_void_p()]
    for p, a in zip(dev, (o, w)):
        assert hip.hipMalloc(C.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, vp(a), a.nbytes, 1) == 0
    st = _lib.MapObserveStats()
    rc = hip_lib.rgbd360_map_observe_rays(m._handle(), n, dev[0], dev[1], 1, None, C.byref(st))
    for p in dev:
        hip.hipFree(p)
    assert rc == 0
    V.assert_observation_equals({k: getattr(st, k) for k in V.STAT_NAMES}, m.votes(), ref, want, "on_device %d" % n)
    assert m.vote_bytes() == 8 * (1 << 14) and len(m) == len(ref)


def test_the_layered_walk_equals_the_plain_walk(blob_map):
    m, ref, pts = blob_map
    o, w = with_invalid(*segments(2000, pts, seed=7))
    layered_stats = m.observe_rays(o, w)
    layered = m.votes()
    m.raycast_set_plain(True)
    try:
        plain_stats = m.observe_rays(o, w)
        plain = m.votes()
    finally:
        m.raycast_set_plain(False)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(layered, plain))
    assert {k: v for k, v in layered_stats.items() if k != "n_lookups"} == {k: v for k, v in plain_stats.items() if k != "n_lookups"}
    assert plain_stats["n_lookups"] == plain_stats["n_steps"] > 10 * layered_stats["n_lookups"] > 0
    V.assert_observation_equals(layered_stats, layered, ref, V.observe_rays(ref, LEAF, o, w), "layered")
    V.assert_observation_equals(plain_stats, plain, ref, V.observe_rays(ref, LEAF, o, w, layer=False), "plain")


def phantom_points(pose, n=20000, seed=5):
    """A 0.3 m cube of points in the room's free space, 0.7 m from `pose`: what no frame contains."""
    rng = np.random.default_rng(seed)
    mid = np.asarray(pose, np.float64)[:3, 3] + np.array([0.2, 0.4, 0.5])
    return (mid[None, :] + rng.uniform(-0.15, 0.15, size=(n, 3))).astype(F)


@pytest.fixture(scope="module")
def room(reg):
    """Per size: three frames of the synthetic room along its trajectory, as uint16 and as spoiled float32 depth, and their true poses."""
    from rgbd360_amd import synth
    out = {}
    for width, height in ((64, 32), (256, 128)):
        poses = [synth.trajectory_pose(k).astype(F) for k in range(3)]
        u16 = [synth.render(synth.trajectory_pose(k), width, height) for k in range(3)]
        f32 = [synth.spoil_depth(synth.render(synth.trajectory_pose(k), width, height, depth_f32=True)[1], seed=k) for k in range(3)]
        out[(height, width)] = dict(poses=poses, u16=u16, f32=f32)
    return out


def fill_room(reg, room, size, extra=()):
    """Frames 0-2 (uint16, convention 2) under SMALL_BOX and the clouds of `extra` [(xyz, pose), ...] in a 2^15-slot table: (map, ref, frames
    as the restatement takes them)."""
    scene = room[size]
    frames = [(reg.sphere_cloud(scene["u16"][k][1], 2), scene["u16"][k][0].reshape(-1, 3), scene["poses"][k]) for k in range(3)]
    frames += [(xyz, None, pose) for xyz, pose in extra]
    ref = R.Map(frames, LEAF, SMALL_BOX)
    m = new_map(reg, 1 << 15, SMALL_BOX)
    for k in range(3):
        m.insert_sphere(scene["u16"][k][0], scene["u16"][k][1], scene["poses"][k], convention=2)
    for xyz, pose in extra:
        m.insert_cloud(xyz, None, pose)
    assert not m.full and len(m) == len(ref) < 0.8 * (1 << 15)
    return m, ref, frames


SPHERE_CASES = [((32, 64), 0, "u16"), ((32, 64), 2, "f32"), ((128, 256), 2, "u16"), ((128, 256), 0, "f32")]


@pytest.mark.parametrize("size,convention,kind", SPHERE_CASES, ids=["64x32-c0-u16", "64x32-c2-f32", "256x128-c2-u16", "256x128-c0-f32"])
def test_sphere_frames_equal_the_restatement(reg, room, size, convention, kind):
    """The room with a phantom box, observed by frame 1 in either convention (convention 0 reads the same depth image as another sphere: its
    rays still cross the map), uint16 depth or float32 depth with NaN, Inf, negative, zero and far pixels."""
    scene = room[size]
    m, ref, _ = fill_room(reg, room, size, [(phantom_points(scene["poses"][1]), EYE)])
    with m:
        depth = scene["u16"][1][1] if kind == "u16" else scene["f32"][1]
        cloud = reg.sphere_cloud(depth, convention)
        for params in ({}, dict(margin_leaves=4.0, max_offset=np.inf, min_count=3)):
            want = V.observe_cloud(ref, LEAF, cloud, scene["poses"][1], **params)
            stats = m.observe_sphere(depth, scene["poses"][1], convention=convention, **params)
            print(size, convention, kind, params, stats)
            V.assert_observation_equals(stats, m.votes(), ref, want, str(params))
        base = V.observe_cloud(ref, LEAF, cloud, scene["poses"][1])["stats"]
        assert base["n_through"] > (100 if size[0] == 32 else 2000) and base["n_steps"] > 20 * size[0] * size[1]
        if kind == "f32":
            assert base["n_skipped"] > size[0] * size[1] // 60
        if convention == 2 and kind == "u16":          # the frame is in the map: it protects what it measures inside the box
            assert base["n_end"] > size[0] * size[1] // 8


def test_two_frames_accumulate_to_the_restated_sum(reg, room):
    size = (32, 64)
    scene = room[size]
    m, ref, frames = fill_room(reg, room, size, [(phantom_points(scene["poses"][1]), EYE)])
    with m:
        a = V.observe_cloud(ref, LEAF, frames[0][0], scene["poses"][0])
        b = V.observe_cloud(ref, LEAF, frames[2][0], scene["poses"][2])
        m.observe_sphere(scene["u16"][0][1], scene["poses"][0], convention=2)
        stats = m.observe_sphere(scene["u16"][2][1], scene["poses"][2], convention=2, accumulate=True)
        both = V.add(a, b)
        assert both["stats"]["n_voxels_voted"] > 0 and (both["through"] > np.maximum(a["through"], b["through"])).any()
        V.assert_observation_equals(stats, m.votes(), ref, both, "accumulated")
        # without `accumulate` the second call starts again
        stats = m.observe_sphere(scene["u16"][2][1], scene["poses"][2], convention=2)
        V.assert_observation_equals(stats, m.votes(), ref, b, "fresh")
        # accumulate on a map without votes starts them
        m.release_votes()
        assert m.vote_bytes() == 0
        stats = m.observe_sphere(scene["u16"][0][1], scene["poses"][0], convention=2, accumulate=True)
        V.assert_observation_equals(stats, m.votes(), ref, a, "accumulate from nothing")


def test_carve_and_what_follows(reg, room):
    from rgbd360_amd.register import Rgbd360Error
    from test_map_normals_gpu import assert_normals_equal
    size = (128, 256)
    scene = room[size]
    phantom = phantom_points(scene["poses"][1])
    m, ref, frames = fill_room(reg, room, size, [(phantom, EYE)])
    with m:
        ob = V.observe_cloud(ref, LEAF, frames[1][0], scene["poses"][1])
        erased, want = V.carve(ref, ob)
        room_only = R.Map(frames[:3], LEAF, SMALL_BOX)
        is_phantom = ~np.isin(M.packed_keys(ref.key), M.packed_keys(room_only.key))
        print("phantom voxels %d erased %.3f; room voxels %d erased %.4f" % (is_phantom.sum(), erased[is_phantom].mean(), (~is_phantom).sum(),
                                                                              erased[~is_phantom].mean()))
        assert erased[is_phantom].mean() > 0.9 and erased[~is_phantom].mean() < 0.005
        before = m.census()
        m.observe_sphere(scene["u16"][1][1], scene["poses"][1], convention=2)
        got = m.carve()
        print(got)
        assert got == want and len(m) == want["n_voxels"]
        carved = V.without(ref, erased)
        R.assert_map_equals(m.extract(), carved, "after the carve")
        c = m.census()
        assert c["n_tombstones"] == before["n_tombstones"] + want["n_voxels_carved"] and c["n_points"] == before["n_points"] - want["n_points_carved"]
        assert (c["n_live"], c["n_inconsistent"]) == (len(carved), 0)
        # ordering: the votes are spent but readable, with count 0 on the carved voxels
        with pytest.raises(Rgbd360Error):
            m.carve()
        with pytest.raises(Rgbd360Error):
            m.observe_sphere(scene["u16"][1][1], scene["poses"][1], convention=2, accumulate=True)
        key3, through, end, count = m.votes()
        wk, wt, we, wc = V.votes(ref, ob, erased)
        assert np.array_equal(key3, wk) and np.array_equal(through, wt) and np.array_equal(end, we) and np.array_equal(count, wc)
        assert int((count == 0).sum()) == want["n_voxels_carved"]
        # the derived layers follow the carve
        pose = scene["poses"][2]
        M.assert_sphere_equals(m.raycast_sphere(32, 64, pose), M.cast_sphere(carved, LEAF, 32, 64, pose), "ray cast of the carved map")
        assert_normals_equal(m.normals(), N.normals(carved), "normals of the carved map")
        carved2 = carved
        # an insert makes the votes stale
        m.observe_sphere(scene["u16"][0][1], scene["poses"][0], convention=2)
        m.insert_cloud(phantom[:10], None, EYE)
        for call in (m.votes, m.carve, lambda: m.observe_sphere(scene["u16"][0][1], scene["poses"][0], convention=2, accumulate=True)):
            with pytest.raises(Rgbd360Error):
                call()
        m.remove_cloud(phantom[:10], None, EYE)
        assert not m.mismatch
        # rehash drops the tombstones and frees the vote array
        assert m.vote_bytes() == 8 * (1 << 15)
        m.rehash()
        c = m.census()
        assert m.vote_bytes() == 0 and (c["n_tombstones"], c["n_live"], c["n_inconsistent"]) == (0, len(carved2), 0)
        R.assert_map_equals(m.extract(), carved2, "after the rehash")
        with pytest.raises(Rgbd360Error):
            m.votes()


@pytest.mark.parametrize("thresholds", [dict(min_through=2), dict(max_count=4), dict(min_through=2, max_end=1, max_count=8)], ids=["min_through", "max_count", "all"])
def test_carve_thresholds_on_the_blob(reg, thresholds):
    pts, ref = blob()
    o, w = segments(600, pts)
    ob = V.observe_rays(ref, LEAF, o, w)
    erased, want = V.carve(ref, ob, **thresholds)
    assert 0 < want["n_voxels_carved"] < V.carve(ref, ob)[1]["n_voxels_carved"]          # the thresholds bite
    with new_map(reg) as m:
        m.insert_cloud(pts, None, EYE)
        m.observe_rays(o, w)
        assert m.carve(**thresholds) == want
        R.assert_map_equals(m.extract(), V.without(ref, erased), str(thresholds))
        c = m.census()
        assert (c["n_live"], c["n_tombstones"], c["n_points"], c["n_inconsistent"]) == (want["n_voxels"], want["n_voxels_carved"],
                                                                                        int(ref.count.sum()) - want["n_points_carved"], 0)


def test_removing_a_frame_that_fed_carved_voxels_reports_the_mismatch(reg, room):
    """Frame 2 goes in at a pose 0.4 m off (a ghost of the room), frame 1 looks through the ghost and carves; removing frame 2 at the pose it
    went in at then finds its points in the carved voxels gone."""
    from rgbd360_amd.voxel_map import MAP_MISMATCH
    size = (128, 256)
    scene = room[size]
    wrong = scene["poses"][2].copy()
    wrong[:3, 3] += np.array([0.1, 0.4, -0.3], F)
    clouds = [reg.sphere_cloud(scene["u16"][k][1], 2) for k in range(3)]
    kept = [(clouds[k], scene["u16"][k][0].reshape(-1, 3), scene["poses"][k]) for k in range(2)]
    ghost = (clouds[2], scene["u16"][2][0].reshape(-1, 3), wrong)
    ref = R.Map(kept + [ghost], LEAF, SMALL_BOX)
    with new_map(reg, 1 << 15, SMALL_BOX) as m:
        for k, pose in enumerate((scene["poses"][0], scene["poses"][1], wrong)):
            m.insert_sphere(scene["u16"][k][0], scene["u16"][k][1], pose, convention=2)
        assert not m.full and len(m) == len(ref)
        ob = V.observe_cloud(ref, LEAF, clouds[1], scene["poses"][1])
        erased, want = V.carve(ref, ob)
        lost = V.points_in(ref, erased, ghost[0], wrong, LEAF, SMALL_BOX)
        print(want, "points of the ghost frame in carved voxels:", lost)
        assert want["n_voxels_carved"] > 100 and lost > 100
        m.observe_sphere(scene["u16"][1][1], scene["poses"][1], convention=2)
        assert m.carve() == want
        st = m.remove_sphere(scene["u16"][2][0], scene["u16"][2][1], wrong, convention=2)
        print(st)
        passing = R.Map([ghost], LEAF, SMALL_BOX).n_passing
        assert m.last_status == MAP_MISMATCH and m.mismatch
        assert (st["n_underflow"], st["n_missing"], st["n_removed"]) == (lost, 0, passing - lost)
        assert m.census()["n_inconsistent"] == 0
        rest = R.Map(kept, LEAF, SMALL_BOX)
        rest = V.without(rest, np.isin(M.packed_keys(rest.key), M.packed_keys(ref.key[erased])))
        R.assert_map_equals(m.extract(), rest, "all other voxels")


def test_refusals_and_empty_inputs(hip_lib, reg, blob_map):
    """Nothing is launched: the return code, the message, the statistics zero-filled on an empty input and untouched on a refusal, the
    votes as they were."""
    from rgbd360_amd import _lib
    m, ref, pts = blob_map
    H = m._handle()
    o, w = segments(10, pts)
    stats0 = m.observe_rays(o, w)
    votes0 = m.votes()
    depth = np.ones((4, 8), F)
    pose = np.ascontiguousarray(EYE.reshape(16))

    def fresh(t=_lib.MapObserveStats):
        st = t()
        C.memset(C.byref(st), SENTINEL, C.sizeof(st))
        return st

    def params(**fields):
        return C.byref(m.observe_params(**fields))

    def rays(n=10, oo=o, ww=w, p=None, st=None):
        return hip_lib.rgbd360_map_observe_rays(H, n, vp(oo), vp(ww), 0, p, None if st is None else C.byref(st))

    def sphere(d=depth, step=32, dt=1, rows=4, cols=8, conv=2, ps=pose, p=None, st=None):
        return hip_lib.rgbd360_map_observe_sphere(H, vp(d), step, dt, rows, cols, conv, vp(ps), 0, p, None if st is None else C.byref(st))

    bad = [lambda st: rays(n=-1, st=st), lambda st: rays(n=1 << 31, st=st), lambda st: rays(oo=None, st=st), lambda st: rays(ww=None, st=st),
           lambda st: rays(p=params(min_count=0), st=st), lambda st: rays(p=params(near=-1.0), st=st), lambda st: rays(p=params(near=np.inf), st=st),
           lambda st: rays(p=params(margin_leaves=np.nan), st=st), lambda st: rays(p=params(margin_rel=-0.1), st=st),
           lambda st: rays(p=params(max_offset=-1.0), st=st), lambda st: rays(p=params(max_offset=np.nan), st=st),
           lambda st: rays(p=params(max_steps=0), st=st), lambda st: rays(p=params(max_steps=(1 << 23) + 1), st=st), lambda st: rays(p=params(accumulate=2), st=st),
           lambda st: sphere(d=None, st=st), lambda st: sphere(ps=None, st=st), lambda st: sphere(conv=3, st=st), lambda st: sphere(dt=2, st=st),
           lambda st: sphere(rows=-1, st=st), lambda st: sphere(step=31, st=st)]
    for k, call in enumerate(bad):
        st = fresh()
        assert call(st) == -1 and hip_lib.rgbd360_map_last_error(H) != b"", k
        assert bytes(st) == bytes([SENTINEL]) * C.sizeof(st), k
    for call in (lambda st: rays(n=0, oo=None, ww=None, st=st), lambda st: sphere(rows=0, st=st), lambda st: sphere(rows=5, cols=0, step=0, st=st)):
        st = fresh()
        assert call(st) == 0 and bytes(st) == bytes(C.sizeof(st))
    cs = fresh(_lib.MapCarveStats)
    for args in ((0, 0, 0), (1, -1, 0), (1, 0, -1)):
        assert hip_lib.rgbd360_map_carve(H, *args, C.byref(cs)) == -1
        assert (cs.n_voted, cs.n_voxels_carved, cs.n_points_carved, cs.n_voxels) == (0, 0, 0, len(ref))
    assert hip_lib.rgbd360_map_votes(H, -1, None, None, None, None) == -1
    # the votes are what they were, and so is the map
    assert all(a.tobytes() == b.tobytes() for a, b in zip(votes0, m.votes())) and len(m) == len(ref)
    V.assert_observation_equals(stats0, votes0, ref, V.observe_rays(ref, LEAF, o, w), "before the refusals")
    # a level of the pyramid observes nothing and carves nothing
    level = m.level(1)
    st, cs = fresh(), fresh(_lib.MapCarveStats)
    assert hip_lib.rgbd360_map_observe_rays(level._handle(), 10, vp(o), vp(w), 0, None, C.byref(st)) == -1 and bytes(st) == bytes([SENTINEL]) * C.sizeof(st)
    assert hip_lib.rgbd360_map_observe_sphere(level._handle(), vp(depth), 32, 1, 4, 8, 2, vp(pose), 0, None, C.byref(st)) == -1
    assert hip_lib.rgbd360_map_carve(level._handle(), 1, 0, 0, C.byref(cs)) == -1 and hip_lib.rgbd360_map_votes(level._handle(), 0, None, None, None, None) == -1
    m.release_levels()
    # an empty map: zero statistics, no votes, nothing to carve
    with new_map(reg, 1 << 10) as e:
        st = fresh()
        assert hip_lib.rgbd360_map_observe_rays(e._handle(), 10, vp(o), vp(w), 0, None, C.byref(st)) == 0 and bytes(st) == bytes(C.sizeof(st))
        st = fresh()
        assert hip_lib.rgbd360_map_observe_sphere(e._handle(), vp(depth), 32, 1, 4, 8, 2, vp(pose), 0, None, C.byref(st)) == 0 and bytes(st) == bytes(C.sizeof(st))
        assert e.vote_bytes() == 0 and hip_lib.rgbd360_map_votes(e._handle(), 0, None, None, None, None) == -1
        assert hip_lib.rgbd360_map_carve(e._handle(), 1, 0, 0, None) == -1


ADAPTER_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "rgbd360/GlobalMap.hpp"
static std::vector<float> read(FILE* f) {
    long long n = 0;
    if (fread(&n, sizeof n, 1, f) != 1) return {};
    std::vector<float> v((size_t)n);
    if (n && fread(v.data(), sizeof(float), (size_t)n, f) != (size_t)n) return {};
    return v;
}
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    const std::vector<float> pts = read(f), origins = read(f), endpoints = read(f);
    fclose(f);
    rgbd360::RegisterPhotoICP align;
    rgbd360::GlobalMap map(align, rgbd360::FilterPointCloud(0.05f), 1 << 14);
    if (!map.insert(pts.data(), nullptr, (long long)(pts.size() / 3), rgbd360::Mat4f::Identity())) return 4;
    rgbd360_map_observe_params p = map.observeParams();
    const size_t half = origins.size() / 6 * 3;
    map.observe(std::vector<float>(origins.begin(), origins.begin() + half), std::vector<float>(endpoints.begin(), endpoints.begin() + half), &p);
    p.accumulate = 1;
    map.observe(std::vector<float>(origins.begin() + half, origins.end()), std::vector<float>(endpoints.begin() + half, endpoints.end()), &p);
    const rgbd360_map_observe_stats& s = map.observeStats();
    printf("stats %lld %lld %lld %lld %lld\n", s.n_rays, s.n_valid, s.n_through, s.n_end, s.n_voxels_voted);
    std::vector<int32_t> key3, through, end, count;
    const long long n = map.votes(key3, through, end, &count);
    for (long long k = 0; k < n; ++k) printf("vote %d %d %d %d %d %d\n", key3[3 * k], key3[3 * k + 1], key3[3 * k + 2], through[k], end[k], count[k]);
    const long long carved = map.carve(1, 0, 0);
    const rgbd360_map_carve_stats& c = map.carveStats();
    printf("carve %lld %lld %lld %lld %lld %zu\n", carved, c.n_voted, c.n_points_carved, c.n_protected_end, map.size(), map.voteBytes());
    try {
        map.carve();
    } catch (const std::exception&) {
        printf("spent\n");
    }
    return 0;
}
"""


def test_cpp_adapter_gives_the_python_wrappers_votes(tmp_path, reg):
    from rgbd360_amd import build
    lib = build.build()
    pts, _ = blob()
    pts = pts[(pts[:, 0] >= -2.0) & (pts[:, 0] <= 1.0)]          # (the adapter's map has FilterPointCloud's default box)
    o, w = segments(300, pts, seed=3)
    data = tmp_path / "scene.bin"
    with open(data, "wb") as f:
        for a in (pts, o, w):
            f.write(np.int64(a.size).tobytes())
            f.write(np.ascontiguousarray(a, F).tobytes())
    src = tmp_path / "carve_adapter.cpp"
    src.write_text(ADAPTER_PROGRAM)
    exe = str(tmp_path / "carve_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.dirname(lib),
                           "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = subprocess.check_output([exe, str(data)], text=True).strip().splitlines()
    from rgbd360_amd.voxel_map import VoxelMap
    with VoxelMap(reg, LEAF, 1 << 14) as m:          # the default box, as the adapter's
        m.insert_cloud(pts, None, EYE)
        m.observe_rays(o[:150], w[:150])
        st = m.observe_rays(o[150:], w[150:], accumulate=True)
        key3, through, end, count = m.votes()
        cs = m.carve()
        size, vote_bytes = len(m), m.vote_bytes()
    assert out[0].split() == ["stats"] + [str(st[k]) for k in ("n_rays", "n_valid", "n_through", "n_end", "n_voxels_voted")]
    votes = np.array([l.split()[1:] for l in out if l.startswith("vote ")], np.int32)
    assert len(votes) == len(key3) > 100 and np.array_equal(votes, np.column_stack([key3, through, end, count]))
    assert out[-2].split() == ["carve"] + [str(v) for v in (cs["n_voxels_carved"], cs["n_voted"], cs["n_points_carved"], cs["n_protected_end"], size, vote_bytes)]
    assert out[-1] == "spent" and cs["n_voxels_carved"] > 50


def test_odometry_replay_carves_what_each_frame_sees_through(tmp_path):
    """examples/odometry_replay.cpp --carve: the pose lines of the plain replay, one "carve" line per inserted frame whose counts add up,
    and a map file of the voxels the last line reports as live."""
    import sys
    from tests.test_cpp_adapter import build_example
    exe = build_example(tmp_path)
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "3", "256", "128"])
    assert subprocess.call([exe, str(seq), "3", "256", "128", "--carve"], stderr=subprocess.DEVNULL) == 2
    assert subprocess.call([exe, str(seq), "3", "256", "128", "--map", str(tmp_path / "w.txt"), "--map-window", "2", "--carve"], stderr=subprocess.DEVNULL) == 2
    plain = subprocess.run([exe, str(seq), "3", "256", "128", "--map", str(tmp_path / "plain.txt")], text=True, capture_output=True, check=True)
    out = tmp_path / "map.txt"
    carved = subprocess.run([exe, str(seq), "3", "256", "128", "--map", str(out), "--carve"], text=True, capture_output=True, check=True)
    lines = carved.stdout.splitlines()
    assert [l for l in lines if not l.startswith("carve ")] == plain.stdout.splitlines()
    rows = [dict(zip(l.split()[2::2], map(int, l.split()[3::2]))) for l in lines if l.startswith("carve ")]
    print(rows)
    assert len(rows) == 3 and [int(l.split()[1]) for l in lines if l.startswith("carve ")] == [0, 1, 2]
    n_plain = len(np.loadtxt(str(tmp_path / "plain.txt")).reshape(-1, 7))
    for r in rows:
        assert 0 < r["rays"] <= 256 * 128 and r["end"] > r["rays"] // 4 and r["carved"] + r["protected"] <= r["voted"]
    assert rows[0]["carved"] == 0          # every voxel of the first map holds a measurement of the frame that observes it: end >= 1
    assert len(np.loadtxt(str(out)).reshape(-1, 7)) == rows[-1]["live"] and n_plain - sum(r["carved"] for r in rows) <= rows[-1]["live"] <= n_plain
