"""Composing voxel maps on the device (rgbd360_map_merge / _unmerge / _records / _add_records, csrc/map_merge.h) against the numpy
restatement (tests/map_merge_reference.py), bit for bit: a sum-mode merge is the map of both clouds, a pose-mode merge is the restated
terms, un-merge leaves the map that never saw the merge, records carry a map over with its bits intact, and outside the contract the
counters are those of the definition and no word wraps.  The shapes are the smallest at which each mechanism of the kernel can fail:
tables below a wave's eight slots, a final partial block, thousands of source voxels on eight destination slots, a full table."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import map_merge_reference as M
import map_pyramid_reference as Y
import voxel_map_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
LEAF = 0.05


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def cloud():
    """5 000 points with colours: a crowded corner (voxels of many points) and a sparse rest; its two halves share voxels."""
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-1.5, 1.0, (5000, 3)).astype(np.float32)
    xyz[:1250] = (xyz[:1250] * np.float32(0.1)).astype(np.float32)
    rgb = rng.integers(0, 256, (5000, 3)).astype(np.uint8)
    order = rng.permutation(5000)
    return xyz[order], rgb[order]


def new_map(reg, leaf=LEAF, capacity=1 << 14, box="default"):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, leaf, capacity)
    if box is None:
        m.set_box(None, None)
    elif box != "default":
        m.set_box(*box)
    return m


def filled(reg, clouds, leaf=LEAF, capacity=1 << 14, box="default"):
    m = new_map(reg, leaf, capacity, box)
    for xyz, rgb, pose in clouds:
        m.insert_cloud(xyz, rgb, pose)
        assert not m.full
    return m


def ref_box(box):
    return R.DEFAULT_BOX if box == "default" else box


def restated(clouds, leaf=LEAF, box="default"):
    m = M.MergeMap(leaf, ref_box(box))
    for c in clouds:
        m.insert(*c)
    return m


def check_equal(m, ref, what=""):
    """The device map against a restated one (MergeMap): records, extract, size and census."""
    out = ref.read_out()
    assert np.array_equal(m.records(), M.records_of(out)), what
    R.assert_map_equals(m.extract(), out, what)
    c, want = m.census(), ref.census()
    assert {k: c[k] for k in want} == want and len(m) == len(out), (what, c, want)


def check_stats(got, want):
    assert {k: got[k] for k in M.STAT_NAMES} == {k: want[k] for k in M.STAT_NAMES}
    M.check_stats_add_up(got)


# ---- 1 sum mode = union --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.edge_cases(), ids=lambda c: c[0])
def test_sum_mode_is_the_union_on_the_edge_cases(reg, case):
    name, xyz, rgb, pose, leaf, box = case
    halves = [(xyz[k::2], None if rgb is None else rgb[k::2], pose) for k in (0, 1)]
    with filled(reg, halves[:1], leaf, 512, box) as a, filled(reg, halves[1:], leaf, 512, box) as b:
        ra, rb = restated(halves[:1], leaf, box), restated(halves[1:], leaf, box)
        check_stats(a.merge(b), ra.merge(rb.read_out()))
        assert a.last_status == 0 and not a.full
        check_equal(a, ra, name)
        R.assert_map_equals(a.extract(), R.Map([(xyz, rgb, pose)], leaf, box), name)


def test_sum_mode_is_the_union_on_a_split_random_cloud(reg, cloud):
    xyz, rgb = cloud
    P = R.general_pose()
    halves = [(xyz[:2500], rgb[:2500], P), (xyz[2500:], rgb[2500:], P)]
    with filled(reg, halves[:1]) as a, filled(reg, halves[1:]) as b:
        ra, rb = restated(halves[:1]), restated(halves[1:])
        st = a.merge(b)
        check_stats(st, ra.merge(rb.read_out()))
        assert 0 < st["n_voxels_new"] < st["n_voxels_added"]            # voxels both maps hold, and new ones
        check_equal(a, ra)
        R.assert_map_equals(a.extract(), R.Map([(xyz, rgb, P)], LEAF))
        check_equal(b, rb)                                              # the source is only read
        # min_count: the source's thin voxels stay out and are counted
        with filled(reg, halves[:1]) as c:
            rc = restated(halves[:1])
            st = c.merge(b, min_count=3)
            check_stats(st, rc.merge(rb.read_out(), None, 3))
            assert st["n_voxels_below_min_count"] > 0
            check_equal(c, rc)


# ---- 2 pose mode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_leaf", [0.05, 0.02, 0.25])
def test_pose_mode_at_the_general_pose(reg, cloud, src_leaf):
    xyz, rgb = cloud
    P = R.general_pose()
    with filled(reg, [(xyz, rgb, EYE)], src_leaf) as src, filled(reg, [(xyz[:300] + np.float32(0.2), rgb[:300], P)], LEAF, box=None) as dst:
        rs, rd = restated([(xyz, rgb, EYE)], src_leaf), restated([(xyz[:300] + np.float32(0.2), rgb[:300], P)], LEAF, None)
        st = dst.merge(src, P)
        check_stats(st, rd.merge(rs.read_out(), P))
        assert st["n_voxels_added"] == len(src) and dst.census()["n_inconsistent"] == 0
        check_equal(dst, rd, "source leaf %g" % src_leaf)


# ---- 3 contention --------------------------------------------------------------------------------------------------------------------
def contended_source():
    """4 096 voxels of 0.01 m, the cells -8 .. 7 of every axis, one to three points each: eight voxels of 0.16 m hold them all."""
    ijk = np.stack(np.meshgrid(*[np.arange(-8, 8)] * 3, indexing="ij"), axis=3).reshape(-1, 3)
    rng = np.random.default_rng(11)
    which = np.concatenate([np.arange(4096), rng.integers(0, 4096, 4096)])
    xyz = ((ijk[which] + rng.uniform(0.3, 0.7, (len(which), 3))) * 0.01).astype(np.float32)
    return xyz, rng.integers(0, 256, xyz.shape).astype(np.uint8)


def test_thousands_of_source_voxels_on_eight_destination_slots(reg):
    xyz, rgb = contended_source()
    with filled(reg, [(xyz, rgb, EYE)], 0.01, 1 << 13, None) as src, new_map(reg, 0.16, 64, None) as dst:
        rs, rd = restated([(xyz, rgb, EYE)], 0.01, None), M.MergeMap(0.16, None)
        assert len(src) == 4096
        check_stats(dst.merge(src, EYE), rd.merge(rs.read_out(), EYE))
        assert 1 <= len(dst) <= 8 and dst.census()["n_points"] == len(xyz)
        check_equal(dst, rd)
        check_stats(dst.unmerge(src, EYE), rd.unmerge(rs.read_out(), EYE))      # ... and the compare-and-swap loop under the same contention
        assert len(dst) == 0 and not dst.mismatch
        check_equal(dst, rd)


# ---- 4 ragged and tiny tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 2, 4, 8, 16, 32])
def test_source_tables_smaller_than_a_block(reg, slots):
    """Fewer slots than a wave carries (8) and than a block carries (32); every slot of the source is occupied."""
    xyz = (np.arange(slots)[:, None] * np.float32([0.11, 0.07, -0.13]) + np.float32(0.02)).astype(np.float32)
    rgb = (np.arange(3 * slots).reshape(-1, 3) * 5 % 256).astype(np.uint8)
    P = R.general_pose()
    with filled(reg, [(xyz, rgb, EYE)], LEAF, slots, None) as src, new_map(reg, LEAF, 256, None) as a, new_map(reg, 0.1, 256, None) as b:
        rs = restated([(xyz, rgb, EYE)], LEAF, None)
        assert len(src) == slots and src.bytes == 64 * slots
        ra, rb = M.MergeMap(LEAF, None), M.MergeMap(0.1, None)
        check_stats(a.merge(src), ra.merge(rs.read_out()))
        check_stats(b.merge(src, P), rb.merge(rs.read_out(), P))
        check_equal(a, ra)
        check_equal(b, rb)


@pytest.mark.parametrize("n", [1, 7, 31, 33, 257])
def test_record_lists_of_ragged_lengths(reg, cloud, n):
    rec = M.records_of(R.Map([(cloud[0], cloud[1], EYE)], LEAF))[:n]
    with new_map(reg, LEAF, 1024) as m:
        ref = M.MergeMap(LEAF)
        check_stats(m.add_records(rec), ref.add_records(rec))
        assert np.array_equal(m.records(), rec) and len(m) == n
        check_equal(m, ref)


def test_an_empty_source_touches_nothing(reg, cloud):
    with filled(reg, [(cloud[0][:500], cloud[1][:500], EYE)]) as dst, new_map(reg) as empty:
        before = dst.records()
        dst.observe_rays(np.zeros((1, 3), np.float32), cloud[0][:1])
        for st in (dst.merge(empty), dst.merge(empty, R.general_pose()), dst.unmerge(empty), dst.add_records(np.zeros((0, 8), np.uint64))):
            assert dst.last_status == 0 and all(st[k] == 0 for k in M.STAT_NAMES if k != "n_voxels") and st["n_voxels"] == len(before)
        dst.votes()                                                     # not even the revision moved: the votes are still good
        assert np.array_equal(dst.records(), before)


# ---- 5 un-merge is exact -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tombstones", [("sum", False), ("pose", False), ("sum", True), ("pose", True)])
def test_unmerge_leaves_the_map_that_never_saw_the_merge(reg, cloud, mode, tombstones):
    xyz, rgb = cloud
    P = None if mode == "sum" else R.general_pose()
    further = (xyz[3000:] + np.float32(0.01), rgb[3000:], EYE)
    ghost = (xyz[:800], rgb[:800], R.general_pose())
    with filled(reg, [(xyz[:3000], rgb[:3000], EYE)], LEAF, box=None) as src, new_map(reg, LEAF, box=None) as dst:
        rs, rd = restated([(xyz[:3000], rgb[:3000], EYE)], LEAF, None), M.MergeMap(LEAF, None)
        if tombstones:          # the destination already holds tombstones: new voxels are counted as revivals
            dst.insert_cloud(*ghost), dst.remove_cloud(*ghost)
            rd.insert(*ghost), rd.remove(*ghost)
            assert len(dst) == 0 and dst.census()["n_tombstones"] > 0
        check_stats(dst.merge(src, P), rd.merge(rs.read_out(), P))
        assert len(dst) == len(rd) and not dst.full
        dst.insert_cloud(*further)
        rd.insert(*further)
        check_equal(dst, rd, "merged")
        check_stats(dst.unmerge(src, P), rd.unmerge(rs.read_out(), P))
        assert dst.last_status == 0 and not dst.mismatch
        only = R.Map([further], LEAF, None)
        assert np.array_equal(dst.records(), M.records_of(only)) and len(dst) == len(only)
        R.assert_map_equals(dst.extract(), only)
        c = dst.census()
        assert c["n_tombstones"] == rd.census()["n_tombstones"] > 0 and c["n_inconsistent"] == 0
        assert dst.rehash() == 0
        c = dst.census()
        assert (c["n_tombstones"], c["n_live"], c["n_inconsistent"]) == (0, len(only), 0) and np.array_equal(dst.records(), M.records_of(only))


# ---- 6 outside the contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sum", "pose"])
def test_unmerge_of_a_source_never_merged_is_a_mismatch(reg, cloud, mode):
    from rgbd360_amd.voxel_map import MAP_MISMATCH
    xyz, rgb = cloud
    P = None if mode == "sum" else EYE
    with filled(reg, [(xyz, rgb, EYE)], LEAF, box=None) as src, filled(reg, [(xyz[::2], rgb[::2], EYE)], LEAF, box=None) as dst:
        rs, rd = restated([(xyz, rgb, EYE)], LEAF, None), restated([(xyz[::2], rgb[::2], EYE)], LEAF, None)
        st = dst.unmerge(src, P)
        check_stats(st, rd.unmerge(rs.read_out(), P))
        assert dst.last_status == MAP_MISMATCH and dst.mismatch and st["n_missing"] > 0 and st["n_underflow"] > 0
        c = dst.census()
        assert c["n_points"] == rd.census()["n_points"] and c["n_live"] == len(rd) == len(dst)
        rec = dst.records()
        assert (rec[:, 1] < np.uint64(1 << 31)).all()                   # no count wrapped


# ---- 7 range -----------------------------------------------------------------------------------------------------------------------
def test_a_pose_that_carries_part_of_the_source_out_of_range(reg):
    f = np.float32
    edge = f(1.0) - f(2.0) ** -12                                       # 4095 + edge is the float below 4096
    xs = np.array([0.1, 0.5, 0.9, edge, 1.0, 1.2, 1.7], f)
    xyz = np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], axis=1)
    xyz = np.concatenate([xyz, xyz[4:]])                                # the voxels that leave hold two points each
    T = EYE.copy()
    T[0, 3] = 4095.0
    with filled(reg, [(xyz, None, EYE)], LEAF, 64, None) as src, new_map(reg, LEAF, 64, None) as dst:
        rs, rd = restated([(xyz, None, EYE)], LEAF, None), M.MergeMap(LEAF, None)
        st = dst.merge(src, T)
        check_stats(st, rd.merge(rs.read_out(), T))
        assert (st["n_voxels_out_of_range"], st["n_points_out_of_range"], st["n_voxels_added"], st["n_points_added"]) == (3, 6, 4, 4)
        check_equal(dst, rd)
        assert dst.extract()[0][:, 0].max() == np.nextafter(f(4096.0), f(0.0))      # the float below 4096 is kept
        check_stats(dst.unmerge(src, T), rd.unmerge(rs.read_out(), T))
        assert len(dst) == 0 and not dst.mismatch


# ---- 8 full table --------------------------------------------------------------------------------------------------------------------
def test_a_full_destination_drops_new_voxels_and_keeps_adding_to_old_ones(reg):
    from rgbd360_amd.voxel_map import MAP_FULL
    ijk = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(2), indexing="ij"), axis=3).reshape(-1, 3)
    xyz = np.repeat(((ijk + 0.5) * LEAF).astype(np.float32), 2, axis=0)                 # 200 voxels of two points
    rgb = (np.arange(xyz.size).reshape(-1, 3) * 7 % 256).astype(np.uint8)
    with filled(reg, [(xyz, rgb, EYE)], LEAF, 512, None) as src, filled(reg, [(xyz[:40:2], rgb[:40:2], EYE)], LEAF, 64, None) as dst:
        assert len(src) == 200 and len(dst) == 20 and dst.bytes == 64 * 64
        before = {int(r[0]): r[1:].astype(np.int64) for r in dst.records()}
        term = {int(r[0]): r[1:].astype(np.int64) for r in src.records()}
        st = dst.merge(src)
        M.check_stats_add_up(st)
        assert dst.last_status == MAP_FULL and dst.full and st["n_voxels_dropped"] > 0 and st["n_points_dropped"] == 2 * st["n_voxels_dropped"]
        assert st["n_voxels_added"] + st["n_voxels_dropped"] == 200 and st["n_voxels_new"] == st["n_voxels_added"] - 20
        after = {int(r[0]): r[1:].astype(np.int64) for r in dst.records()}
        assert len(after) == len(dst) == st["n_voxels"] == 20 + st["n_voxels_new"] <= 64 and set(before) <= set(after)
        for key, row in after.items():                                  # old voxels received their terms, new ones are the source's
            assert np.array_equal(row, before.get(key, 0) + term[key]), key
        c = dst.census()
        assert (c["n_live"], c["n_inconsistent"]) == (len(after), 0)


# ---- 9 refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_untouched(reg, cloud):
    from rgbd360_amd.register import Rgbd360Error
    xyz, rgb = cloud
    with filled(reg, [(xyz[:500], rgb[:500], EYE)]) as dst, filled(reg, [(xyz[500:900], rgb[500:900], EYE)], 0.1) as coarse, \
            filled(reg, [(xyz[500:900], rgb[500:900], EYE)]) as src:
        before = dst.records()
        dst.observe_rays(np.zeros((1, 3), np.float32), xyz[:1])
        nan_pose = EYE.copy()
        nan_pose[1, 2] = np.nan
        lv = dst.level(1)
        closed = new_map(reg)
        closed.close()
        for what, call in (("itself", lambda: dst.merge(dst)), ("itself", lambda: dst.unmerge(dst, EYE)), ("read-only", lambda: lv.merge(src)),
                           ("read-only", lambda: lv.unmerge(src, EYE)), ("read-only", lambda: lv.add_records(before[:1])),
                           ("one leaf", lambda: dst.merge(coarse)), ("one leaf", lambda: dst.unmerge(coarse)),
                           ("non-finite", lambda: dst.merge(src, nan_pose)), ("non-finite", lambda: dst.unmerge(src, nan_pose)),
                           ("min_count", lambda: dst.merge(src, min_count=0)), ("closed", lambda: dst.merge(closed)),
                           ("closed", lambda: closed.merge(src)), ("VoxelMap", lambda: dst.merge(before))):
            with pytest.raises(Rgbd360Error, match=what):
                call()
        dst.votes()                                                     # nothing was launched: the votes are not stale
        assert np.array_equal(dst.records(), before) and len(lv) > 0


# ---- 10 a level as source ----------------------------------------------------------------------------------------------------------------
def test_a_level_of_a_pyramid_as_the_source(reg, cloud):
    xyz, rgb = cloud
    P = R.general_pose()
    with filled(reg, [(xyz, rgb, EYE)], 0.02, 1 << 14) as b, new_map(reg, LEAF, box=None) as a, new_map(reg, 0.04, box=None) as s:
        level = Y.Level(R.Map([(xyz, rgb, EYE)], 0.02), 1)
        ra, rsum = M.MergeMap(LEAF, None), M.MergeMap(0.04, None)
        check_stats(a.merge(b.level(1), P), ra.merge(level, P))
        check_equal(a, ra)
        check_stats(s.merge(b.level(1)), rsum.merge(level))            # sum mode: the level's leaf is 0.02 * 2 in float32
        check_equal(s, rsum)


# ---- 11 writers' duties -----------------------------------------------------------------------------------------------------------------
def test_a_merge_is_a_write_like_any_other(reg):
    from rgbd360_amd.register import Rgbd360Error
    g = (np.stack(np.meshgrid(np.arange(10), np.arange(10), indexing="ij"), axis=2).reshape(-1, 2) + 0.5) * LEAF
    wall = lambda y0: np.stack([np.full(len(g), 1.0), g[:, 0] + y0, g[:, 1] - 0.25], axis=1).astype(np.float32)      # two patches of one wall, 1 m away
    left, right = wall(-0.6), wall(0.1)

    def hits(m):
        _, _, count, key3, _ = m.raycast_sphere(64, 128, EYE)
        return {tuple(k) for k in key3[count > 0].tolist()}

    with filled(reg, [(left, None, EYE)], LEAF, 1024, None) as a, filled(reg, [(right, None, EYE)], LEAF, 1024, None) as b:
        only_b = {tuple(k) for k in b.extract()[3].tolist()}
        assert hits(a) and not hits(a) & only_b and len(a.level(1)) > 0
        a.observe_rays(np.zeros((1, 3), np.float32), left[:1])
        a.votes()
        n_level = len(a.level(1))
        st = a.merge(b)
        assert st["n_voxels_new"] == len(b) == 100 and len(a) == 200
        with pytest.raises(Rgbd360Error):
            a.votes()                                                   # taken before the merge: stale
        assert len(a.normals()[0]) == len(a) == 200
        assert hits(a) & only_b                                         # the ray cast sees a voxel only the merged source held
        want = Y.Level(R.Map([(left, None, EYE), (right, None, EYE)], LEAF, None), 1)
        assert len(a.level(1)) == len(want) > n_level
        assert np.array_equal(a.level(1).records(), M.records_of(want))
        a.unmerge(b)
        assert len(a) == 100 and len(a.level(1)) == n_level and not hits(a) & only_b and len(a.normals()[0]) == 100


# ---- 12 records ----------------------------------------------------------------------------------------------------------------------
def test_records_carry_a_map_over_with_its_bits(reg, cloud, tmp_path):
    from rgbd360_amd.register import Rgbd360Error
    from rgbd360_amd.voxel_map import VoxelMap
    xyz, rgb = cloud
    P = R.general_pose()
    box = (np.float32([-1.0, -1.5, -1.5]), np.float32([0.5, 1.0, 1.0]))
    with filled(reg, [(xyz, rgb, P)], LEAF, 1 << 14, box) as a, new_map(reg, LEAF, 1 << 15) as b:
        ref = R.Map([(xyz, rgb, P)], LEAF, box)
        rec = a.records()
        assert rec.dtype == np.uint64 and np.array_equal(rec, M.records_of(ref)) and np.array_equal(a.records(10), rec[:10])
        st = b.add_records(rec)
        M.check_stats_add_up(st)
        assert st["n_voxels_new"] == st["n_voxels_added"] == len(ref) and a.bytes != b.bytes
        assert np.array_equal(b.records(), rec)
        R.assert_map_equals(b.extract(), ref)
        # a file and back: the records, the leaf and the box
        path = str(tmp_path / "map.npz")
        a.save(path)
        with VoxelMap.load(reg, path) as c, VoxelMap.load(reg, path, capacity=1 << 13, leaf=LEAF) as d:
            for m in (c, d):
                assert np.array_equal(m.records(), rec) and m.leaf == a.leaf and m.box[0] and all(np.array_equal(u, v) for u, v in zip(m.box[1:], box))
                R.assert_map_equals(m.extract(), ref)
            c.insert_cloud(xyz[:100] * np.float32(3.0), None, EYE)      # the restored box is in force: the same insert on both
            a.insert_cloud(xyz[:100] * np.float32(3.0), None, EYE)
            assert np.array_equal(c.records(), a.records())
        with pytest.raises(Rgbd360Error, match="leaf"):
            VoxelMap.load(reg, path, leaf=0.051)
        # equal keys in one list add up
        with new_map(reg, LEAF, 1 << 14) as e:
            twice = M.MergeMap(LEAF)
            dup = np.concatenate([rec, rec[:300], rec[:7]])
            check_stats(e.add_records(dup), twice.add_records(dup))
            check_equal(e, twice)
        # each kind of bad record: refused as a whole, the map unchanged
        before = b.records()
        n = int(rec[5, 1])
        for word, value in ((0, 0xFFFFFFFFFFFFFFFF), (1, 0), (5, 256 * n), (2, n << 32)):
            bad = rec[:40].copy()
            bad[5, word] = value
            assert M.bad_records(bad).sum() == 1
            with pytest.raises(Rgbd360Error, match="1 of 40 records"):
                b.add_records(bad)
            assert np.array_equal(b.records(), before)


# ---- 13 same bits from run to run ----------------------------------------------------------------------------------------------------------
def test_two_merges_of_the_same_inputs_give_the_same_bits(reg, cloud):
    xyz, rgb = cloud
    P = R.general_pose()
    cx, cr = contended_source()
    with filled(reg, [(xyz, rgb, EYE)], 0.02) as src, filled(reg, [(cx, cr, EYE)], 0.01, 1 << 13, None) as dense:
        out = []
        for capacity in (1 << 13, 1 << 16, 1 << 14):
            with new_map(reg, LEAF, capacity, None) as dst:
                dst.merge(src, P)
                dst.merge(dense, P)
                out.append(dst.records())
        assert len(out[0]) > 1000 and np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


def test_the_timing_entry_changes_neither_map(reg, cloud):
    """rgbd360_map_time_merge (the diagnostics header) works on a scratch table: four figures, both maps as they were."""
    from rgbd360_amd.register import _ptr, pose_to_cm
    xyz, rgb = cloud
    with filled(reg, [(xyz[:2000], rgb[:2000], EYE)]) as dst, filled(reg, [(xyz[2000:], rgb[2000:], EYE)], 0.02) as src:
        before = dst.records(), src.records()
        dst.observe_rays(np.zeros((1, 3), np.float32), xyz[:1])
        g = pose_to_cm(R.general_pose())
        for pose, want in ((_ptr(g), 0), (None, -1)):                  # (sum mode between unequal leaves is refused here too)
            avg = np.zeros(4, np.float32)
            assert dst._L.rgbd360_map_time_merge(dst._handle(), src._handle(), pose, 2, _ptr(avg)) == want
            assert (avg > 0).all() if want == 0 else not avg.any()
        assert dst._L.rgbd360_map_time_merge(dst._handle(), dst._handle(), _ptr(g), 2, _ptr(avg)) == -1
        dst.votes()                                                     # the revision did not move
        assert np.array_equal(dst.records(), before[0]) and np.array_equal(src.records(), before[1])


# ---- 14 the example ----------------------------------------------------------------------------------------------------------------------
def test_submap_compose_example_matches_the_python_mirror(reg, tmp_path):
    """examples/submap_compose.cpp on 6 dumped frames, W = 3: the sizes and the CRC of records() of the composed map, before and after one
    submap is re-posed, are those of VoxelMap.merge / unmerge of the same submaps."""
    from rgbd360_amd import build, synth
    lib = build.build()
    exe = str(tmp_path / "submap_compose")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "submap_compose.cpp"),
                           "-L" + os.path.dirname(lib), "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    seq = tmp_path / "seq"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "dump_sequence.py"), str(seq), "6", "256", "128"])
    world = [synth.trajectory_pose(k, 7) for k in range(6)]
    frame_pose = [(np.linalg.inv(world[3 * (k // 3)]) @ world[k]).astype(np.float32) for k in range(6)]
    sub_pose = [world[0].astype(np.float32), world[3].astype(np.float32)]
    shift = np.eye(4)
    shift[:3, 3] = [0.03, -0.02, 0.04]
    new_pose = (shift @ world[3]).astype(np.float32)
    with open(tmp_path / "poses.txt", "w") as f:
        for T in frame_pose + sub_pose:
            f.write(" ".join("%.9g" % v for v in T.T.reshape(-1)) + "\n")
        f.write("1 " + " ".join("%.9g" % v for v in new_pose.T.reshape(-1)) + "\n")
    got = subprocess.run([exe, str(seq), "6", "256", "128", "3", str(tmp_path / "poses.txt")], text=True, capture_output=True, check=True).stdout
    crc = lambda m: "%08x" % (zlib.crc32(m.records().tobytes()) & 0xFFFFFFFF)
    want = []
    subs = [new_map(reg, LEAF, 1 << 17) for _ in range(2)]
    with subs[0], subs[1], new_map(reg, LEAF, 1 << 19) as glob:
        for s in range(2):
            for k in range(3 * s, 3 * s + 3):
                rgb, depth = synth.render(world[k], 256, 128, 7)
                subs[s].insert_sphere(rgb, depth, frame_pose[k], convention=2)
            want.append("submap %d frames %d %d voxels %d" % (s, 3 * s, 3 * s + 2, len(subs[s])))
            glob.merge(subs[s], sub_pose[s])
        want.append("composed voxels %d points %d crc %s" % (len(glob), glob.census()["n_points"], crc(glob)))
        st = glob.unmerge(subs[1], sub_pose[1])
        glob.merge(subs[1], new_pose)
        c = glob.census()
        want.append("reposed submap 1 emptied %d voxels %d points %d tombstones %d crc %s" % (st["n_voxels_new"], len(glob), c["n_points"], c["n_tombstones"], crc(glob)))
        assert st["n_voxels_new"] > 0 and c["n_inconsistent"] == 0 and not glob.mismatch
    assert got.strip().splitlines() == want, got
