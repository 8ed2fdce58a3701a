"""The voxel table's probe bound on the device (find_or_claim, csrc/voxel_map.h; find, csrc/map_table.h) against the plain model
(tests/voxel_table_reference.py): a key's probes are the slots home .. home + 2047 (mod the table; the whole table when it is smaller) for
every writer and every reader.  The inputs are crafted: cells whose home slots fall in one window of eight, so that 2048 of them fill one
run of 2048 slots that wraps round the table's end, whatever order the device's threads arrive in; the keys inserted behind them, one per
call, are accepted or dropped by the set of occupied slots alone.  The verdicts and counters come from the model and from
voxel_map_reference; the readers' bits from the same content in a table too large to crowd (map Y) and from the restatements.

Shapes: 4096-slot tables with 2048 + 15 keys of three points each, 79 query points, panoramas of 32 x 64; 8192 slots for the refusals."""
import ctypes as C

import numpy as np
import pytest

import map_align_reference as A
import map_pyramid_reference as Y
import map_raycast_reference as M
import voxel_map_reference as R
import voxel_table_reference as T
from test_map_align_gpu import check_eval, device_eval

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)
LEAF = 0.05
N, W = 4096, 3096
LAST = T.MAX_PROBES - 1
OFFSETS = ((0.0, 0.0, 0.0), (0.1, -0.05, 0.05), (-0.1, 0.1, -0.05))      # of a cell's points from its centre, in leaves
PER_CELL = len(OFFSETS)
MAX_DIST = 0.25 * LEAF      # of the align evaluation: a cell's centroid lies within 0.18 leaves of its centre, a neighbour's beyond 0.9


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


@pytest.fixture(scope="module")
def scenario():
    return T.Scenario(N, W, 8)


def new_map(reg, capacity, leaf=LEAF):
    from rgbd360_amd.voxel_map import VoxelMap
    m = VoxelMap(reg, leaf, capacity)
    m.set_box(None, None)
    return m


def cloud_of(cells, leaf=LEAF):
    """(xyz, rgb, EYE) of PER_CELL points in each of `cells`, offset-major (a tile of the insert kernel holds 1024 distinct cells: more
    than its 512 LDS entries, so both the merged and the direct path run); the cells come back from the library's own definition."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    xyz = T.cell_points(cells, leaf, OFFSETS)
    k = np.tile(T.cell_keys(cells), PER_CELL) + np.repeat(np.arange(PER_CELL), len(cells))
    rgb = np.stack([k % 251, (k // 7) % 253, (k // 3) % 256], axis=1).astype(np.uint8)
    ref = R.Map([(xyz, rgb, EYE)], leaf, None)
    assert sorted(T.cell_keys(ref.key).tolist()) == sorted(T.cell_keys(cells).tolist()) and (ref.count == PER_CELL).all()
    assert np.array_equal(R.voxel_index(xyz, leaf), np.tile(cells, (PER_CELL, 1)))
    return xyz, rgb, EYE


def same_bytes(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def check_books(m, model, ref):
    """The map's size, census and read-out against the model's table and the restated map of the accepted clouds."""
    assert m.census() == model.census() and len(m) == len(ref) == model.census()["n_live"] and m.bytes == model.n_slots * 64
    R.assert_map_equals(m.extract(), ref)


def insert_checked(m, model, cells, accepted, repeat=False):
    """One insert call of `cells` (one key each, PER_CELL points) on the device and on the model: the statistics and the status are the
    model's.  accepted: the clouds the model took so far, extended here."""
    cloud = cloud_of(cells)
    before = model.census()["n_live"]
    verdicts = [model.insert(k, PER_CELL) for k in T.cell_keys(cells).tolist()]
    taken = [c for c, v in zip(np.asarray(cells).reshape(-1, 3), verdicts) if v is not None]
    n_dropped = PER_CELL * (len(verdicts) - len(taken))
    st = m.insert_cloud(*cloud)
    want = dict(n_valid=len(cloud[0]), n_box_rejected=0, n_out_of_range=0, n_added=PER_CELL * len(taken), n_dropped_full=n_dropped,
                n_voxels=model.census()["n_live"])
    assert {k: st[k] for k in R.STAT_NAMES} == want, (st, want, verdicts)
    assert m.full == (n_dropped > 0) and m.last_status == (3 if n_dropped else 0)
    assert repeat or model.census()["n_live"] - before == len(taken)
    if taken:
        accepted.append(cloud_of(np.array(taken)))
    return verdicts


def build_x(reg, scenario, capacity=N, chain=True, check=False):
    """Map X: stage 1 in one call, then (chain) the chain's keys one call each.  Returns (map, model, accepted clouds, chain verdicts)."""
    m, model, accepted = new_map(reg, capacity), T.Table(capacity), []
    v = insert_checked(m, model, scenario.stage1, accepted)
    assert None not in v and len(m) == T.MAX_PROBES and not m.full
    if check:
        assert capacity != N or model.occupied() == {(W + i) % N for i in range(T.MAX_PROBES)}
        check_books(m, model, R.Map(accepted, LEAF, None))
    verdicts = []
    for cell in (scenario.chain if chain else ()):
        verdicts += insert_checked(m, model, cell[None, :], accepted)
        if check:
            check_books(m, model, R.Map(accepted, LEAF, None))
    return m, model, accepted, verdicts


def build_y(reg, accepted):
    y = new_map(reg, 1 << 16)
    for cloud in accepted:
        y.insert_cloud(*cloud)
        assert not y.full
    return y


# ---- a: the last probe is a slot, the one after is not ---------------------------------------------------------------------------------
def test_the_last_probe_is_a_slot_and_the_one_after_is_not(reg, scenario):
    m, model, accepted, verdicts = build_x(reg, scenario, check=True)
    with m:
        # home W: first free slot at offset 2048, dropped; home W + d: at offset 2047, accepted; a second of that home: dropped
        assert verdicts == [None] + [LAST, None] * 7
        assert len(m) == T.MAX_PROBES + 7
        # a dropped key's points again: dropped again, nothing changes; an accepted key's points again: added to it
        before = m.extract()
        for i in (0, 2, 14):
            assert insert_checked(m, model, scenario.chain[i][None, :], accepted, repeat=True) == [None]
            assert same_bytes(before, m.extract())
        assert insert_checked(m, model, scenario.chain[1][None, :], accepted, repeat=True) == [LAST]
        check_books(m, model, R.Map(accepted, LEAF, None))
        assert len(m) == T.MAX_PROBES + 7 and m.extract()[2].max() == 2 * PER_CELL


# ---- b: the readers agree with the writer ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def xy(reg, scenario):
    """X: the crowded map of (a) after its chain; Y: the accepted points in 2^16 slots; the queries with their kinds."""
    x, model, accepted, verdicts = build_x(reg, scenario)
    y = build_y(reg, accepted)
    took = np.array([v is not None for v in verdicts])
    cells = np.concatenate([scenario.chain[took], scenario.chain[~took], scenario.absent])
    kind = np.array(["accepted"] * int(took.sum()) + ["dropped"] * int((~took).sum()) + ["absent"] * len(scenario.absent))
    world = dict(x=x, y=y, model=model, accepted=accepted, ref=R.Map(accepted, LEAF, None), cells=cells, kind=kind, points=T.cell_points(cells, LEAF))
    yield world
    x.close()
    y.close()


def rays_through(cells, leaf=LEAF, radius=64):
    """Rays along +x through the centres of `cells`, from two cells outside the block [-radius, radius)^3."""
    origins = T.cell_points(cells, leaf).copy()
    origins[:, 0] = np.float32(-(radius + 2) * leaf)
    return origins, np.tile(np.array([1.0, 0.0, 0.0], np.float32), (len(cells), 1))


def by_key(records, key_at):
    """A read-out in no specified order, ordered by (i_z, i_y, i_x): the arrays (the trailing statistics dict stays as it is)."""
    key3 = records[key_at]
    order = np.lexsort((key3[:, 0], key3[:, 1], key3[:, 2]))
    return [a[order] if isinstance(a, np.ndarray) else a for a in records]


def test_the_readers_agree_with_the_writer(reg, hip_lib, hip, xy):
    x, y, ref = xy["x"], xy["y"], xy["ref"]
    assert x.bytes == N * 64 and y.bytes == (1 << 16) * 64 and len(x) == len(y) == len(ref) == T.MAX_PROBES + 7
    R.assert_map_equals(x.extract(), ref)
    assert same_bytes(x.extract(), y.extract()) and x.records().tobytes() == y.records().tobytes()
    rec = x.records()
    assert np.array_equal(rec[:, 0].astype(np.int64), np.sort(T.cell_keys(ref.key))) and np.array_equal(rec[:, 1].astype(np.int64), ref.count)
    # the align evaluation: the queries as a cloud at the identity
    want = A.Evaluation(ref, xy["points"], EYE, LEAF, None, MAX_DIST)
    got = {name: device_eval(hip_lib, hip, m, EYE, xyz=xy["points"], max_dist=MAX_DIST) for name, m in (("x", x), ("y", y))}
    for name in got:
        check_eval(got[name], want, name)
    (kx, dx, sx, cx), (ky, dy, sy, cy) = got["x"], got["y"]
    assert kx.tobytes() == ky.tobytes() and dx.tobytes() == dy.tobytes() and sx.tobytes() == sy.tobytes() and cx == cy
    took = xy["kind"] == "accepted"
    assert took.sum() == 7 and np.array_equal(kx[took], xy["cells"][took]) and (kx[~took] == A.NO_KEY).all()
    assert want.n == 7
    # rays through the queried cells: the layered traversal, and the plain one, which looks every cell of a ray up -- the absent ones too,
    # whose search ends by the bound in X and at an empty slot in Y
    origins, dirs = rays_through(xy["cells"])
    for plain in (False, True):
        casts = []
        for m in (x, y):
            m.raycast_set_plain(plain)
            casts.append(m.raycast(origins, dirs))
            m.raycast_set_plain(False)
            M.assert_cast_equals(casts[-1], M.cast(ref, LEAF, origins, dirs, layer=not plain), "plain" if plain else "layered")
        assert same_bytes(casts[0][:5], casts[1][:5]) and casts[0][5] == casts[1][5]
        hit = casts[0][4] == 1
        assert hit[took].all() and 7 <= hit.sum() < len(hit)
    panoramas = [m.render_sphere(32, 64, EYE) for m in (x, y)]
    assert same_bytes(panoramas[0][:4], panoramas[1][:4]) and panoramas[0][4] == panoramas[1][4] and panoramas[0][4]["n_voxels"] == len(ref)
    assert panoramas[0][4]["n_pixels_covered"] > 100
    for read, key_at in ((lambda m: m.normals(), 5), (lambda m: m.colours(), 5), (lambda m: m.plane_labels(), 0)):
        a, b = by_key(read(x), key_at), by_key(read(y), key_at)
        assert np.array_equal(a[key_at], ref.key)
        assert all(u.tobytes() == v.tobytes() if isinstance(u, np.ndarray) else u == v for u, v in zip(a, b))


def test_edits_inside_the_run(reg, scenario):
    from rgbd360_amd.voxel_map import MAP_MISMATCH
    x, model, accepted, verdicts = build_x(reg, scenario)
    y = build_y(reg, accepted)
    with x, y:
        last_accepted, last_dropped = scenario.chain[13], scenario.chain[14]      # home W + 7: the accepted key stands at that home's last probe
        assert verdicts[13] == LAST and verdicts[14] is None
        gone = cloud_of(last_accepted[None, :])
        # an accepted last-probe key leaves: found by the read-only loop at offset 2047
        st = x.remove_cloud(*gone)
        assert not x.mismatch and (st["n_removed"], st["n_missing"], st["n_underflow"], st["n_voxels_emptied"]) == (PER_CELL, 0, 0, 1)
        assert model.remove(int(T.cell_keys(last_accepted)[0])) and x.census() == model.census() and model.census()["n_tombstones"] == 1
        y.remove_cloud(*gone)
        assert same_bytes(x.extract(), y.extract()) and len(x) == T.MAX_PROBES + 6
        # a dropped key is asked to leave: missing, and nothing else changes
        st = x.remove_cloud(*cloud_of(last_dropped[None, :]))
        assert x.mismatch and x.last_status == MAP_MISMATCH
        assert (st["n_removed"], st["n_missing"], st["n_underflow"], st["n_voxels_emptied"]) == (0, PER_CELL, 0, 0)
        assert same_bytes(x.extract(), y.extract()) and x.census() == model.census()
        # while the tombstone stands no other key takes its slot: the dropped key of that home meets it at its last probe and stays dropped
        assert model.first_free_offset(T.home(int(T.cell_keys(last_dropped)[0]), N)) == T.MAX_PROBES
        trash = []
        assert insert_checked(x, model, last_dropped[None, :], trash) == [None] and not trash
        assert same_bytes(x.extract(), y.extract()) and x.census() == model.census()
        # its own key revives it: one voxel more, no second slot
        n = len(x)
        assert insert_checked(x, model, last_accepted[None, :], trash) == [LAST] and len(x) == n + 1 == T.MAX_PROBES + 7
        y.insert_cloud(*gone)
        assert same_bytes(x.extract(), y.extract()) and x.census() == model.census() and model.census()["n_tombstones"] == 0
        R.assert_map_equals(x.extract(), R.Map(accepted, LEAF, None))
        # a move of an accepted key onto itself is the identity
        removed, inserted = x.move_cloud(gone[0], gone[1], EYE, EYE)
        assert not x.mismatch and not x.full and (removed["n_removed"], removed["n_missing"], removed["n_voxels_emptied"]) == (PER_CELL, 0, 1)
        assert (inserted["n_added"], inserted["n_dropped_full"], inserted["n_voxels"]) == (PER_CELL, 0, T.MAX_PROBES + 7)
        assert same_bytes(x.extract(), y.extract()) and x.census() == model.census()


# ---- c: rehash ------------------------------------------------------------------------------------------------------------------------
def test_rehash_out_of_and_into_the_crowded_table(reg, scenario):
    from rgbd360_amd.voxel_map import MAP_FULL
    x, model, accepted, _ = build_x(reg, scenario)
    ref = R.Map(accepted, LEAF, None)
    with x:
        want = x.extract()
        R.assert_map_equals(want, ref)
        # into the same number of slots: the threads' order decides whether every key finds a slot within the bound (the run's 2055 keys
        # need the order to leave no key more than 2047 slots from its home); either way the content is what it was
        rc = x.rehash(0)
        assert rc in (0, MAP_FULL) and x.bytes == N * 64 and len(x) == len(ref) and same_bytes(want, x.extract())
        assert x.census() == model.census()
        print("same-capacity rehash of the crowded table:", "done" if rc == 0 else "refused")
        for capacity in (8192, 1 << 16):
            assert x.rehash(capacity) == 0 and x.bytes == capacity * 64 and len(x) == len(ref)
            assert same_bytes(want, x.extract()) and x.census() == dict(model.census(), n_slots=capacity)


def test_rehash_refuses_what_cannot_fit(reg):
    """2060 cells whose home in a 4096-slot table lies in one window of eight: from the window's end at most 7 + 2048 slots are within
    reach of any of them, so no order places them all."""
    from rgbd360_amd.voxel_map import MAP_FULL
    cells = T.window_cells(N, W, 8)[-2060:]
    keys = T.cell_keys(cells).tolist()
    assert {T.home(k, N) for k in keys} <= set(range(W, W + 8)) and len(set(keys)) == 2060 > 7 + T.MAX_PROBES
    small = T.Table(N)
    assert sum(small.insert(k) is None for k in keys) >= 2060 - (7 + T.MAX_PROBES)        # (the model's order; any order drops at least that many)
    model, accepted = T.Table(8192), []
    with new_map(reg, 8192) as m:
        assert None not in insert_checked(m, model, cells, accepted)       # two runs of about 1030 slots in 8192: nothing is dropped
        ref = R.Map(accepted, LEAF, None)
        before, census = m.extract(), m.census()
        assert m.rehash(N) == MAP_FULL
        assert m.bytes == 8192 * 64 and len(m) == 2060 and same_bytes(before, m.extract()) and m.census() == census == model.census()
        R.assert_map_equals(m.extract(), ref)
        extra = T.window_cells(N, W, 8)[:1]
        assert insert_checked(m, model, extra, accepted) != [None] and len(m) == 2061
        check_books(m, model, R.Map(accepted, LEAF, None))


# ---- d: merge and records into a crowded destination ----------------------------------------------------------------------------------
def test_merge_and_records_into_the_crowded_table(reg, scenario):
    from rgbd360_amd.voxel_map import MAP_FULL
    x, model, accepted, _ = build_x(reg, scenario, chain=False)
    dropped, taken, existing = scenario.chain[0], scenario.chain[1], scenario.stage1[5]
    with x, new_map(reg, 64) as src_taken, new_map(reg, 64) as src_mixed:
        src_taken.insert_cloud(*cloud_of(taken[None, :]))
        src_mixed.insert_cloud(*cloud_of(np.stack([existing, dropped])))
        assert len(src_taken) == 1 and len(src_mixed) == 2
        stage1 = x.records()
        # a source voxel of home W + 1 finds the last probe free
        st = x.merge(src_taken)
        assert not x.full and (st["n_voxels_added"], st["n_voxels_new"], st["n_voxels_dropped"], st["n_voxels"]) == (1, 1, 0, T.MAX_PROBES + 1)
        assert model.insert(int(T.cell_keys(taken)[0]), PER_CELL) == LAST and x.census() == model.census()
        R.assert_map_equals(x.extract(), R.Map(accepted + [cloud_of(taken[None, :])], LEAF, None))
        # ... and leaves again: the bytes of stage 1, with a tombstone behind the run
        st = x.unmerge(src_taken)
        assert not x.mismatch and (st["n_voxels_new"], st["n_missing"], st["n_underflow"], st["n_voxels"]) == (1, 0, 0, T.MAX_PROBES)
        assert model.remove(int(T.cell_keys(taken)[0])) and x.census() == model.census() and x.records().tobytes() == stage1.tobytes()
        # a source voxel of home W finds none and is reported; the voxel that is already there still receives its terms
        st = x.merge(src_mixed)
        assert x.full and x.last_status == MAP_FULL
        assert (st["n_voxels_read"], st["n_voxels_added"], st["n_points_added"], st["n_voxels_new"], st["n_voxels_dropped"], st["n_points_dropped"],
                st["n_voxels"]) == (2, 1, PER_CELL, 0, 1, PER_CELL, T.MAX_PROBES)
        assert model.insert(int(T.cell_keys(existing)[0]), PER_CELL) is not None and model.insert(int(T.cell_keys(dropped)[0]), PER_CELL) is None
        accepted.append(cloud_of(existing[None, :]))
        R.assert_map_equals(x.extract(), R.Map(accepted, LEAF, None))
        assert x.census() == model.census()
        # the same through record lists: the accepted one revives its tombstone, the other is dropped
        st = x.add_records(src_taken.records())
        assert not x.full and (st["n_voxels_added"], st["n_voxels_new"], st["n_voxels_dropped"], st["n_voxels"]) == (1, 1, 0, T.MAX_PROBES + 1)
        assert model.insert(int(T.cell_keys(taken)[0]), PER_CELL) == LAST
        st = x.add_records(src_mixed.records())
        assert x.full and (st["n_voxels_added"], st["n_voxels_new"], st["n_voxels_dropped"], st["n_points_dropped"]) == (1, 0, 1, PER_CELL)
        model.insert(int(T.cell_keys(existing)[0]), PER_CELL)
        accepted += [cloud_of(taken[None, :]), cloud_of(existing[None, :])]
        R.assert_map_equals(x.extract(), R.Map(accepted, LEAF, None))
        assert x.census() == model.census() and model.census()["n_tombstones"] == 0


# ---- e: the sizes where the regime changes ----------------------------------------------------------------------------------------------
def block_cells(n, seed, radius=8):
    """n distinct cells of [-radius, radius)^3 in a seeded order."""
    r = np.arange(-radius, radius)
    cells = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=3).reshape(-1, 3)
    return cells[np.random.default_rng(seed).permutation(len(cells))[:n]].astype(np.int64)


def test_a_table_of_exactly_the_bound(reg, hip_lib, hip):
    """2048 slots: the bound is the whole table.  Any 2048 distinct cells fit, the 2049th is dropped, and a lookup of an absent key in a
    table without an empty slot ends by the bound."""
    cells = block_cells(2048 + 1 + 256, seed=3)
    inside, extra, absent = cells[:2048], cells[2048:2049], cells[2049:]
    model, accepted = T.Table(2048), []
    with new_map(reg, 2048) as m:
        assert None not in insert_checked(m, model, inside, accepted) and len(m) == 2048 and len(model.occupied()) == 2048
        assert insert_checked(m, model, extra, accepted) == [None]
        ref = R.Map(accepted, LEAF, None)
        check_books(m, model, ref)
        points = T.cell_points(absent, LEAF)
        got = device_eval(hip_lib, hip, m, EYE, xyz=points, max_dist=MAX_DIST)
        check_eval(got, A.Evaluation(ref, points, EYE, LEAF, None, MAX_DIST))
        assert (got[0] == A.NO_KEY).all() and got[2][0] == 0
        origins, dirs = rays_through(absent, radius=8)
        for plain in (False, True):
            m.raycast_set_plain(plain)
            cast = m.raycast(origins, dirs)
            M.assert_cast_equals(cast, M.cast(ref, LEAF, origins, dirs, layer=not plain))
            hit = cast[4] == 1
            assert not np.any((cast[1][hit][:, None, :] == absent[None, :, :]).all(axis=2))       # no ray ends in an absent cell
        m.raycast_set_plain(False)
        assert m.rehash(0) == 0 and m.census() == model.census()
        R.assert_map_equals(m.extract(), ref)


@pytest.mark.parametrize("capacity", [1, 2])
def test_tables_of_one_and_two_slots(reg, hip_lib, hip, capacity):
    cells = block_cells(capacity + 1, seed=capacity)
    model, accepted = T.Table(capacity), []
    with new_map(reg, capacity) as m:
        for k, cell in enumerate(cells):
            assert (insert_checked(m, model, cell[None, :], accepted) == [None]) == (k == capacity)
        ref = R.Map(accepted, LEAF, None)
        check_books(m, model, ref)
        points = T.cell_points(cells, LEAF)
        got = device_eval(hip_lib, hip, m, EYE, xyz=points, max_dist=MAX_DIST)
        check_eval(got, A.Evaluation(ref, points, EYE, LEAF, None, MAX_DIST))
        assert np.array_equal(got[0][:capacity], cells[:capacity]) and (got[0][capacity] == A.NO_KEY).all()
        origins, dirs = rays_through(cells, radius=8)
        M.assert_cast_equals(m.raycast(origins, dirs), M.cast(ref, LEAF, origins, dirs))
        assert m.rehash(0) == 0 and m.bytes == capacity * 64
        check_books(m, model, ref)
        assert insert_checked(m, model, cells[capacity][None, :], accepted) == [None]      # still full


# ---- f: a pyramid level that cannot hold its content -----------------------------------------------------------------------------------
def test_a_level_that_cannot_hold_its_content(reg, hip_lib):
    """2094 fine cells 2 c whose coarse cells c all have their home in one window of eight of the level's table (8192 slots for 2049 ..
    4096 voxels below it): at most 7 + 2048 of them are within reach of a slot, so the build drops voxels in any order."""
    from rgbd360_amd.register import Rgbd360Error
    from rgbd360_amd.voxel_map import MAP_FULL
    coarse = T.window_cells(8192, 7192, 8)
    assert len(coarse) == 2094 > 7 + T.MAX_PROBES and 4096 < 2 * len(coarse) <= 8192
    fine = 2 * coarse
    model, accepted = T.Table(1 << 14), []
    with new_map(reg, 1 << 14) as m:
        assert None not in insert_checked(m, model, fine, accepted)
        ref = R.Map(accepted, LEAF, None)
        before = m.extract()
        handle = C.c_void_p()
        assert hip_lib.rgbd360_map_level(m._handle(), 1, C.byref(handle)) == MAP_FULL and not handle.value
        assert b"probe bound" in hip_lib.rgbd360_map_last_error(m._handle()) and m.pyramid_bytes == 0
        with pytest.raises(Rgbd360Error, match="probe bound"):
            m.level(1)
        with pytest.raises(Rgbd360Error, match="probe bound"):      # the coarse-to-fine chain needs the level: it says so, and aligns nothing
            m.align_cloud_c2f(T.cell_points(fine[:64], LEAF), EYE, top_shift=1)
        # the parent is what it was and still usable
        assert same_bytes(before, m.extract()) and m.census() == model.census()
        R.assert_map_equals(m.extract(), ref)
        assert insert_checked(m, model, np.array([[1, 1, 1]]), accepted) != [None] and len(m) == 2095
        # an uncrowded content afterwards: the level builds
        m.clear()
        few = block_cells(100, seed=9)
        m.insert_cloud(*cloud_of(few))
        lv = m.level(1)
        want = R.Map([cloud_of(few)], Y.level_leaf(LEAF, 1), None)
        R.assert_map_equals(lv.extract(), want)
        assert len(lv) == len(want) == len({tuple(c) for c in (few >> 1).tolist()})
