"""The plain model of the voxel map's table (tests/voxel_table_reference.py) against itself and against the figures the probe-bound
tests rest on: the occupied set does not depend on the order of insertion, the crafted window has the cells it is said to have, the run
they fill wraps round the table's end, the chain of accepted and dropped keys behind it is the documented one, and the writer and the
reader of the model agree on the last probe.  No device."""
import numpy as np
import pytest

import voxel_map_reference as R
import voxel_table_reference as T

N, W = 4096, 3096


@pytest.fixture(scope="module")
def scenario():
    return T.Scenario(N, W, 8)


def test_the_hash_and_the_key_on_ints_and_arrays_agree():
    cells = np.array([[0, 0, 0], [-1, -1, -1], [63, -64, 5], [-(1 << 20), (1 << 20) - 1, 0]], np.int64)
    keys = T.cell_keys(cells)
    assert keys.tolist() == [T.pack_key(*c) for c in cells.tolist()] and keys[0] == (1 << 62) | (1 << 41) | (1 << 20)
    assert [T.unpack_key(k) for k in keys.tolist()] == [tuple(c) for c in cells.tolist()]
    assert T.mix64_np(keys.astype(np.uint64)).tolist() == [T.mix64(k) for k in keys.tolist()]
    assert T.mix64(0) == 0 and T.mix64(1) == 0xb456bcfc34c2cb2c          # MurmurHash3's fmix64 of 1
    # the packing is voxel_map_reference's: a point at a cell's centre gets that cell's key
    ref = R.Map([(T.cell_points(cells[:3], 0.05), None, np.eye(4, dtype=np.float32))], 0.05, None)
    assert sorted(T.cell_keys(ref.key).tolist()) == sorted(keys[:3].tolist())


def test_the_crafted_windows_hold_the_cells_counted():
    by_home = T.crafted_cells(N, W, 8)
    sizes = [len(by_home[W + d]) for d in range(8)]
    assert sum(sizes) == 4125 and (min(sizes), max(sizes)) == (488, 547)
    assert all(T.home(k, N) == h for h, c in by_home.items() for k in T.cell_keys(c).tolist())
    by_home = T.crafted_cells(8192, 7192, 8)
    sizes = [len(by_home[7192 + d]) for d in range(8)]
    assert sum(sizes) == 2094 and (min(sizes), max(sizes)) == (250, 286)
    assert T.crafted_cells(N, W, 8) is T.crafted_cells(N, W, 8)           # cached
    wrapped = T.crafted_cells(16, 14, 4, radius=4)                       # a window that wraps: homes 14, 15, 0, 1
    assert sorted(wrapped) == [0, 1, 14, 15] and all(T.home(k, 16) == h for h, c in wrapped.items() for k in T.cell_keys(c).tolist())
    assert sum(len(c) for c in T.crafted_cells(16, 0, 16, radius=4).values()) == 8 ** 3


def test_the_occupied_set_does_not_depend_on_the_order(scenario):
    keys = T.cell_keys(scenario.stage1).tolist()
    assert len(set(keys)) == T.MAX_PROBES
    run = {(W + i) % N for i in range(T.MAX_PROBES)}
    assert min(run) == 0 and max(run) == N - 1                            # the run wraps round the table's end
    largest = []
    for seed in (0, 1, 2):
        t = T.Table(N)
        offsets = [t.insert(keys[i]) for i in np.random.default_rng(seed).permutation(len(keys))]
        assert None not in offsets and t.occupied() == run
        # the run's last slot holds a key whose home is one of the window's eight
        assert T.MAX_PROBES - 8 <= max(offsets) <= T.MAX_PROBES - 1
        largest.append(max(offsets))
        assert all(t.find(k) is not None for k in keys)
    assert largest[0] == 2041
    # the insert kernel's per-workgroup table: these keys use 502 of its 512 entries, at most 10 keys to an entry
    entries = np.bincount([T.lds_entry(k) for k in keys], minlength=T.LDS_SLOTS)
    assert (int((entries > 0).sum()), int(entries.max())) == (502, 10)


def test_the_chain_behind_the_run(scenario):
    t, offsets = scenario.model()
    last = T.MAX_PROBES - 1
    assert offsets == [None] + [last, None] * 7
    homes = [T.home(k, N) for k in T.cell_keys(scenario.chain).tolist()]
    assert homes == [W] + [W + d for d in range(1, 8) for _ in (0, 1)]
    assert t.occupied() == {(W + i) % N for i in range(T.MAX_PROBES + 7)}
    assert t.first_free_offset(W) == T.MAX_PROBES + 7 and t.first_free_offset((W + T.MAX_PROBES + 7) % N) == 0
    assert t.census() == dict(n_slots=N, n_live=T.MAX_PROBES + 7, n_tombstones=0, n_points=T.MAX_PROBES + 7, n_inconsistent=0)
    # no absent key collides with an inserted one, and a reader's search for it ends by the bound, not at an empty slot
    inserted = set(T.cell_keys(scenario.stage1).tolist()) | set(T.cell_keys(scenario.chain).tolist())
    for k in T.cell_keys(scenario.absent).tolist():
        assert k not in inserted and t.find(k) is None and t.first_free_offset(T.home(k, N)) >= T.MAX_PROBES
    assert len(scenario.absent) == 64


def test_writer_and_reader_agree_on_the_last_probe(scenario):
    t = T.Table(N)
    for k in T.cell_keys(scenario.stage1).tolist():
        t.insert(k)
    dropped, accepted = T.cell_keys(scenario.chain[:2]).tolist()
    assert t.first_free_offset(T.home(dropped, N)) == T.MAX_PROBES and t.first_free_offset(T.home(accepted, N)) == T.MAX_PROBES - 1
    assert t.insert(accepted) == T.MAX_PROBES - 1 == t.find(accepted)     # offset 2047: a slot for both
    assert t.insert(dropped) is None and t.find(dropped) is None          # offset 2048: a slot for neither
    # a key that stands one slot past the bound (put there by a writer with a longer bound) is invisible to the bounded reader
    long = T.Table(N, max_probes=T.MAX_PROBES + 2)
    long.keys, long.count = list(t.keys), list(t.count)
    assert long.insert(dropped) == T.MAX_PROBES + 1                       # (the accepted key took offset 2048 from W)
    t.keys, t.count = list(long.keys), list(long.count)
    assert long.find(dropped) == T.MAX_PROBES + 1 and t.find(dropped) is None


def test_tombstones_keep_their_slot():
    t, keys = T.Table(4), [T.pack_key(i, 0, 0) for i in range(6)]
    taken = [k for k in keys if t.insert(k) is not None][:4]
    assert len(taken) == 4 and len(t.occupied()) == 4
    other = next(k for k in keys if k not in taken)
    assert t.insert(other) is None                                        # full: the bound is the whole table
    assert t.remove(taken[0]) and not t.remove(taken[0]) and t.find(taken[0]) is None and t.find(taken[0], tombstones=True) is not None
    assert t.insert(other) is None and len(t.occupied()) == 4             # the tombstone is not reused by another key
    assert t.census()["n_tombstones"] == 1 and t.insert(taken[0], 2) is not None and t.census() == dict(n_slots=4, n_live=4, n_tombstones=0, n_points=5, n_inconsistent=0)
    assert T.Table(1).insert(keys[0]) == 0 and T.Table(2048).n_probes == 2048 == T.Table(4096).n_probes and T.Table(1024).n_probes == 1024
