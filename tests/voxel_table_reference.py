"""A plain model of the voxel map's table (csrc/map_table.h, csrc/voxel_map.h; DESIGN.md 3.11, probe bound): the hash, the key, the
home slot and a sequential linear-probing table with the probe bound and tombstones.  Independent of the library: integer and array
operations only, no code shared with it.

The bound, as the headers document it: a key's probe sequence visits the slots home, home + 1, ... home + min(n_slots, 2048) - 1 (mod
the table) and no other.  A writer claims the first empty one of them; a key that finds none is dropped.  A reader visits the same slots
and stops at the first empty one.  A removal leaves the key in its slot (a tombstone): the slot stays occupied for every probe sequence
that passes it, no other key ever takes it, and readers take it as absent.

Two facts make expectations from this model exact for a table filled by concurrent threads:
  * the set of occupied slots of a linear-probing table does not depend on the order of insertion, as long as nothing is dropped;
  * whether a key inserted afterwards, in a call of its own, finds a slot depends only on that set."""
import functools

import numpy as np

MAX_PROBES = 2048
BIAS = 1 << 20
MASK64 = (1 << 64) - 1
EMPTY = MASK64
LDS_SLOTS = 512      # of the insert kernel's per-workgroup table; its entry of a key is bits 40 .. 48 of the hash


def mix64(k):
    """The 64-bit finaliser of MurmurHash3, on a Python int."""
    k &= MASK64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & MASK64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & MASK64
    k ^= k >> 33
    return k


def mix64_np(k):
    """The same on a numpy.uint64 array (the products wrap)."""
    k = np.asarray(k, np.uint64).copy()
    s = np.uint64(33)
    with np.errstate(over="ignore"):
        k ^= k >> s
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> s
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> s
    return k


def pack_key(ix, iy, iz):
    """The key of the cell (ix, iy, iz): the three biased 21-bit indices, i_z, i_y, i_x from the top.  Python ints or int64 arrays."""
    return ((iz + BIAS) << 42) | ((iy + BIAS) << 21) | (ix + BIAS)


def unpack_key(key):
    return (key & 0x1fffff) - BIAS, ((key >> 21) & 0x1fffff) - BIAS, (key >> 42) - BIAS


def home(key, n_slots):
    return mix64(int(key)) & (n_slots - 1)


def lds_entry(key):
    return (mix64(int(key)) >> 40) & (LDS_SLOTS - 1)


class Table:
    """A sequential linear-probing table of n_slots slots (a power of two): per slot a key and the points it holds."""

    def __init__(self, n_slots, max_probes=MAX_PROBES):
        assert n_slots >= 1 and n_slots & (n_slots - 1) == 0
        self.n_slots = n_slots
        self.n_probes = min(n_slots, max_probes)
        self.keys = [EMPTY] * n_slots
        self.count = [0] * n_slots

    def _slot(self, key, off):
        return (home(key, self.n_slots) + off) & (self.n_slots - 1)

    def _sequence(self, key):
        """(offset, slot) of every probe of `key`: the bound is here and nowhere else."""
        h, mask = home(key, self.n_slots), self.n_slots - 1
        return ((off, (h + off) & mask) for off in range(self.n_probes))

    def insert(self, key, n_points=1):
        """The offset from its home at which `key` landed or already stood (a tombstone of it is revived); None: dropped."""
        for off, s in self._sequence(key):
            if self.keys[s] == EMPTY:
                self.keys[s] = key
            if self.keys[s] == key:
                self.count[s] += n_points
                return off
        return None

    def find(self, key, tombstones=False):
        """The offset at which a reader finds `key`; None: absent -- an empty slot or the bound ended the search, or (unless `tombstones`)
        the slot found is a tombstone."""
        for off, s in self._sequence(key):
            if self.keys[s] == EMPTY:
                return None
            if self.keys[s] == key:
                return off if tombstones or self.count[s] > 0 else None
        return None

    def remove(self, key):
        """All points of `key` leave; its slot becomes a tombstone.  False: the key is not there (or is a tombstone already)."""
        off = self.find(key)
        if off is None:
            return False
        self.count[self._slot(key, off)] = 0
        return True

    def occupied(self):
        """The slots that hold a key, live or tombstone."""
        return {s for s, k in enumerate(self.keys) if k != EMPTY}

    def first_free_offset(self, home_slot):
        """The offset of the first empty slot from `home_slot` on, the bound left aside; None: the table has none."""
        for off in range(self.n_slots):
            if self.keys[(home_slot + off) & (self.n_slots - 1)] == EMPTY:
                return off
        return None

    def census(self):
        live = sum(1 for k, c in zip(self.keys, self.count) if k != EMPTY and c > 0)
        tomb = sum(1 for k, c in zip(self.keys, self.count) if k != EMPTY and c == 0)
        return dict(n_slots=self.n_slots, n_live=live, n_tombstones=tomb, n_points=sum(self.count), n_inconsistent=0)

    def live_keys(self):
        return sorted(k for k, c in zip(self.keys, self.count) if k != EMPTY and c > 0)


@functools.lru_cache(maxsize=None)
def _cells_and_hashes(radius):
    r = np.arange(-radius, radius, dtype=np.int64)
    ix, iy, iz = (a.reshape(-1) for a in np.meshgrid(r, r, r, indexing="ij"))      # three nested loops, i_x outermost, i_z innermost
    keys = pack_key(ix, iy, iz)
    return np.stack([ix, iy, iz], axis=1), keys, mix64_np(keys.astype(np.uint64))


@functools.lru_cache(maxsize=None)
def crafted_cells(n_slots, window_start, window, radius=64):
    """The cells of [-radius, radius)^3 whose home slot in a table of n_slots lies in [window_start, window_start + window) (mod n_slots):
    {home slot: int64 [k, 3] cells (i_x, i_y, i_z) in the order of three nested loops, i_x outermost}.  Cached per process; the arrays are
    read-only."""
    cells, _, hashed = _cells_and_hashes(radius)
    homes = (hashed & np.uint64(n_slots - 1)).astype(np.int64)
    out = {}
    for d in range(window):
        h = (window_start + d) & (n_slots - 1)
        c = cells[homes == h]
        c.setflags(write=False)
        out[h] = c
    return out


def window_cells(n_slots, window_start, window, radius=64):
    """All cells of crafted_cells(...) as one int64 [k, 3] array in the order of three nested loops, i_x outermost, i_z innermost."""
    cells = np.concatenate(list(crafted_cells(n_slots, window_start, window, radius).values()))
    return cells[np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))]


def cell_keys(cells):
    """Packed keys (Python-int-safe int64 array) of int cells [k, 3]."""
    c = np.asarray(cells, np.int64).reshape(-1, 3)
    return pack_key(c[:, 0], c[:, 1], c[:, 2])


def cell_points(cells, leaf, offsets=((0.0, 0.0, 0.0),)):
    """float32 points [k * len(offsets), 3] inside `cells`: the centre (i + 0.5) * leaf moved by each of `offsets` (in leaves, |o| < 0.5),
    offset-major: all cells at the first offset, then all at the second.  So a kernel tile of consecutive points holds as many
    distinct cells as it has points.  The test asserts through voxel_map_reference.Map that the library's own definition puts every
    point back in its cell."""
    c = np.asarray(cells, np.float64).reshape(-1, 3)
    return np.concatenate([((c + 0.5 + np.asarray(o, np.float64)) * float(np.float32(leaf))).astype(np.float32) for o in offsets])


class Scenario:
    """The crafted run the probe-bound tests share: a table of n_slots slots (larger than the bound), a window of `window` home slots from
    W on, chosen so that a run of MAX_PROBES slots from W wraps past the table's end.
      stage1   the first MAX_PROBES window cells: whatever the order, they occupy exactly [W, W + MAX_PROBES) (the CPU test holds that)
      chain    then one cell per call: home W (its first free slot is at offset MAX_PROBES: dropped), and for d = 1 .. window - 1 a cell
               of home W + d (first free slot at offset MAX_PROBES - 1, the last probe: accepted) and a second of that home (dropped)
      absent   64 further window cells that are never inserted
    The verdicts are not stored: model() replays the inserts on a Table."""

    def __init__(self, n_slots=4096, W=3096, window=8):
        assert n_slots > MAX_PROBES and W + MAX_PROBES > n_slots
        self.n_slots, self.W, self.window = n_slots, W, window
        cells = window_cells(n_slots, W, window)
        self.stage1 = cells[:MAX_PROBES]
        rest = cells[MAX_PROBES:]
        homes = np.array([home(k, n_slots) for k in cell_keys(rest).tolist()])
        pick, used = [], set()
        for d in [0] + [d for d in range(1, window) for _ in (0, 1)]:
            i = next(i for i in np.nonzero(homes == ((W + d) & (n_slots - 1)))[0].tolist() if i not in used)
            used.add(i)
            pick.append(i)
        self.chain = rest[pick]
        self.absent = rest[[i for i in range(len(rest)) if i not in used][:64]]

    def model(self, points_per_cell=1):
        """(the Table after stage 1 and the chain, the offsets the chain's inserts returned: None = dropped)."""
        t = Table(self.n_slots)
        for k in cell_keys(self.stage1).tolist():
            assert t.insert(k, points_per_cell) is not None
        return t, [t.insert(k, points_per_cell) for k in cell_keys(self.chain).tolist()]
