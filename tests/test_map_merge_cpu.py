"""CPU tests of composing voxel maps (csrc/map_merge.h) on the numpy restatement (tests/map_merge_reference.py): a
sum-mode merge is the map of both clouds word for word, pose-mode terms keep the census rules, un-merge is the exact inverse and counts
what the contract forbids; the new symbols, structs and defaults agree between the headers, the library and the binding; the GlobalMap
members and the example compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_merge_reference as M
import voxel_map_edit_reference as E
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rgbd360_map_default_merge_params", "rgbd360_map_merge", "rgbd360_map_unmerge", "rgbd360_map_records", "rgbd360_map_add_records")


def random_cloud(n=5000, seed=5):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.5, 1.0, (n, 3)).astype(np.float32)
    xyz[: n // 4] = (xyz[: n // 4] * np.float32(0.1)).astype(np.float32)        # a crowded corner: voxels of many points
    return xyz, rng.integers(0, 256, (n, 3)).astype(np.uint8)


def split(case):
    """One edge case as two clouds: the even and the odd points."""
    name, xyz, rgb, pose, leaf, box = case
    halves = [(xyz[k::2], None if rgb is None else rgb[k::2], pose) for k in (0, 1)]
    return name, halves, (xyz, rgb, pose), leaf, box


def merge_map(clouds, leaf, box):
    m = M.MergeMap(leaf, box)
    for c in clouds:
        m.insert(*c)
    return m


@pytest.mark.parametrize("case", R.edge_cases(), ids=lambda c: c[0])
def test_sum_mode_is_the_map_of_both_clouds_on_the_edge_cases(case):
    name, halves, whole, leaf, box = split(case)
    a, b = merge_map(halves[:1], leaf, box), merge_map(halves[1:], leaf, box)
    st = a.merge(b.read_out())
    M.check_stats_add_up(st)
    ref = R.Map([whole], leaf, box)
    E.assert_same_map(a.read_out(), ref, name)
    assert np.array_equal(M.records_of(a.read_out()), M.records_of(ref)) and st["n_voxels"] == len(ref)
    assert a.census()["n_inconsistent"] == 0


def test_sum_mode_is_the_map_of_both_clouds_on_a_random_cloud():
    xyz, rgb = random_cloud()
    P = R.general_pose()
    a, b = merge_map([(xyz[:2500], rgb[:2500], P)], 0.05, R.DEFAULT_BOX), merge_map([(xyz[2500:], rgb[2500:], P)], 0.05, R.DEFAULT_BOX)
    st = a.merge(b.read_out())
    ref = R.Map([(xyz, rgb, P)], 0.05)
    assert 1000 < len(b) and 0 < st["n_voxels_new"] < st["n_voxels_added"] == len(b)      # shared and new voxels both
    E.assert_same_map(a.read_out(), ref)
    # min_count: the voxels below it stay out and are counted
    c = merge_map([(xyz[:2500], rgb[:2500], P)], 0.05, R.DEFAULT_BOX)
    st = c.merge(b.read_out(), None, 3)
    M.check_stats_add_up(st)
    few = int((b.read_out().count < 3).sum())
    assert 0 < few == st["n_voxels_below_min_count"] and st["n_voxels_added"] == len(b) - few


@pytest.mark.parametrize("dst_leaf", [0.05, 0.02, 0.25])
def test_pose_mode_terms_keep_the_census_rules_and_unmerge_is_exact(dst_leaf):
    xyz, rgb = random_cloud()
    src = R.Map([(xyz, rgb, np.eye(4, dtype=np.float32))], 0.05)
    P = R.general_pose()
    keys, rows, st = M.terms(src, P, dst_leaf)
    assert len(keys) == len(src) and M.census_rules_hold(rows) and st["n_voxels_out_of_range"] == 0
    assert rows[:, 0].sum() == src.count.sum() and np.array_equal(rows[:, 4:7], src.C)
    dst = M.MergeMap(dst_leaf, None)
    other = (xyz[:700] + np.float32(0.3), rgb[:700], P)
    st = dst.merge(src, P)
    M.check_stats_add_up(st)
    assert dst.census()["n_inconsistent"] == 0 and dst.census()["n_points"] == src.count.sum()
    dst.insert(*other)
    st = dst.unmerge(src, P)
    M.check_stats_add_up(st)
    assert st["n_missing"] == st["n_underflow"] == 0 and st["n_points_added"] == src.count.sum()
    only = M.MergeMap(dst_leaf, None)
    only.insert(*other)
    E.assert_same_map(dst.read_out(), only.read_out())
    assert dst.census()["n_inconsistent"] == 0 and dst.census()["n_tombstones"] == st["n_voxels_new"] > 0


def test_unmerge_outside_the_contract_counts_and_never_wraps():
    xyz, rgb = random_cloud(2000)
    eye = np.eye(4, dtype=np.float32)
    src = R.Map([(xyz, rgb, eye)], 0.05, None)
    dst = M.MergeMap(0.05, None)
    dst.insert(xyz[::2], rgb[::2], eye)              # holds part of what the source holds
    held = dst.read_out()
    st = dst.unmerge(src)
    M.check_stats_add_up(st)
    assert st["n_missing"] > 0 and st["n_underflow"] > 0 and st["n_points_added"] + st["n_missing"] + st["n_underflow"] == src.count.sum()
    assert st["n_points_added"] == held.count.sum() and len(dst) == 0      # every voxel held is a voxel of the source: all taken, none below zero
    assert all(r[0] >= 0 for r in dst.rows.values())


def test_records_round_trip_and_bad_records():
    xyz, rgb = random_cloud(1500)
    ref = R.Map([(xyz, rgb, R.general_pose())], 0.05)
    rec = M.records_of(ref)
    assert rec.dtype == np.uint64 and rec.shape == (len(ref), 8) and (np.diff(rec[:, 0].astype(np.int64)) > 0).all() and not M.bad_records(rec).any()
    m = M.MergeMap(0.05)
    m.add_records(np.concatenate([rec, rec[:10]]))       # equal keys add up
    twice = m.read_out()
    assert np.array_equal(twice.count[:10], 2 * ref.count[:10]) and np.array_equal(twice.S[10:], ref.S[10:])
    one = rec[:1].copy()
    n = int(one[0, 1])
    for word, value in ((0, 0xFFFFFFFFFFFFFFFF), (0, 1 << 63), (1, 0), (1, 1 << 31), (5, 256 * n), (5, 255 * n + 1), (2, n << 32),
                        (3, (-(n << 32)) & 0xFFFFFFFFFFFFFFFF)):
        bad = one.copy()
        bad[0, word] = value
        assert M.bad_records(bad).all(), (word, value)
    for word, value in ((5, 255 * n), (2, (n << 32) - 1), (3, (-(n << 32) + 1) & 0xFFFFFFFFFFFFFFFF), (1, max(n, (1 << 31) - 1))):
        good = one.copy()
        good[0, word] = value
        assert not M.bad_records(good).any(), (word, value)


def test_new_symbols_structs_and_defaults(tmp_path):
    from rgbd360_amd import _lib, build
    L = C.CDLL(build.build())
    main_txt = open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read()
    main = re.sub(r"/\*.*?\*/", "", main_txt, flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS, name
    name = "rgbd360_map_time_merge"
    assert re.search(r"\b%s\s*\(" % name, diag) and name not in main and hasattr(L, name) and name in _lib.SYMBOLS

    def fields(struct):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, main).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
        return names

    assert fields("rgbd360_map_merge_params") == [n for n, _ in _lib.MapMergeParams._fields_]
    assert fields("rgbd360_map_merge_stats") == [n for n, _ in _lib.MapMergeStats._fields_] == list(M.STAT_NAMES)
    # the structs' sizes as a C compiler lays them out
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "rgbd360_hip.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(rgbd360_map_merge_params), sizeof(rgbd360_map_merge_stats)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [C.sizeof(_lib.MapMergeParams), C.sizeof(_lib.MapMergeStats)] == [4, 8 * len(M.STAT_NAMES)]
    # the default: in the header's comment, in the library and in the restatement
    assert int(re.search(r"int min_count;\s*/\*[^*]*: (\d+) \*/", main_txt).group(1)) == M.DEFAULT_MIN_COUNT == 1
    L.rgbd360_map_default_merge_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapMergeParams)]
    L.rgbd360_map_default_merge_params.restype = None
    p = _lib.MapMergeParams(min_count=77)
    L.rgbd360_map_default_merge_params(None, C.byref(p))
    assert p.min_count == M.DEFAULT_MIN_COUNT
    # entries that need no device: no map
    for f in (L.rgbd360_map_merge, L.rgbd360_map_unmerge):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        assert f(None, None, None, None, None) == -1
    L.rgbd360_map_records.restype = C.c_longlong
    L.rgbd360_map_records.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
    L.rgbd360_map_add_records.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
    assert L.rgbd360_map_records(None, 0, None) == -1 and L.rgbd360_map_add_records(None, None, 0, 0, None) == -1
    py = open(os.path.join(ROOT, "rgbd360_amd", "voxel_map.py")).read()
    for name in ("def merge", "def unmerge", "def records", "def add_records", "def save", "def load"):
        assert name in py, name
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "rgbd360_map_merge" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "profiles", "map_merge_perf.txt"))


def test_global_map_members_compile_and_link(tmp_path):
    from rgbd360_amd import build
    lib = build.build()
    src = tmp_path / "use_merge.cpp"
    src.write_text('''
#include "rgbd360/GlobalMap.hpp"
int main(int argc, char**) {
    if (argc < 100) return 0;      // linked, not run: it would need a device
    rgbd360::RegisterPhotoICP align;
    rgbd360::GlobalMap a(align), b(align);
    rgbd360::Mat4f pose = rgbd360::Mat4f::Identity();
    rgbd360_map_merge_params p = a.mergeParams();
    bool ok = a.merge(b) && a.merge(b, &pose, &p) && a.unmerge(b, &pose, &p) && a.unmerge(b);
    std::vector<uint64_t> rec = a.records();
    ok = ok && b.addRecords(rec);
    const rgbd360_map_merge_stats& st = a.mergeStats();
    return ok && st.n_voxels_read == st.n_voxels_added ? 0 : 1;
}
''')
    exe = tmp_path / "use_merge"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.dirname(lib),
                           "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_the_example_compiles_with_wall(tmp_path):
    from rgbd360_amd import build
    lib = build.build()
    exe = tmp_path / "submap_compose"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "submap_compose.cpp"), "-L" + os.path.dirname(lib), "-lrgbd360_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 2 and subprocess.call([str(exe), str(tmp_path / "missing"), "2", "8", "8", "1", str(tmp_path / "none")]) == 3
