"""CPU tests of the voxel map's editing (rgbd360_map_remove_* / _move_* / _rehash / _census): the numpy restatement's removal is the
exact inverse of its insertion, the header, the ctypes binding, the Python adapter and the C++ adapter agree, and the C++ adapter
and the replay example compile against the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_align_reference as A
import voxel_map_edit_reference as E
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def frames():
    """The GPU tests' three frames (the conftest pair's scene along its trajectory) as numpy clouds with colours and poses."""
    from rgbd360_amd import synth
    out = []
    for k in range(3):
        T = synth.trajectory_pose(k)
        rgb, depth = synth.render(T, 256, 128, 1234)
        out.append((A.sphere_cloud_np(depth), rgb.reshape(-1, 3), T.astype(np.float32)))
    return out


def test_removal_is_the_exact_inverse_in_the_restatement(frames):
    m = E.EditMap(0.05)
    for f in frames:
        m.insert(*f)
    E.assert_same_map(m.read_out(), R.Map(frames, 0.05), "three frames")
    before = {k: int(r[0]) for k, r in m.rows.items()}
    st = m.remove(*frames[1])
    ref = R.Map([frames[0], frames[2]], 0.05)
    E.assert_same_map(m.read_out(), ref, "frame 1 removed")
    # the three classes of voxels a removal meets: emptied, touched and surviving, untouched
    touched = {k for k, _ in zip(*E.rows_of(*frames[1], 0.05, R.DEFAULT_BOX)[:2])}
    emptied = sum(1 for k in touched if m.rows[k][0] == 0)
    surviving = len(touched) - emptied
    untouched = len(before) - len(touched)
    print("emptied", emptied, "touched and surviving", surviving, "untouched", untouched, "of", len(before))
    assert min(emptied, surviving, untouched) > 1000
    assert st["n_voxels_emptied"] == emptied and st["n_missing"] == st["n_underflow"] == 0 and st["n_removed"] == R.Map([frames[1]], 0.05).n_passing
    c = m.census()
    assert c == dict(n_live=len(ref), n_tombstones=emptied, n_points=int(ref.count.sum()), n_inconsistent=0)
    # tombstones are absent from the read-out; a revival brings the map back; rehash drops them
    assert len(m.read_out()) == len(ref) == len(m) and len(m.rows) == len(ref) + emptied
    m.insert(*frames[1])
    E.assert_same_map(m.read_out(), R.Map(frames, 0.05), "revived")
    assert m.census()["n_tombstones"] == 0 and len(m.rows) == len(before)
    for f in frames:
        assert m.remove(*f)["n_missing"] == 0
    assert len(m) == 0 and m.census() == dict(n_live=0, n_tombstones=len(before), n_points=0, n_inconsistent=0)
    m.rehash()
    assert len(m.rows) == 0


def test_restatement_outside_the_contract():
    """One voxel asked for more than it holds gives what it holds; a voxel that was never there is missing; a tombstone underflows."""
    leaf = 0.5
    a = np.array([(0.1, 0.1, 0.1), (0.2, 0.2, 0.2), (0.7, 0.1, 0.1)], np.float32)
    b = np.array([(0.1, 0.2, 0.1), (0.3, 0.2, 0.2), (0.4, 0.4, 0.4), (1.2, 0.1, 0.1)], np.float32)
    m = E.EditMap(leaf, None)
    m.insert(a, None, EYE)
    st = m.remove(b, None, EYE)
    assert (st["n_removed"], st["n_underflow"], st["n_missing"], st["n_voxels_emptied"]) == (2, 1, 1, 1)
    assert len(m) == 1 and m.census()["n_points"] == 1
    st = m.remove(b, None, EYE)
    assert (st["n_removed"], st["n_underflow"], st["n_missing"]) == (0, 3, 1)


def _fields(text, struct):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, text).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
    return names


def test_header_binding_and_adapters_agree():
    from rgbd360_amd import _lib, build, voxel_map
    L = C.CDLL(build.build())
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    entries = ("rgbd360_map_remove_sphere", "rgbd360_map_remove_cloud", "rgbd360_map_move_sphere", "rgbd360_map_move_cloud", "rgbd360_map_rehash",
               "rgbd360_map_census")
    for name in entries:
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS, name
    assert re.search(r"\brgbd360_map_time_edit\s*\(", diag) and "rgbd360_map_time_edit" not in main and hasattr(L, "rgbd360_map_time_edit")
    assert re.search(r"\bRGBD360_MAP_MISMATCH\s*=\s*4\b", main) and voxel_map.MAP_MISMATCH == 4
    assert "Out of scope: removing points" not in open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read()
    for struct, cls, names in (("rgbd360_map_edit_stats", _lib.MapEditStats, list(E.EDIT_STAT_NAMES)),
                               ("rgbd360_map_census_counts", _lib.MapCensus, ["n_slots", "n_live", "n_tombstones", "n_points", "n_inconsistent"])):
        assert _fields(main, struct) == [n for n, _ in cls._fields_] == names, struct
        assert C.sizeof(cls) == 8 * len(names), struct
    # a null map is refused by every entry before anything else is looked at
    L.rgbd360_map_rehash.argtypes = [C.c_void_p, C.c_longlong]
    L.rgbd360_map_census.argtypes = [C.c_void_p, C.c_void_p]
    assert L.rgbd360_map_rehash(None, 0) == -1 and L.rgbd360_map_census(None, None) == -1
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in entries + ("bool remove(", "bool move(", "bool rehash(long long capacity = 0)", "census() const", "editStats() const"):
        assert name in hpp, name
    assert hpp.count("bool remove(") == 2 and hpp.count("bool move(") == 2
    for name in ("remove_sphere", "remove_cloud", "move_sphere", "move_cloud", "rehash", "census"):
        assert callable(getattr(voxel_map.VoxelMap, name)), name
    example = open(os.path.join(ROOT, "examples", "odometry_replay.cpp")).read()
    assert "--map-window" in example and "globalMap->remove(" in example and "globalMap->rehash()" in example


_SNIPPET = r'''
#include "rgbd360/GlobalMap.hpp"
int use(rgbd360::GlobalMap& g, const rgbd360::ImageView& rgb, const rgbd360::ImageView& depth, const rgbd360::Mat4f& a, const rgbd360::Mat4f& b,
        const float* xyz, const uint8_t* rgb3) {
    bool ok = g.remove(rgb, depth, a) && g.remove(xyz, rgb3, 10, a) && g.move(rgb, depth, a, b, 2) && g.move(xyz, rgb3, 10, a, b) && g.rehash() && g.rehash(1 << 20);
    const rgbd360_map_census_counts c = g.census();
    const rgbd360_map_edit_stats& e = g.editStats();
    return ok && c.n_tombstones <= c.n_slots && e.n_removed >= e.n_voxels_emptied ? RGBD360_MAP_MISMATCH : 0;
}
'''


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_headers"])
def test_adapter_and_example_compile_against_the_header(tmp_path, mock):
    extra = ["-I" + os.path.join(ROOT, "tests", "mock_headers")] if mock else []
    src = tmp_path / "edit_snippet.cpp"
    src.write_text(_SNIPPET)
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + extra
    subprocess.check_call(base + [str(src)])
    subprocess.check_call(base + [os.path.join(ROOT, "examples", "odometry_replay.cpp")])
    # and the header is C: the two structs, the status and the entries parse as C99
    c_src = tmp_path / "edit_c.c"
    c_src.write_text('#include "rgbd360_hip.h"\nint f(rgbd360_map* m) { rgbd360_map_census_counts c; rgbd360_map_edit_stats e; e.n_missing = 0; '
                     'return rgbd360_map_census(m, &c) + rgbd360_map_rehash(m, 0) + (int)e.n_missing + RGBD360_MAP_MISMATCH; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(c_src)])
