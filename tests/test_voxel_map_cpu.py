"""CPU tests of the voxel map: the numpy restatement of its definition (tests/voxel_map_reference.py) against a plain Python loop over a
dict on hand-made points around every decision of the definition, and the new symbols in the built library."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dict_loop_map(clouds, leaf, box):
    """The definition point by point: numpy float32 SCALARS for the float32 steps (each operation rounds once), Python integers for
    the sums, a dict keyed by (i_z, i_y, i_x)."""
    f = np.float32
    inv_leaf = f(1.0) / f(leaf)
    cells = {}
    totals = dict(n_valid=0, n_box_rejected=0, n_out_of_range=0, n_added=0)
    for xyz, rgb, pose in clouds:
        T = [[f(v) for v in row] for row in np.asarray(pose, np.float32).reshape(4, 4)]
        for n, p in enumerate(np.asarray(xyz, np.float32).reshape(-1, 3)):
            x, y, z = f(p[0]), f(p[1]), f(p[2])
            if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
                continue
            totals["n_valid"] += 1
            if box is not None and not all(f(box[0][k]) <= p[k] <= f(box[1][k]) for k in range(3)):
                totals["n_box_rejected"] += 1
                continue
            with np.errstate(all="ignore"):
                w = [f(f(f(f(T[k][0] * x) + f(T[k][1] * y)) + f(T[k][2] * z)) + T[k][3]) for k in range(3)]
            if not all(math.isfinite(v) and abs(float(v)) < 4096.0 for v in w):
                totals["n_out_of_range"] += 1
                continue
            totals["n_added"] += 1
            i = [int(math.floor(float(f(v * inv_leaf)))) for v in w]
            cell = cells.setdefault((i[2], i[1], i[0]), [0, [0, 0, 0], [0, 0, 0]])
            cell[0] += 1
            for k in range(3):
                cell[1][k] += round(float(w[k]) * 1048576.0)          # exact product, Python's round is half to even
                if rgb is not None:
                    cell[2][k] += int(rgb[n][k])
    return cells, totals


CASES = R.edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_the_point_by_point_loop(case):
    name, xyz, rgb, pose, leaf, box = case
    ref = R.Map([(xyz, rgb, pose)], leaf, box)
    cells, totals = dict_loop_map([(xyz, rgb, pose)], leaf, box)
    assert {k: ref.stats[0][k] for k in totals} == totals
    assert ref.stats[0]["n_voxels"] == len(cells) == len(ref)
    order = sorted(cells)
    assert [tuple(k) for k in ref.key[:, ::-1].tolist()] == order
    for row, key in enumerate(order):
        n, S, Csum = cells[key]
        assert int(ref.count[row]) == n
        assert ref.S[row].tolist() == S and ref.C[row].tolist() == Csum
        assert ref.xyz[row].tolist() == [float(np.float32(s / (n * 1048576.0))) for s in S]
        assert ref.rgb[row].tolist() == [c // n for c in Csum]


def test_edge_cases_decide_what_their_comments_say():
    """The hand-made points do exercise the decisions they are named after (the restatement's answer, stated by hand here)."""
    name, xyz, rgb, pose, leaf, box = CASES[0]
    ref = R.Map([(xyz, rgb, pose)], leaf, box)
    keys = {tuple(k) for k in ref.key.tolist()}
    assert (0, 0, 0) in keys and (-1, -1, -1) in keys                     # -0.0 in cell 0, -0.01 in cell -1
    assert (5, 5, 5) in keys and (4, 4, 4) in keys and (-5, -5, -5) in keys and (-6, -6, -6) in keys      # a boundary belongs to the upper cell
    st = ref.stats[0]
    assert st["n_valid"] == len(xyz) - 6                                   # three NaN rows, two Inf rows, one mixed
    assert st["n_out_of_range"] == 5 and st["n_box_rejected"] == 0        # +-4096 three times, 1e9, -3e38; the float below 4096 stays
    cell0 = ref.key.tolist().index([0, 0, 0])
    assert int(ref.count[cell0]) == 3                                      # -0.0 / 0.0 twice and (0.01, 0.01, 0.01); the mixed-sign rows lie elsewhere
    name, xyz, rgb, pose, leaf, box = CASES[2]
    ref = R.Map([(xyz, rgb, pose)], leaf, box)
    assert ref.stats[0]["n_box_rejected"] == 6 + 3 and ref.stats[0]["n_added"] == 12 + 3      # per limit: itself and its inner neighbour stay
    name, xyz, rgb, pose, leaf, box = CASES[4]
    ref = R.Map([(xyz, rgb, pose)], leaf, box)
    assert ref.stats[0]["n_out_of_range"] == 2 and ref.stats[0]["n_added"] == 4


def test_half_units_round_to_even():
    h = np.float32(2.0) ** -21
    xyz = np.array([(h, 3 * h, 5 * h), (-h, -3 * h, 7 * h)], np.float32)
    ref = R.Map([(xyz, None, np.eye(4, dtype=np.float32))], 1.0, None)
    assert ref.key.tolist() == [[-1, -1, 0], [0, 0, 0]]
    assert ref.S.tolist() == [[0, -2, 4], [0, 2, 2]]


def test_library_exports_the_map_symbols():
    """Every rgbd360_map_* the headers declare is in the built library and in the ctypes binding."""
    from rgbd360_amd import _lib, build
    L = C.CDLL(build.build())
    decl = set()
    for hdr in ("rgbd360_hip.h", "rgbd360_hip_diag.h"):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
        decl |= set(re.findall(r"\b(rgbd360_map_[a-z0-9_]+)\s*\(", txt))
    want = {"rgbd360_map_create", "rgbd360_map_destroy", "rgbd360_map_last_error", "rgbd360_map_bytes", "rgbd360_map_set_box",
            "rgbd360_map_insert_sphere", "rgbd360_map_insert_cloud", "rgbd360_map_size", "rgbd360_map_clear", "rgbd360_map_extract",
            "rgbd360_map_extract_dev"}
    assert want <= decl
    for name in sorted(decl):
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS, name
    txt = open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read()
    assert re.search(r"RGBD360_MAP_FULL\s*=\s*3\b", txt) and re.search(r"RGBD360_NO_VALID_PIXELS\s*=\s*2\b", txt)
    assert C.sizeof(_lib.MapStats) == 48
