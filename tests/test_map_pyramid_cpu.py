"""CPU tests of the map pyramid and the coarse-to-fine chain (csrc/map_pyramid.h) on the numpy restatement
(tests/map_pyramid_reference.py): the shift-merge of a map equals the map built directly at the coarser leaf, word for word; the new
symbols and structs agree between the headers, the library and the binding; the Python mirror's refusals; and the number the feature is
for -- from 0.15 m / 0.03 rad the single-level ICP stalls more than a leaf from the truth and the chain ends where the single level
ends from an easy guess."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_align_reference as A
import map_pyramid_reference as Y
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 0.05


@pytest.fixture(scope="module")
def world(oracle_mod, small_pair):
    """The first synthetic frame's convention-2 cloud with its colours at the general pose, in a map of 0.05 m."""
    rgb, depth = small_pair[0]
    cloud = oracle_mod.sphere_cloud(depth, 2)
    P = R.general_pose()
    return dict(cloud=cloud, rgb=rgb.reshape(-1, 3), P=P, map=R.Map([(cloud, rgb.reshape(-1, 3), P)], LEAF))


@pytest.mark.parametrize("s", [1, 2, 3])
def test_shift_merge_equals_the_map_built_at_the_coarser_leaf(world, s):
    direct = R.Map([(world["cloud"], world["rgb"], world["P"])], Y.level_leaf(LEAF, s))
    merged = Y.Level(world["map"], s)
    assert 100 < len(direct) < len(world["map"]) and merged.n_points == world["map"].n_passing
    Y.assert_words_equal(merged, direct, "s = %d" % s)
    if s > 1:       # level s out of level s - 1 is level s out of level 0: integer adds
        Y.assert_words_equal(Y.Level(Y.Level(world["map"], s - 1), 1), direct, "chained, s = %d" % s)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_shift_merge_on_indices_straddling_zero(s):
    pts, rgb = Y.straddling_points()
    eye = np.eye(4, dtype=np.float32)
    fine = R.Map([(pts, rgb, eye)], 0.25, None)
    assert fine.key.min() == -4 and fine.key.max() == 3
    merged = Y.Level(fine, s)
    Y.assert_words_equal(merged, R.Map([(pts, rgb, eye)], Y.level_leaf(0.25, s), None), "s = %d" % s)
    keys = {tuple(k) for k in merged.key.tolist()}
    if s == 1:      # -1 and 0 stay apart; -1 and -2 merge
        assert (-1, -1, -1) in keys and (0, 0, 0) in keys
        row = {tuple(k): c for k, c in zip(merged.key.tolist(), merged.count.tolist())}
        both = {tuple(k): c for k, c in zip(fine.key.tolist(), fine.count.tolist())}
        assert row[(-1, -1, -1)] == sum(both[(a, b, c)] for a in (-2, -1) for b in (-2, -1) for c in (-2, -1))
        assert row[(0, 0, 0)] == sum(both[(a, b, c)] for a in (0, 1) for b in (0, 1) for c in (0, 1))
    assert merged.key.min() == -4 >> s and merged.key.max() == 3 >> s


def test_new_symbols_structs_and_defaults():
    from rgbd360_amd import _lib, build
    L = C.CDLL(build.build())
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    for name in ("rgbd360_map_level", "rgbd360_map_pyramid_bytes", "rgbd360_map_release_levels", "rgbd360_map_default_c2f_params",
                 "rgbd360_map_align_c2f_sphere", "rgbd360_map_align_c2f_cloud"):
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS, name
    name = "rgbd360_map_time_coarsen"
    assert re.search(r"\b%s\s*\(" % name, diag) and name not in main and hasattr(L, name) and name in _lib.SYMBOLS
    assert int(re.search(r"#define\s+RGBD360_MAP_MAX_SHIFT\s+(\d+)", main).group(1)) == _lib.MAP_MAX_SHIFT == Y.MAX_SHIFT == 6

    def fields(struct):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, main).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
        return names

    for struct, cls, size in (("rgbd360_map_c2f_params", _lib.MapC2fParams, 40), ("rgbd360_map_c2f_level", _lib.MapC2fLevel, 120),
                              ("rgbd360_map_c2f_result", _lib.MapC2fResult, 8 + 7 * 120 + 42 * 4)):
        assert fields(struct) == [n for n, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    L.rgbd360_map_default_c2f_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapC2fParams)]
    L.rgbd360_map_default_c2f_params.restype = None
    p = _lib.MapC2fParams()
    L.rgbd360_map_default_c2f_params(None, C.byref(p))
    assert (p.top_shift, p.kind, p.max_iters, p.min_count, p.min_matches, p.min_support) == (3, 0, 10, 1, 6, 5)
    assert p.eps == np.float32(1e-6) and p.max_dist_leaves == 1.0 and p.max_flatness == np.float32(0.05)
    # entries that need no device: no map, no levels
    L.rgbd360_map_pyramid_bytes.restype = C.c_size_t
    L.rgbd360_map_pyramid_bytes.argtypes = [C.c_void_p]
    L.rgbd360_map_level.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.rgbd360_map_release_levels.argtypes = [C.c_void_p]
    h = C.c_void_p(1)
    assert L.rgbd360_map_pyramid_bytes(None) == 0 and L.rgbd360_map_release_levels(None) == -1
    assert L.rgbd360_map_level(None, 1, C.byref(h)) == -1 and not h.value
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("alignSphereCoarseToFine", "alignCloudCoarseToFine", "c2fParams", "c2fResult", "pyramidBytes", "rgbd360_map_align_c2f_sphere",
                 "rgbd360_map_align_c2f_cloud", "rgbd360_map_default_c2f_params", "rgbd360_map_pyramid_bytes"):
        assert name in hpp, name
    py = open(os.path.join(ROOT, "rgbd360_amd", "voxel_map.py")).read()
    for name in ("def level", "def pyramid_bytes", "def release_levels", "def align_sphere_c2f", "def align_cloud_c2f"):
        assert name in py, name


def test_the_mirror_refuses_bad_shifts_and_radii():
    from rgbd360_amd import _lib
    from rgbd360_amd.register import Rgbd360Error
    from rgbd360_amd.voxel_map import check_c2f_params, check_shift
    assert [check_shift(s) for s in (1, 3, 6)] == [1, 3, 6] and check_shift(0, 0) == 0
    for bad in (0, -1, 7, 1.5, True):
        with pytest.raises(Rgbd360Error):
            check_shift(bad)

    def params(**fields):
        p = _lib.MapC2fParams()
        _lib.load().rgbd360_map_default_c2f_params(None, C.byref(p))
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    assert check_c2f_params(params()).top_shift == 3
    assert check_c2f_params(params(top_shift=0, kind=1, max_dist_leaves=0.5)).kind == 1
    for bad in (dict(max_dist_leaves=0.0), dict(max_dist_leaves=-0.5), dict(max_dist_leaves=1.0000001), dict(max_dist_leaves=float("nan")),
                dict(top_shift=7), dict(top_shift=-1), dict(kind=2)):
        with pytest.raises(Rgbd360Error):
            check_c2f_params(params(**bad))


def test_the_chain_reaches_what_a_single_level_cannot(world):
    """0.15 m / 0.03 rad off, seeds 1 - 12: the single-level ICP (max_dist = leaf) ends more than one leaf from the truth; the chain over
    leaves 0.4, 0.2, 0.1, 0.05 ends within twice the error the single level reaches from the easy guess of the existing loop tests
    (0.01 m / 0.003 rad, seed 6)."""
    tgt = R.Map([(world["cloud"], None, world["P"])], LEAF)
    easy = A.Alignment(tgt, world["cloud"], A.perturbed(world["P"], 0.01, 0.003, 6), LEAF, R.DEFAULT_BOX, LEAF)
    easy_t = A.pose_error(easy.pose, world["P"])[1]
    assert easy.status == A.OK and easy_t < 1e-3
    maps = {}
    for seed in range(1, 13):
        guess = A.perturbed(world["P"], 0.15, 0.03, seed)
        single = A.Alignment(tgt, world["cloud"], guess, LEAF, R.DEFAULT_BOX, LEAF)
        chain = Y.Chain(tgt, world["cloud"], guess, LEAF, R.DEFAULT_BOX, maps=maps)
        t_single, (r_chain, t_chain) = A.pose_error(single.pose, world["P"])[1], A.pose_error(chain.pose, world["P"])
        print("seed %2d: single level %.4f m (%d matched), chain %.3e m %.3e rad, iterations %s" %
              (seed, t_single, single.n_matched, t_chain, r_chain, [lv["al"].iterations for lv in chain.levels]))
        assert t_single > LEAF, seed
        assert chain.status == A.OK and t_chain <= 2.0 * easy_t, (seed, t_chain, easy_t)
