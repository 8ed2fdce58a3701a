"""CPU tests of the map rendered as a spherical frame: the numpy restatement (tests/map_render_reference.py) on hand-made cases -- its
fused multiply-add against exact rational arithmetic, the footprint with its seam and pole logic, the tie rule -- the two conditions
of the sphere scene the GPU test asserts, proven on the restatement first, and the agreement of the header, the ctypes binding and the
C++ adapter."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import map_render_reference as M
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
F = np.float32
LEAF = 0.05


def round_to_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the rational x, ties to even (normal range)."""
    if x == 0:
        return F(0)
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    scaled = x / Fraction(2) ** (e - 23)          # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return F(sign * float(n) * 2.0 ** (e - 23))


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    rng = np.random.default_rng(3)
    a = rng.normal(size=4000).astype(F)
    b = rng.normal(size=4000).astype(F)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.normal(size=4000) * 1e-6)).astype(F)      # heavy cancellation
    c[::3] = rng.normal(size=len(c[::3])).astype(F)
    # a case where rounding the float64 sum to nearest first gives the wrong float32: a b = 1 + 2^-24 + 2^-60, c = 2^-80
    a = np.concatenate([a, [F(1 + 2.0 ** -12), F(2.0 ** -30)]])
    b = np.concatenate([b, [F(1 + 2.0 ** -12), F(2.0 ** -30)]])
    c = np.concatenate([c, [F(-2.0 ** -11 + 2.0 ** -60), F(1 + 2.0 ** -24)]])
    got = M.fma32(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got):
        assert g == round_to_f32(Fraction(x) * Fraction(y) + Fraction(z)), (x, y, z)


def test_footprint_clips_rows_and_wraps_columns():
    rows, cols = 32, 64
    pix = M.footprint(0, 0, 2, rows, cols)
    assert sorted(pix.tolist()) == sorted(r * cols + c for r in (0, 1, 2) for c in (62, 63, 0, 1, 2))
    pix = M.footprint(31, 63, 1, rows, cols)
    assert sorted(pix.tolist()) == sorted(r * cols + c for r in (30, 31) for c in (62, 63, 0))
    assert M.footprint(5, 7, 0, rows, cols).tolist() == [5 * cols + 7]
    # 2 h + 1 >= cols: every column once, whatever the centre
    for h, tc in ((4, 3), (5, 0), (8, 7)):
        pix = M.footprint(3, tc, h, 16, 9)
        assert len(pix) == len(set(pix.tolist())) == (min(3 + h, 15) - max(3 - h, 0) + 1) * 9
    pix = M.footprint(3, 3, 3, 16, 8)          # 7 of 8 columns: one is left out
    assert len(set((pix % 8).tolist())) == 7 and 7 not in (pix % 8).tolist()


def test_half_width_truncates_and_saturates():
    k_inv = M.level_consts(32, 64)[0]
    foot = F(F(1.0) * F(LEAF)) * k_inv
    dist = np.array([0.0625, 0.125, 0.25, 0.5, 1.0, 1e-30, np.inf], F)
    h = M.half_width(dist, LEAF, 64, 1.0, 8)
    with np.errstate(all="ignore"):
        want = [min(8, int(foot * (F(1) / d))) for d in dist[:5]]
    assert h.tolist() == want + [8, 0] and want == [8, 4, 2, 1, 0]
    assert M.half_width(dist, LEAF, 64, 0.0, 8).tolist() == [0] * 7          # splat 0: single pixels, also where 0 x inf is not a number
    assert M.half_width(dist, LEAF, 64, 100.0, 0).tolist() == [0] * 7


def test_the_tie_goes_to_the_smaller_key():
    pix = np.array([5, 5, 5, 9, 9, 2])
    bits = np.array([700, 600, 600, 100, 100, 1])
    keys = np.array([1, 50, 40, 8, 7, 3])
    p, win = M.resolve(pix, bits, keys)
    assert p.tolist() == [2, 5, 9] and win.tolist() == [5, 2, 4]
    # the order of the candidates does not matter
    perm = np.array([3, 5, 0, 2, 4, 1])
    p2, win2 = M.resolve(pix[perm], bits[perm], keys[perm])
    assert p2.tolist() == p.tolist() and perm[win2].tolist() == win.tolist()


def single_points(points):
    """A map of single points at dyadic coordinates (each its own voxel's centroid), colours 10 k + (1, 2, 3)."""
    xyz = np.array(points, F)
    rgb = np.array([[10 * k + 1, 10 * k + 2, 10 * k + 3] for k in range(len(points))], np.uint8)
    ref = R.Map([(xyz, rgb, EYE)], LEAF, None)
    assert len(ref) == len(points) and {tuple(c) for c in ref.xyz.tolist()} == {tuple(c) for c in xyz.tolist()}
    return ref, xyz, rgb


SEAM_POLE_POINTS = [(0.0, -2.0 ** -8, -0.125), (-0.125, 2.0 ** -7, -0.125), (0.125, -2.0 ** -9, 0.0), (-0.125, 2.0 ** -9, 0.0)]


def test_seam_and_poles_on_the_restatement():
    """At 32 x 64: a point just past theta = -pi lands in column 0 and one just before +pi in column 63, both footprints wrap; a point
    near each pole lands in the first / last row and its footprint is clipped there."""
    rows, cols = 32, 64
    ref, xyz, rgb = single_points(SEAM_POLE_POINTS)
    Rinv, tinv = M.inverse_pose(EYE)
    tr, tc, d2, vis = M.warp_device(xyz, Rinv, tinv, rows, cols)
    assert vis.all() and tc[0] == 0 and tc[1] == 63 and tr[2] == 0 and tr[3] == 31
    h = M.half_width(np.sqrt(d2), LEAF, cols, 1.0, 8)
    assert (h >= 2).all()
    out = M.render(ref, LEAF, rows, cols, EYE)
    assert out["stats"] == dict(n_voxels=4, n_below_min_count=0, n_near=0, n_splatted=4, n_pixels_covered=int((out["count"] > 0).sum()))
    cols_of = lambda k: set(np.nonzero((out["rgb"][..., 0] == 10 * k + 1).any(axis=0))[0].tolist())
    rows_of = lambda k: set(np.nonzero((out["rgb"][..., 0] == 10 * k + 1).any(axis=1))[0].tolist())
    assert {0, 1, 63, 62} <= cols_of(0) and {63, 62, 0, 1} <= cols_of(1)
    assert rows_of(2) == set(range(0, int(h[2]) + 1)) and rows_of(3) == set(range(31 - int(h[3]), 32))
    # a point exactly at theta = +pi rounds to column `cols`: not visible, as in the dense alignment
    # ... and phi = 0 lies half way between rows 15 and 16: half up
    ref2, _, _ = single_points([(0.0, 0.0, -0.25), (0.0, -2.0 ** -12, -0.25)])
    out2 = M.render(ref2, LEAF, rows, cols, EYE, splat=0.0)
    assert out2["stats"]["n_near"] == 1 and out2["stats"]["n_splatted"] == 1 and out2["count"][16, 0] == 1 and out2["count"].sum() == 1


def test_tie_on_the_restatement():
    a, z = 2.0 ** -4, 0.25
    ref, xyz, _ = single_points([(0.0, a, -z), (0.0, -a, -z)])
    Rinv, tinv = M.inverse_pose(EYE)
    tr, tc, d2, vis = M.warp_device(ref.xyz, Rinv, tinv, 32, 64)
    assert vis.all() and d2[0] == d2[1] and tc[0] != tc[1]
    out = M.render(ref, LEAF, 32, 64, EYE, splat=4.0)
    own = [(out["key3"] == k).all(axis=2) for k in ref.key]
    assert own[0].sum() > own[1].sum() > 0          # ref.key is ascending: the first voxel has the smaller key and takes the shared pixels
    assert M.packed_keys(ref.key)[0] < M.packed_keys(ref.key)[1]
    assert (out["depth"][own[0] | own[1]] == np.sqrt(d2[0])).all()


def test_near_min_count_and_empty_inputs():
    ref, _, _ = single_points([(0.0, -2.0 ** -10, -0.03125), (0.0, -2.0 ** -10, -0.5)])
    out = M.render(ref, LEAF, 32, 64, EYE)
    assert out["stats"]["n_near"] == 1 and out["stats"]["n_splatted"] == 1          # 0.03125 < near = leaf
    out = M.render(ref, LEAF, 32, 64, EYE, min_count=2)
    assert out["stats"]["n_below_min_count"] == 2 and out["stats"]["n_pixels_covered"] == 0 and not out["depth"].any()
    empty = R.Map([], LEAF, None)
    out = M.render(empty, LEAF, 32, 64, EYE)
    assert out["stats"] == dict.fromkeys(M.STAT_NAMES, 0) and out["depth"].shape == (32, 64)


def sphere_scene_checks(out, rows, cols, radius, leaf):
    """The two conditions of the sphere scene, on a render (the restatement's here, the device's in the GPU test)."""
    d = out["depth"]
    hit = out["count"] > 0
    lo, hi = radius - leaf * np.sqrt(3.0), radius * (1 + 2.0 ** -20)
    assert hit.any() and (d[hit] >= lo).all() and (d[hit] <= hi).all(), (d[hit].min(), d[hit].max(), lo, hi)
    phi = (0.5 * rows - 0.5 - np.arange(rows)) * (2 * np.pi / cols)
    band = np.abs(phi) <= np.radians(30.0)
    assert band.sum() >= rows // 4 and hit[band].all(), int((~hit[band]).sum())


def test_sphere_scene_conditions_hold_on_the_restatement(oracle_mod):
    rows, cols, radius = 128, 256, 1.5
    depth = np.full((rows, cols), radius, F)
    cloud = oracle_mod.sphere_cloud(depth, 2)
    P = R.general_pose()
    ref = R.Map([(cloud, None, P)], LEAF, None)
    out = M.render(ref, LEAF, rows, cols, P, splat=2.5, max_half=32)
    print("voxels", len(ref), "stats", out["stats"])
    sphere_scene_checks(out, rows, cols, radius, LEAF)


def test_header_binding_and_adapter_agree():
    from rgbd360_amd import _lib, build
    L = C.CDLL(build.build())
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    for name in ("rgbd360_map_default_render_params", "rgbd360_map_render_sphere", "rgbd360_map_render_sphere_dev"):
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS
    assert re.search(r"\brgbd360_map_time_render\s*\(", diag) and "rgbd360_map_time_render" not in main and hasattr(L, "rgbd360_map_time_render")

    def fields(text, struct):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, text).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
        return names

    for struct, cls, size in (("rgbd360_map_render_params", _lib.MapRenderParams, 16), ("rgbd360_map_render_stats", _lib.MapRenderStats, 40)):
        assert fields(main, struct) == [n for n, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    assert [n for n, _ in _lib.MapRenderStats._fields_] == list(M.STAT_NAMES)
    L.rgbd360_map_default_render_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapRenderParams)]
    L.rgbd360_map_default_render_params.restype = None
    p = _lib.MapRenderParams()
    L.rgbd360_map_default_render_params(None, C.byref(p))
    assert (p.min_count, p.max_half) == (1, 8) and p.splat == 1.0 and p.near == F(0.05)
    assert (M.DEFAULTS["min_count"], M.DEFAULTS["splat"], M.DEFAULTS["max_half"]) == (p.min_count, p.splat, p.max_half)
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("renderSphere", "renderParams", "renderStats", "rgbd360_map_render_sphere", "rgbd360_map_default_render_params"):
        assert name in hpp, name
    py = open(os.path.join(ROOT, "rgbd360_amd", "voxel_map.py")).read()
    assert "def render_sphere" in py and "def render_params" in py
    assert "--render-map" in open(os.path.join(ROOT, "examples", "odometry_replay.cpp")).read()
    assert "rgbd360_map_render_sphere" in open(os.path.join(ROOT, "README.md")).read()
