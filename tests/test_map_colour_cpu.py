"""CPU tests of the voxel map's colour layer and of coloured ICP against the map: the restated gradient fit (tests/map_colour_reference.py)
on an analytic field; the library's host compile of the fit against the restatement, bit for bit; the agreement of the headers, the
library, the ctypes binding, the Python wrapper's refusals and the C++ adapter; and the restated loop on the sliding scene, a textured
floor and wall on which geometry alone leaves one translation free."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_align_reference as A
import map_colour_reference as CR
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
F = np.float32
# The restated loop on the sliding scene (CR.sliding_scene(): 60 000 map points, 3 403 source points, uint8 colours; guess 10 cm along the
# free axis y, 2 and 3 cm in x and z, 2 and 1 mrad about x and z; defaults, max_dist = leaf), measured:
#   leaf   geometric H eigenvalues (lambda 1)   coloured H, largest / smallest   steps   distance from the truth (rad, m)
#   0.05   -5.9e-13 .. 4943                     133                              3       (3.18e-6, 6.41e-5)
#   0.10   -5.9e-13 .. 4943                     153                              3       (2.51e-6, 7.63e-5)
# (5 and 15 cm along y end on (3.13e-6, 5.56e-5), (3.05e-6, 5.89e-5) at leaf 0.05 and (2.82e-6, 7.01e-5), (4.71e-6, 2.86e-5) at 0.1.)
SLIDING_MEASURED = {0.05: (3.18e-6, 6.41e-5), 0.1: (2.51e-6, 7.63e-5)}


# ---- 1 the gradient of an analytic field ------------------------------------------------------------------------------------------------
def test_the_fitted_gradient_of_a_linear_field_on_a_tilted_plane():
    """A linear field I(x) = c + g . x on the plane spanned by p = (1, 0, 1) and q = (0, 1, 1), sampled at the 24 lattice points i p h +
    j q h (h = 2^-5, |i|, |j| <= 2) around the voxel.  c, g and the samples are dyadic, so every r and every intensity is exact in
    float32 and the data are exactly linear.  The one rounded input is the normal: n32 = float32(n), |n32 - n| <= sqrt(3) 2^-25 = D.
    r is exactly linear in (a, b) (r . D n = (a u + b v + c n32) . D n), so the exact least-squares fit is g's part tangent to n32 plus
    (g . n32) times a vector of length <= D (1 + D); that part differs from the true tangential gradient g - (g . n) n by at most
    2 |g| D (1 + D).  The float32 cast of d adds 2^-24 |d|, the float64 arithmetic of a well-conditioned 2 x 2 system (its scatter is that of
    a lattice: condition 3) a few 1e-16, bounded here by 1e-12.  Hence |d - g_t| <= |g| (3 sqrt(3) 2^-25 (1 + 1e-6) + 2^-24 + 1e-12),
    and |d . n32| <= |g| (2^-24 + 1e-12): d64 is tangent to n32 up to the arithmetic, the cast moves it by 2^-24 |d|."""
    h = 2.0 ** -5
    p, q = np.array([1.0, 0.0, 1.0]), np.array([0.0, 1.0, 1.0])
    n = np.cross(p, q)
    n = n / np.linalg.norm(n)
    n32 = n.astype(F)
    lattice = [(i, j) for i in range(-2, 3) for j in range(-2, 3) if (i, j) != (0, 0)]
    r = np.array([(i * p + j * q) * h for i, j in lattice])
    assert np.array_equal(r.astype(F).astype(np.float64), r)
    worst = worst_n = 0.0
    for g in ([0.5, -0.25, 0.125], [-1.0, 0.75, 0.5], [0.0, 0.0, 1.0], [1.0, 1.0, -1.0], [0.0625, 0.0, 0.0], [0.0, 0.0, 0.0]):
        g = np.array(g)
        c = 0.5
        inb = c + r @ g
        assert np.array_equal(inb.astype(F).astype(np.float64), inb)
        d, st, _, m = CR.fit(n32[None], np.array([c], F), r.astype(F)[None], inb.astype(F)[None], np.ones((1, len(r)), bool))
        assert st[0] == CR.OK and m[0] == 24
        gt = g - (g @ n) * n
        gn = np.linalg.norm(g)
        err, dn = np.linalg.norm(d[0].astype(np.float64) - gt), abs(d[0].astype(np.float64) @ n32.astype(np.float64))
        print("g", g, "d", d[0], "|d - g_t|", err, "|d . n|", dn, "bounds", gn * (3 * np.sqrt(3) * 2.0 ** -25 * (1 + 1e-6) + 2.0 ** -24 + 1e-12),
              gn * (2.0 ** -24 + 1e-12))
        assert err <= gn * (3 * np.sqrt(3) * 2.0 ** -25 * (1 + 1e-6) + 2.0 ** -24 + 1e-12)
        assert dn <= gn * (2.0 ** -24 + 1e-12)
        if gn:
            worst, worst_n = max(worst, err / gn), max(worst_n, dn / gn)
    print("largest |d - g_t| / |g|", worst, "largest |d . n| / |g|", worst_n)


def test_intensity_weights_and_range():
    """The gray weights sum to 2^14, so white is exactly 1 and a gray level v is v / 255 rounded once."""
    assert CR.intensity64([[255, 255, 255]], [1])[0] == 1.0 and CR.intensity64([[0, 0, 0]], [1])[0] == 0.0
    assert CR.intensity64([[255 * 7, 255 * 7, 255 * 7]], [7])[0] == 1.0
    v = np.arange(256)
    assert np.array_equal(CR.intensity64(np.stack([v, v, v], axis=1), np.ones(256, np.int64)), v / 255.0)
    assert CR.intensity64([[255, 0, 0]], [1])[0] == 4899.0 / 16384.0


# ---- 2 the library's host compile of the fit ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rgbd360_amd import build
    L = C.CDLL(build.build())
    L.rgbd360_map_colour_gradient.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    L.rgbd360_map_colour_intensity.argtypes = [C.c_longlong] * 4
    L.rgbd360_map_colour_intensity.restype = C.c_double
    return L


def neighbourhoods(seed=11, k=3000):
    """(n32 [k, 3], i32 [k], r [k, 26, 3] float32, i_nb [k, 26] float32, present [k, 26]): random unit normals and neighbourhoods of 0 ..
    26 members, then by blocks of the first rows: ties in |n_k| (two or three equal components, one or two zeros), collinear neighbours,
    equal intensities, fewer than four neighbours."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(k, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    ties = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0.6, np.sqrt(0.28)], [0.6, np.sqrt(0.28), 0.6], [np.sqrt(0.28), 0.6, 0.6],
                     [1, 1, 1] / np.sqrt(3.0), [-0.6, 0.6, np.sqrt(0.28)], [0, np.sqrt(0.5), np.sqrt(0.5)], [np.sqrt(0.5), 0, -np.sqrt(0.5)],
                     [-1, -1, 1] / np.sqrt(3.0), [0.8, -0.6, 0.0]])
    n[:len(ties) * 20] = np.repeat(ties, 20, axis=0)
    n32 = n.astype(F)
    r = rng.uniform(-0.1, 0.1, (k, 26, 3)).astype(F)
    i32 = rng.uniform(0, 1, k).astype(F)
    i_nb = rng.uniform(0, 1, (k, 26)).astype(F)
    m = rng.integers(0, 27, k)
    m[300:600] = rng.integers(0, 4, 300)                      # fewer than four
    present = np.arange(26)[None, :] < m[:, None]
    rng.permuted(present, axis=1, out=present)                # (the places of the absent ones vary)
    line = rng.normal(size=(300, 1, 3)) * rng.uniform(-1, 1, (300, 26, 1)) * 0.05
    r[600:900] = line.astype(F)                               # collinear
    i_nb[900:1100] = i32[900:1100, None]                      # equal intensities: a zero gradient with status OK
    return n32, i32, r, i_nb, present


@pytest.mark.parametrize("min_gradient_support, min_spread", [(4, 0.01), (1, 0.0), (8, 0.1)])
def test_the_library_fit_is_the_restatement_bit_for_bit(lib, min_gradient_support, min_spread):
    """rgbd360_map_colour_gradient is the host compile of the fit k_vmap_colour_layer runs: + - x / sqrt in float64 without contraction give
    numpy's bits."""
    n32, i32, r, i_nb, present = neighbourhoods()
    d, st, _, m = CR.fit(n32, i32, r, i_nb, present, min_gradient_support, min_spread)
    print("statuses OK / NO_GRADIENT", int((st == CR.OK).sum()), int((st == CR.NO_GRADIENT).sum()), "below the support", int((m < min_gradient_support).sum()),
          "refused on the determinant", int(((m >= min_gradient_support) & (st == CR.NO_GRADIENT)).sum()))
    assert (st[m < min_gradient_support] == CR.NO_GRADIENT).all()
    if min_spread > 0:
        enough = m[600:900] >= min_gradient_support
        assert (st[600:900][enough] == CR.NO_GRADIENT).all() and enough.sum() > 100          # the determinant's refusal
        assert (st[900:1100] == CR.OK).sum() > 50 and not d[900:1100].any()
    assert (st == CR.OK).sum() > 500 and (st == CR.NO_GRADIENT).sum() > 300
    for k in range(len(n32)):
        rk, ik = np.ascontiguousarray(r[k][present[k]]), np.ascontiguousarray(i_nb[k][present[k]])
        out = np.full(3, 7.0, F)
        rc = lib.rgbd360_map_colour_gradient(n32[k].ctypes.data, float(i32[k]), len(ik), rk.ctypes.data, ik.ctypes.data, min_gradient_support,
                                             min_spread, out.ctypes.data)
        assert rc == st[k], (k, rc, st[k])
        assert out.tobytes() == d[k].tobytes(), (k, out, d[k])
    out = np.full(3, 7.0, F)
    assert lib.rgbd360_map_colour_gradient(None, 0.5, 0, None, None, 4, 0.01, out.ctypes.data) == -1 and (out == 7.0).all()
    assert lib.rgbd360_map_colour_gradient(n32[0].ctypes.data, 0.5, 3, None, None, 4, 0.01, out.ctypes.data) == -1
    assert lib.rgbd360_map_colour_gradient(n32[0].ctypes.data, 0.5, 0, None, None, 4, 0.01, out.ctypes.data) == CR.NO_GRADIENT and not out.any()


def test_the_library_intensity_is_the_restatement_bit_for_bit(lib):
    rng = np.random.default_rng(3)
    count = rng.integers(1, 5000, 2000)
    sums = (rng.integers(0, 256, (2000, 3)) * count[:, None]) - rng.integers(0, 2, (2000, 3)) * (count[:, None] // 2)
    ref = CR.intensity64(sums, count)
    got = np.array([lib.rgbd360_map_colour_intensity(int(s[0]), int(s[1]), int(s[2]), int(c)) for s, c in zip(sums, count)])
    assert got.tobytes() == ref.tobytes() and (ref >= 0).all() and (ref <= 1).all()
    assert lib.rgbd360_map_colour_intensity(1, 1, 1, 0) == 0.0


# ---- 3 symbols, structs, defaults, the Python wrapper's refusals, the adapter ------------------------------------------------------------
def test_header_binding_and_adapter_agree(lib):
    from rgbd360_amd import _lib
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    for name in ("rgbd360_map_default_colour_params", "rgbd360_map_colours", "rgbd360_map_colours_dev", "rgbd360_map_colour_bytes",
                 "rgbd360_map_release_colours", "rgbd360_map_default_align_colour_params", "rgbd360_map_align_colour_sphere",
                 "rgbd360_map_align_colour_cloud"):
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(lib, name) and name in _lib.SYMBOLS, name
    for name in ("rgbd360_map_colour_gradient", "rgbd360_map_colour_intensity", "rgbd360_map_time_colours", "rgbd360_map_align_colour_eval",
                 "rgbd360_map_time_align_colour"):
        assert re.search(r"\b%s\s*\(" % name, diag) and name not in main and hasattr(lib, name) and name in _lib.SYMBOLS, name

    def fields(text, struct):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, text).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
        return names

    for struct, cls, size in (("rgbd360_map_colour_params", _lib.MapColourParams, 20), ("rgbd360_map_colour_stats", _lib.MapColourStats, 40),
                              ("rgbd360_map_align_colour_params", _lib.MapAlignColourParams, 48),
                              ("rgbd360_map_align_colour_result", _lib.MapAlignColourResult, 256)):
        assert fields(main, struct) == [n for n, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    # the existing structs keep their sizes, and the new ones begin with the point method's
    assert C.sizeof(_lib.MapAlignParams) == 24 and C.sizeof(_lib.MapAlignResult) == 224 and C.sizeof(_lib.MapAlignGicpResult) == 256
    assert fields(main, "rgbd360_map_align_colour_params")[:5] == fields(main, "rgbd360_map_align_params")
    assert fields(main, "rgbd360_map_align_colour_result")[:10] == fields(main, "rgbd360_map_align_result")
    assert fields(main, "rgbd360_map_align_colour_result")[10:] == ["n_no_normal", "n_no_gradient", "rms_geometric", "rms_colour"]
    for status, value in (("NONE", 0), ("OK", 1), ("NO_NORMAL", 2), ("NO_GRADIENT", 3)):
        assert re.search(r"RGBD360_COLOUR_%s = %d\b" % (status, value), main)
    lib.rgbd360_map_default_align_colour_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapAlignColourParams)]
    lib.rgbd360_map_default_align_colour_params.restype = None
    p = _lib.MapAlignColourParams()
    lib.rgbd360_map_default_align_colour_params(None, C.byref(p))
    plane = _lib.MapAlignPlaneParams()
    lib.rgbd360_map_default_align_plane_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapAlignPlaneParams)]
    lib.rgbd360_map_default_align_plane_params.restype = None
    lib.rgbd360_map_default_align_plane_params(None, C.byref(plane))
    for name in ("max_dist", "max_iters", "eps", "min_count", "min_matches", "min_support", "max_flatness"):      # the plane method's
        assert getattr(p, name) == getattr(plane, name), name
    assert p.lambda_geometric == F(0.968) and p.min_gradient_support == 4 and p.min_spread == F(0.01)
    assert (p.max_iters, p.min_count, p.min_matches, p.min_support) == (10, 1, 6, 5) and p.max_dist == F(0.05) and p.eps == F(1e-6)
    lib.rgbd360_map_default_colour_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapColourParams)]
    lib.rgbd360_map_default_colour_params.restype = None
    cp = _lib.MapColourParams()
    lib.rgbd360_map_default_colour_params(None, C.byref(cp))
    assert (cp.min_count, cp.min_support, cp.min_gradient_support) == (1, 5, 4) and cp.max_flatness == F(0.05) and cp.min_spread == F(0.01)
    assert {k: v for k, v in CR.DEFAULTS.items()} == dict(min_count=1, min_support=5, max_flatness=0.05, min_gradient_support=4, min_spread=0.01)
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("alignColourParams", "alignSphereColour", "alignCloudColour", "alignColourResult", "colours(", "colourStats", "colourBytes",
                 "releaseColours", "rgbd360_map_align_colour_sphere", "rgbd360_map_align_colour_cloud", "rgbd360_map_colours("):
        assert name in hpp, name
    py = open(os.path.join(ROOT, "rgbd360_amd", "voxel_map.py")).read()
    for name in ("def align_colour_params", "def align_cloud_colour", "def align_sphere_colour", "def colours", "def colour_params", "def colour_bytes",
                 "def release_colours"):
        assert name in py, name
    replay = open(os.path.join(ROOT, "examples", "odometry_replay.cpp")).read()
    assert "--refine-on-map-colour" in replay and "alignSphereColour" in replay


def test_the_python_wrapper_refuses_before_the_library_is_asked():
    """Missing colours, a lambda outside [0, 1] and supports outside their ranges raise in the wrapper: no map, no device is touched."""
    from rgbd360_amd.register import Rgbd360Error
    from rgbd360_amd.voxel_map import COLOUR_NO_GRADIENT, COLOUR_NO_NORMAL, COLOUR_NONE, COLOUR_OK, VoxelMap
    assert (COLOUR_NONE, COLOUR_OK, COLOUR_NO_NORMAL, COLOUR_NO_GRADIENT) == (CR.NONE, CR.OK, CR.NO_NORMAL, CR.NO_GRADIENT)
    m = VoxelMap.__new__(VoxelMap)          # no context behind it: whatever reaches the library raises AttributeError instead
    xyz, depth = np.zeros((4, 3), F), np.zeros((4, 8), np.uint16)
    with pytest.raises(Rgbd360Error):
        m.align_cloud_colour(xyz, None, EYE)
    with pytest.raises(Rgbd360Error):
        m.align_sphere_colour(None, depth, EYE)
    for bad in (dict(lambda_geometric=-0.01), dict(lambda_geometric=1.5), dict(lambda_geometric=float("nan")), dict(min_support=0), dict(min_support=28),
                dict(min_gradient_support=0), dict(min_gradient_support=27)):
        with pytest.raises(Rgbd360Error):
            m.align_colour_params(**bad)
        with pytest.raises(Rgbd360Error):
            m.align_cloud_colour(xyz, np.zeros((4, 3), np.uint8), EYE, **bad)
    with pytest.raises(Rgbd360Error):
        m.align_cloud_colour(xyz, np.zeros((3, 3), np.uint8), EYE)          # one colour per point


_SNIPPET = r'''
#include "rgbd360/GlobalMap.hpp"
int use(rgbd360::GlobalMap& g, const rgbd360::ImageView& rgb, const rgbd360::ImageView& depth, const rgbd360::Mat4f& guess, const float* xyz,
        const uint8_t* rgb3) {
    rgbd360::Mat4f pose;
    rgbd360_map_align_colour_params p = g.alignColourParams();
    p.lambda_geometric = 0.9f;
    p.min_gradient_support = 6;
    int rc = g.alignCloudColour(xyz, rgb3, 10, guess, pose, &p) + g.alignCloudColour(xyz, rgb3, 10, guess, pose);
    rc += g.alignSphereColour(rgb, depth, guess, pose, 2, &p) + g.alignSphereColour(rgb, depth, guess, pose);
    const rgbd360_map_align_colour_result& r = g.alignColourResult();
    std::vector<float> c, i, d;
    std::vector<int32_t> status, count, key3;
    rgbd360_map_colour_params cp = g.colourParams();
    cp.min_spread = 0.02f;
    const long long n = g.colours(c, i, d, &status, &count, &key3, &cp) + g.colours(c, i, d);
    const size_t bytes = g.colourBytes();
    g.releaseColours();
    return rc + (int)(r.n_no_normal + r.n_no_gradient + n + (long long)bytes + g.colourStats().n_gradients) + (r.rms_geometric >= r.rms_colour ? 1 : 0);
}
'''


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_headers"])
def test_adapter_compiles_against_the_header(tmp_path, mock):
    extra = ["-I" + os.path.join(ROOT, "tests", "mock_headers")] if mock else []
    src = tmp_path / "colour_snippet.cpp"
    src.write_text(_SNIPPET)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + extra + [str(src)])
    # and the header is C: the structs and the entries parse as C99
    c_src = tmp_path / "colour_c.c"
    c_src.write_text('#include "rgbd360_hip.h"\nint f(rgbd360_map* m, const float* x, const uint8_t* c, const float* g, float* o) { '
                     'rgbd360_map_align_colour_params p; rgbd360_map_align_colour_result r; rgbd360_map_colour_params cp; rgbd360_map_colour_stats st; '
                     'rgbd360_map_default_align_colour_params(m, &p); rgbd360_map_default_colour_params(m, &cp); p.lambda_geometric = 1.0f; '
                     'return rgbd360_map_align_colour_cloud(m, x, c, 3, g, 0, &p, o, &r) + (int)r.n_no_gradient + '
                     '(int)rgbd360_map_colours(m, &cp, 0, 0, 0, 0, 0, 0, 0, &st) + RGBD360_COLOUR_NO_GRADIENT; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(c_src)])


# ---- 4 the sliding scene ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return CR.sliding_scene()


@pytest.mark.parametrize("leaf", [0.05, 0.1])
def test_the_restated_loop_on_the_sliding_scene(scene, leaf):
    """A textured floor z = 0 and wall x = 0 from clouds with uint8 colours; the guess is 10 cm off along y, which geometry cannot see.
    Measured (this file's header): the geometric normal equations have eigenvalues -5.9e-13 .. 4943 -- the free direction is zero to
    rounding -- the coloured ones a condition of 133 (leaf 0.05) and 153 (leaf 0.1); the restated coloured loop converges in 3 steps and ends
    (3.18e-6 rad, 6.41e-5 m) from the truth at leaf 0.05 and (2.51e-6 rad, 7.63e-5 m) at leaf 0.1.  Asserted: twice those distances -- the
    margin covers the float32 cast of H and g in gn::step."""
    mx, mc, sx, sc = scene
    ref = R.Map([(mx, mc, EYE)], leaf, None)
    layers = CR.Layers(ref)
    guess = CR.sliding_guess(0.10)
    geo = CR.ColourEvaluation(ref, sx, sc, guess, leaf, None, leaf, lambda_geometric=1.0, layers=layers)
    ev = np.linalg.eigvalsh(CR.hessian64(geo.sums))
    col = CR.ColourEvaluation(ref, sx, sc, guess, leaf, None, leaf, layers=layers)
    evc = np.linalg.eigvalsh(CR.hessian64(col.sums))
    print("leaf", leaf, "voxels", len(ref), "geometric eigenvalues", ev[0], ev[-1], "coloured condition", evc[-1] / evc[0], "n", geo.n, geo.counters)
    assert geo.n > 3000 and ev[-1] > 0 and ev[0] * 1e12 <= ev[-1]          # largest / smallest >= 1e12 (the smallest may round below zero)
    assert evc[0] > 0 and evc[-1] / evc[0] < 1e3
    al = CR.ColourAlignment(ref, sx, sc, guess, leaf, None, leaf, layers=layers)
    rot, trans = A.pose_error(al.pose, EYE)
    print("guess", A.pose_error(guess, EYE), "ended", (rot, trans), "steps", al.iterations, "margins", al.margins, "rms", al.rms_geometric, al.rms_colour,
          al.final.counters)
    assert al.status == A.OK and al.converged == 1 and al.n_matched > 3000
    assert rot <= 2 * SLIDING_MEASURED[leaf][0] and trans <= 2 * SLIDING_MEASURED[leaf][1]
    # geometry alone refuses or slides: the restated loop with lambda 1 does not come home
    alone = CR.ColourAlignment(ref, sx, sc, guess, leaf, None, leaf, lambda_geometric=1.0, layers=layers)
    print("lambda 1: status", alone.status, "ended", A.pose_error(alone.pose, EYE))
    assert alone.status == A.ILL_POSED or A.pose_error(alone.pose, EYE)[1] > 0.05
