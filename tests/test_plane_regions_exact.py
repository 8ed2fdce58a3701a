"""The plane stage of Frame360 against the plain references of tests/plane_exact.py: labels pixel for pixel, roots,
counts and plane order, the nine region sums of rgbd360_debug_plane_sums bit for bit, centroids bit for bit, the eigen-descriptors to a
stated bound.  The layouts are the ones the kernels were written around: one component threading the whole image, joins only in the last
or first row, runs that cross the lane rows of the DPP scans, several runs per lane, more than 256 regions in one 8192-pixel block (the
moment hash's and the refinement commit's global fallbacks), rounding ties of the 2^-28 terms, link thresholds met exactly, the
4096-region limit and the range of the sums.

Descriptor bound (the host's sorted_eigen3 is not numpy's eigh; both are float64 solvers good to a few eps x the largest eigenvalue l2):
curvature within 2 float ulps + 1e-12; area_moment and elongation within 2 float ulps where the middle eigenvalue l1 >= 1e-6 l2; normal
and ppal_dir within 1e-6 (|cos| >= 1 - 1e-6) where their eigenvalue is separated from the next by more than 1e-3 l2."""
from __future__ import annotations

import numpy as np
import pytest

from tests import plane_exact as PE

ANG, DIST, MAXC = 0.05, 0.05, 0.9          # MAXC 0.9 > 1/3 >= every curvature: every region becomes a plane


# ---- layouts (masks of finite points; the points lie on z = 2 with normal (0, 0, -1): every finite neighbour pair links) ----------
def serpentine(rows, cols):
    m = np.zeros((rows, cols), bool)
    m[0::2, :] = True
    for k, r in enumerate(range(1, rows, 2)):          # joined alternately at the last and the first column
        m[r, cols - 1 if k % 2 == 0 else 0] = True
    return m


def comb(rows, cols, join_last_row):
    m = np.zeros((rows, cols), bool)
    m[:, 0::2] = True
    m[-1 if join_last_row else 0, :] = True
    return m


def spiral(rows, cols):
    m = np.zeros((rows, cols), bool)
    r0, r1, c0, c1 = 0, rows - 1, 0, cols - 1
    while r0 <= r1 and c0 <= c1:
        m[r0, c0:c1 + 1] = True
        m[r0:r1 + 1, c1] = True
        if r1 - r0 >= 2:
            m[r1, c0:c1 + 1] = True
        if c1 - c0 >= 2 and r1 - r0 >= 4:
            m[r0 + 2:r1 + 1, c0] = True
            m[r0 + 2, c0:c0 + 3] = True
        r0, r1, c0, c1 = r0 + 2, r1 - 2, c0 + 2, c1 - 2
    return m


def staircase(rows, cols):
    """Diagonal steps of width 3 that cross the 256 x 4 link tiles and the 64 x 64 merge tiles: every step joins its neighbour row
    through one column only."""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return ((c - 3 * r) % 7 < 4)


def percolation(rows, cols, seed, p=0.593):
    return np.random.default_rng(seed).random((rows, cols)) < p


def stripes(rows, cols, seed=0):
    """Runs 1-9 px wide with 1-px gaps along the even rows, each its own region (several regions per lane, runs across lanes 15/16,
    31/32, 47/48), whole invalid lanes (8 px) cutting runs, the odd rows invalid but for a link every ~100 columns."""
    rng = np.random.default_rng(seed)
    m = np.zeros((rows, cols), bool)
    for r in range(1, rows, 2):
        m[r, rng.integers(0, cols, max(1, cols // 100))] = True
    for r in range(0, rows, 2):
        c = int(rng.integers(0, 3))
        while c < cols:
            w = int(rng.integers(1, 10))
            m[r, c:c + w] = True
            c += w + 1
        if r % 4 == 2:                                   # a fully invalid lane (8 px) in the middle of the row
            s = 8 * int(rng.integers(0, max(1, cols // 8)))
            m[r, s:s + 8] = False
    return m


def fragments(rows, cols):
    """2-pixel regions with 1-px gaps on every other row: ~680 regions in each 8192 consecutive pixels of a 1024-column image."""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return (r % 2 == 0) & (c % 3 != 2)


def cloud(mask, seed=None):
    rows, cols = mask.shape
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    if seed is None:                                     # dyadic: x, y exact in 1/64 m
        xyz = np.stack([(c - cols // 2) / 64.0, (r - rows // 2) / 64.0, np.full(mask.shape, 2.0)], axis=2).astype(np.float32)
    else:                                                # random float32 mantissas, both signs
        rng = np.random.default_rng(seed)
        xyz = np.stack([rng.uniform(-3, 3, mask.shape), rng.uniform(-3, 3, mask.shape), rng.uniform(1.5, 2.5, mask.shape)],
                       axis=2).astype(np.float32)
    xyz[~mask] = np.nan
    nrm = np.zeros_like(xyz)
    nrm[..., 2] = -1
    return xyz, nrm


# ---- the checks ---------------------------------------------------------------------------------------------------------------
def _ulp(v):
    return float(np.spacing(np.float32(abs(v))))


def check_descriptors(p, d):
    assert np.array_equal(p["centroid"], d["centroid"].astype(np.float32)), (p["centroid"], d["centroid"])
    ev = d["ev"]
    l2 = ev[2]
    assert abs(p["curvature"] - d["curvature"]) <= 2 * _ulp(d["curvature"]) + 1e-12, (p["curvature"], d["curvature"])
    if l2 <= 0:
        return
    if ev[1] >= 1e-6 * l2:
        assert abs(p["area_moment"] - d["area_moment"]) <= 2 * _ulp(d["area_moment"]), (p["area_moment"], d["area_moment"])
        assert abs(p["elongation"] - d["elongation"]) <= 2 * _ulp(d["elongation"]), (p["elongation"], d["elongation"])
    if ev[2] - ev[1] > 1e-3 * l2:
        assert abs(float(np.dot(p["ppal_dir"], d["ppal_dir"]))) >= 1 - 1e-6
    if ev[1] - ev[0] > 1e-3 * l2:
        assert abs(float(np.dot(p["normal"], d["normal"]))) >= 1 - 1e-6


def check_sums(st, xyz, labels, min_inliers, roots=None):
    """The diag records against the exact sums over `labels`; returns (roots, counts, sums) in ascending root order."""
    if roots is None:
        roots, _ = PE.regions(labels, min_inliers)
    ds = st.plane_sums()
    order = np.argsort(ds["root"], kind="stable")
    assert np.array_equal(ds["root"][order], roots)
    sums, counts = PE.region_sums(xyz, labels, roots)
    assert np.array_equal(ds["count"][order], counts)
    bad = np.nonzero((ds["mom"][order] != sums).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} regions' sums differ, first root {roots[bad[0]]}: {ds['mom'][order][bad[0]]} vs {sums[bad[0]]}"
    return roots, counts, sums


def run_case(st, xyz, nrm, min_inliers=1, ang=ANG, dist=DIST, maxc=MAXC):
    rows, cols = xyz.shape[:2]
    labels, planes = st.plane_fit(xyz, nrm, rows, cols, min_inliers, ang, dist, maxc, 0, max_planes=4096)
    ref = PE.label_image(xyz, nrm, rows, cols, ang, dist, 0)
    diff = np.argwhere(labels != ref)
    assert diff.size == 0, f"{len(diff)} labels differ, first at {tuple(diff[0])}: {labels[tuple(diff[0])]} vs {ref[tuple(diff[0])]}"
    roots, counts, sums = check_sums(st, xyz, ref, min_inliers)
    assert [p["root"] for p in planes] == list(roots)
    assert [p["count"] for p in planes] == list(counts)
    for p, s, n in zip(planes, sums, counts):
        check_descriptors(p, PE.derived(s, n))
    return labels, planes


@pytest.fixture(scope="module")
def st(hip_lib):
    from rgbd360_amd.register import Frame360Stages, RegisterPhotoICP
    return Frame360Stages(RegisterPhotoICP())


# ---- the references themselves (no GPU) ---------------------------------------------------------------------------------------
def test_reference_components_on_hand_cases():
    m = np.array([[1, 1, 0, 1],
                  [0, 1, 0, 1],
                  [1, 1, 1, 1],
                  [0, 0, 0, 0],
                  [1, 0, 1, 1]], bool)
    xyz, nrm = cloud(m)
    lab = PE.label_image(xyz, nrm, *m.shape, ANG, DIST)
    want = np.array([[0, 0, -1, 0], [-1, 0, -1, 0], [0, 0, 0, 0], [-1] * 4, [16, -1, 18, 18]])
    assert np.array_equal(lab, want)
    # a serpentine: one component whose root is pixel 0, whatever the number of hooking rounds it takes
    s = serpentine(41, 37)
    lab = PE.label_image(*cloud(s), 41, 37, ANG, DIST)
    assert set(np.unique(lab[s])) == {0} and (lab[~s] == -1).all()


def test_reference_terms_round_half_to_even():
    x = np.array([[0.5, 0, 0], [1.5, 0, 0], [-0.5, 0, 0], [-2.5, 0, 0]], np.float64) / PE.SCALE
    assert list(PE.terms(x.astype(np.float32))[:, 0]) == [0.0, 2.0, -0.0, -2.0]
    a, b = 3 * 2.0 ** -15, 5 * 2.0 ** -14                # x y 2^28 = 7.5 -> 8, and 2 x 1.5... -> even neighbours
    t = PE.terms(np.array([[a, b, 0], [a / 3, b / 5 * 3, 0]], np.float32))
    assert t[0, 4] == 8.0 and t[1, 4] == 2.0             # 7.5 -> 8, 1.5 -> 2
    assert PE.libc_cosf(0.05) == np.float32(np.cos(np.float32(0.05)))  # (cosf of 0.05 is correctly rounded in every libm we know)


def test_reference_link_thresholds_are_strict():
    c = PE.libc_cosf(ANG)
    xyz = np.array([[[0, 0, 1], [0, 0, 1]]], np.float32)
    for nz, want in ((c, False), (np.nextafter(c, np.float32(2)), True)):
        nrm = np.array([[[0, 0, 1], [0, 0, nz]]], np.float32)
        _, left, _ = PE.link_flags(xyz, nrm, 1, 2, ANG, 0.5)
        assert bool(left[0, 1]) == want


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
WIDTHS = [3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1028, 4096]
ROWS = [2, 4, 5, 63, 65]
LAYOUTS = ["serpentine", "comb_last", "comb_first", "staircase", "stripes", "percolation"]


def _mask(layout, rows, cols, seed):
    return {"serpentine": lambda: serpentine(rows, cols), "comb_last": lambda: comb(rows, cols, True),
            "comb_first": lambda: comb(rows, cols, False), "staircase": lambda: staircase(rows, cols),
            "stripes": lambda: stripes(rows, cols, seed), "percolation": lambda: percolation(rows, cols, seed)}[layout]()


@pytest.mark.gpu
@pytest.mark.parametrize("cols", WIDTHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts_exact(st, layout, cols):
    k = WIDTHS.index(cols) + LAYOUTS.index(layout)
    rows = ROWS[k % len(ROWS)] if cols < 4096 else 5
    rnd = layout in ("stripes", "percolation")          # random coordinates: z in [1.5, 2.5], a threshold that links every pair
    xyz, nrm = cloud(_mask(layout, rows, cols, seed=k), seed=k if rnd else None)
    dist = 1.0 if rnd else DIST
    lab = PE.label_image(xyz, nrm, rows, cols, ANG, dist)
    min_inliers = next(m for m in (1, 2, 4, 8, 16, 32) if len(PE.regions(lab, m)[0]) <= 4096)       # inside the slot limit
    run_case(st, xyz, nrm, min_inliers=min_inliers, dist=dist)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(63, 64), (65, 257), (130, 1024), (200, 300)])
def test_spiral_exact(st, rows, cols):
    labels, planes = run_case(st, *cloud(spiral(rows, cols)))
    assert len(planes) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_percolation_seeds_exact(st, seed):
    run_case(st, *cloud(percolation(192, 1024, 100 + seed), seed=seed), dist=1.0)


@pytest.mark.gpu
def test_whole_frame_4096x2048(st):
    m = np.ones((2048, 4096), bool)
    labels, planes = run_case(st, *cloud(m), min_inliers=40)
    assert len(planes) == 1 and planes[0]["count"] == m.size
    run_case(st, *cloud(percolation(2048, 4096, 7), seed=7), min_inliers=60, dist=1.0)      # 3684 regions


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(16, 1024), (20, 1025), (4, 4096)])
def test_moment_hash_overflow(st, rows, cols):
    """Well over 256 regions in one block's 8192 consecutive pixels: k_f360_moments sends most runs to the global table directly."""
    m = fragments(rows, cols)
    xyz, nrm = cloud(m, seed=rows)
    _, planes = run_case(st, xyz, nrm, min_inliers=1, dist=1.0)
    per_block = np.bincount(np.array([p["root"] for p in planes]) // 8192)
    assert per_block.max() > 256


@pytest.mark.gpu
def test_rounding_ties_of_the_terms(st):
    """x 2^28 = k + 1/2 and x y 2^28 = k + 1/2 for both parities of k, among random float32 coordinates of both signs."""
    rows, cols = 16, 128
    xyz, nrm = cloud(np.ones((rows, cols), bool), seed=5)
    rng = np.random.default_rng(6)
    k = rng.integers(-2000, 2000, (rows, cols // 2))
    xyz[:, 0::2, 0] = ((k + 0.5) / PE.SCALE).astype(np.float32)                  # linear ties
    a = 2 * rng.integers(-40, 40, (rows, cols // 2)) + 1
    b = 2 * rng.integers(-40, 40, (rows, cols // 2)) + 1
    xyz[:, 1::2, 0] = (a * 2.0 ** -15).astype(np.float32)                         # x y 2^28 = a b / 2: odd halves
    xyz[:, 1::2, 1] = (b * 2.0 ** -14).astype(np.float32)
    lin = xyz[:, 0::2, 0].astype(np.float64).reshape(-1) * PE.SCALE
    quad = (xyz[:, 1::2, 0].astype(np.float64) * xyz[:, 1::2, 1]).reshape(-1) * PE.SCALE
    for v in (lin, quad):                               # exact ties, below both even and odd integers
        assert (v - np.floor(v) == 0.5).all() and len(set(np.floor(v).astype(np.int64) % 2)) == 2
    run_case(st, xyz, nrm, min_inliers=40, dist=1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("direction", ["left", "up"])
def test_link_thresholds_met_exactly(st, direction):
    """dot == cosf(angular_threshold) and |w - w'| == dist_thr z^2 do not link (strict compares); one float ulp inside, they do."""
    c = PE.libc_cosf(ANG)
    cases = []
    # angle: normals (0, 0, 1) and (0, 0, nz), points (0, 0, 1): dot = nz exactly, |w - w'| = 1 - nz < 0.5
    for nz, want in ((c, False), (np.nextafter(c, np.float32(2)), True)):
        cases.append((np.array([[0, 0, 1], [0, 0, 1]], np.float32), np.array([[0, 0, 1], [0, 0, nz]], np.float32), 0.5, want))
    # distance: normals (0, 0, 1), w = z; the pixel itself (second) at z = 1: threshold 0.0625 exactly
    for z0, want in ((np.float32(1.0625), False), (np.nextafter(np.float32(1.0625), np.float32(0)), True)):
        cases.append((np.array([[0, 0, z0], [0, 0, 1]], np.float32), np.array([[0, 0, 1], [0, 0, 1]], np.float32), 0.0625, want))
    for pts, nrms, dist, want in cases:
        xyz = np.full((3, 3, 3), np.nan, np.float32)
        nrm = np.zeros((3, 3, 3), np.float32)
        nrm[..., 2] = 1
        at = [(1, 0), (1, 1)] if direction == "left" else [(0, 1), (1, 1)]
        for (r, cc), p, q in zip(at, pts, nrms):
            xyz[r, cc], nrm[r, cc] = p, q
        labels, _ = run_case(st, xyz, nrm, min_inliers=0, dist=dist)
        assert (labels[at[1]] == labels[at[0]]) == want, (direction, dist, want)


@pytest.mark.gpu
def test_slot_limit(st):
    """Exactly 4096 regions above min_inliers are served; one more is error -7, not a cut list."""
    from rgbd360_amd.register import Rgbd360Error
    rows, cols = 128, 192
    m = (np.arange(rows)[:, None] % 2 == 0) & (np.arange(cols)[None, :] % 3 != 2)
    _, planes = run_case(st, *cloud(m), min_inliers=1)
    assert len(planes) == 4096
    m2 = np.zeros((rows + 1, cols), bool)
    m2[:rows] = m
    m2[rows, :2] = True
    xyz, nrm = cloud(m2)
    with pytest.raises(Rgbd360Error, match=r"\(-7\)"):
        st.plane_fit(xyz, nrm, rows + 1, cols, 1, ANG, DIST, MAXC, 0, max_planes=4096)


# ---- refinement -------------------------------------------------------------------------------------------------------------
def _refine_case(st, xyz, nrm, min_inliers):
    rows, cols = xyz.shape[:2]
    seg = PE.label_image(xyz, nrm, rows, cols, ANG, DIST, 0)
    st.set_refinement(True, 0.02)
    try:
        labels, planes = st.plane_fit(xyz, nrm, rows, cols, min_inliers, ANG, DIST, MAXC, 0, max_planes=4096)
        stats = st.refinement_stats()
    finally:
        st.set_refinement(False)
    roots, _ = PE.regions(seg, min_inliers)
    assert [p["root"] for p in planes] == list(roots)
    # planes only grow into pixels of regions that did not become planes
    moved = labels.reshape(-1) != seg.reshape(-1)
    assert np.isin(labels.reshape(-1)[moved], roots).all() and not np.isin(seg.reshape(-1)[moved], roots).any()
    assert stats["pixels_relabelled"] == int(moved.sum()) > 0
    _, counts, sums = check_sums(st, xyz, labels, min_inliers, roots=roots)
    assert [p["count"] for p in planes] == list(counts)
    for p, s, n in zip(planes, sums, counts):
        d = PE.derived(s, n)
        l2 = d["ev"][2]
        if d["ev"][1] >= 1e-6 * l2:
            assert abs(p["area_moment"] - d["area_moment"]) <= 2 * _ulp(d["area_moment"])
            assert abs(p["elongation"] - d["elongation"]) <= 2 * _ulp(d["elongation"])
    return labels, planes, moved


def _isolated_normals(nrm, sel):
    """Normals that link to nothing: (1, 0, 0) and (0, 1, 0) in a checkerboard, orthogonal to the planes' and to each other."""
    r, c = np.nonzero(sel)
    nrm[r, c] = 0
    nrm[r, c, np.where((r + c) % 2 == 0, 0, 1)] = 1


@pytest.mark.gpu
def test_refinement_one_plane_waves(st):
    """A whole noisy row across a wall: every 64-pixel wave of grown pixels joins one plane (the commit's wave-sum path)."""
    rows, cols = 48, 512
    xyz, nrm = cloud(np.ones((rows, cols), bool))
    noisy = np.zeros((rows, cols), bool)
    noisy[20, :] = True
    noisy[30:34, 100:103] = True
    _isolated_normals(nrm, noisy)
    _, _, moved = _refine_case(st, xyz, nrm, 40)
    assert moved.reshape(rows, cols)[20].all()


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [1024, 1028])
def test_refinement_hash_overflow(st, cols):
    """Stripes 2 px wide, one isolated pixel between them: ~340 planes grow inside every 8192-pixel block of the commit."""
    rows = 64
    xyz, nrm = cloud(np.ones((rows, cols), bool))
    sep = np.zeros((rows, cols), bool)
    sep[:, 2::3] = True
    _isolated_normals(nrm, sep)
    _, planes, moved = _refine_case(st, xyz, nrm, 40)
    assert len(planes) > 300 and moved.sum() == sep.sum()


# ---- whole chains -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_frame_planes_float_depth_sums(st, oracle_mod):
    """rgbd360_frame_planes with float depth (the k_f360_slot_frames route end to end): exact sums over the device's own cloud and
    labels; labels equal the oracle's on the device's normals (a cross-check of the oracle on this stage)."""
    from rgbd360_amd import synth
    W, H = 512, 256
    depth = synth.make_pair(W, H, seed=77, depth_f32=True)[0][1]
    out = st.frame_planes(depth, convention=2, min_inliers=40)
    roots, counts, sums = check_sums(st, out["xyz"], out["labels"], 40)
    by_root = {int(r): (s, n) for r, s, n in zip(roots, sums, counts)}
    assert out["planes"]
    for p in out["planes"]:
        s, n = by_root[p["root"]]
        assert p["count"] == n
        check_descriptors(p, PE.derived(s, n))
    labels_ref, _ = oracle_mod.f360_plane_segment(out["xyz"], out["normals"], H, W, 40, 0.05, 0.05, 0.001, 1)
    assert np.array_equal(np.asarray(labels_ref).reshape(-1), out["labels"].reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["serpentine", "stripes"])
def test_oracle_agrees_on_exact_layouts(st, oracle_mod, layout):
    rows, cols = 65, 257
    xyz, nrm = cloud(_mask(layout, rows, cols, 3))
    labels, _ = run_case(st, xyz, nrm, min_inliers=1)
    lab_o, _ = oracle_mod.f360_plane_segment(xyz, nrm, rows, cols, 1, ANG, DIST, MAXC, 0)
    assert np.array_equal(np.asarray(lab_o).reshape(rows, cols), labels)


# ---- range of the sums --------------------------------------------------------------------------------------------------------
def _range_call(st, xyz, nrm, min_inliers=40):
    """Either -8, or planes whose sums are the exact (unbounded) integer sums -- never a plane built from wrapped or misrounded sums."""
    from rgbd360_amd.register import Rgbd360Error
    rows, cols = xyz.shape[:2]
    try:
        labels, planes = st.plane_fit(xyz, nrm, rows, cols, min_inliers, ANG, DIST, MAXC, 0, max_planes=4096)
    except Rgbd360Error as e:
        assert "(-8)" in str(e), e
        return None
    ds = st.plane_sums()
    for root, mom in zip(ds["root"], ds["mom"]):
        exact, _ = PE.region_sums_exact(xyz, labels, root)
        assert [int(v) for v in mom] == exact, (root, [int(v) for v in mom], exact)
    return planes


@pytest.mark.gpu
def test_range_sum_of_squares_past_2_64_is_refused(st):
    """A region symmetric in x with sum x^2 2^28 in [2^64, 2^64 + 2^63): a wrapped sum that looks positive and plausible."""
    rows, cols = 128, 256
    xyz, nrm = cloud(np.ones((rows, cols), bool))
    xyz[..., 0] = np.where(np.arange(cols) % 2 == 0, 1620.0, -1620.0)[None, :]
    xyz[..., 2] = 1.0
    s = rows * cols * 1620.0 ** 2 * PE.SCALE
    assert 2.0 ** 64 <= s < 2.0 ** 64 + 2.0 ** 63
    assert _range_call(st, xyz, nrm) is None


@pytest.mark.gpu
def test_range_far_small_region_is_refused(st):
    """64 points 3-4 km away: a squared coordinate beyond 2^51 units does not round exactly (no wrap at all)."""
    rng = np.random.default_rng(11)
    xyz, nrm = cloud(np.ones((8, 8), bool))
    xyz[..., 2] = np.float32(3517.3)                   # one plane z = const: every pair links
    xyz[..., 0] = rng.uniform(-1, 1, (8, 8)).astype(np.float32)
    xyz[..., 1] = rng.uniform(-1, 1, (8, 8)).astype(np.float32)
    assert _range_call(st, xyz, nrm, min_inliers=40) is None


@pytest.mark.gpu
def test_range_just_inside_is_exact(st):
    """Inside the bound the planes come back, with the exact sums: 64 points at 2800-2890 m, and 32768 points at 1000 m
    (N m^2 = 3.28e10 m^2, sum z^2 2^28 = 8.8e18 < 2^63)."""
    rng = np.random.default_rng(12)
    xyz, nrm = cloud(np.ones((8, 8), bool))
    xyz[..., 2] = np.float32(rng.uniform(2800.0, 2890.0))
    xyz[..., 0] = rng.uniform(-1, 1, (8, 8)).astype(np.float32)
    xyz[..., 1] = rng.uniform(-1, 1, (8, 8)).astype(np.float32)
    planes = _range_call(st, xyz, nrm)
    assert planes is not None and len(planes) == 1
    xyz, nrm = cloud(np.ones((128, 256), bool))
    xyz[..., 2] = 1000.0
    planes = _range_call(st, xyz, nrm)
    assert planes is not None and len(planes) == 1 and planes[0]["count"] == 32768
