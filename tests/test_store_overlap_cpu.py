"""Sensed-space overlap of stored frames without a GPU: the reference builder (tests/store_overlap_reference.py) on a hand-made case,
the non-vacuity of the inputs the GPU tests use (measured with the CPU oracle), the host-side candidate selection
(rgbd360_overlap_candidates / rgbd360_overlap_representative), the relative-pose formula of rgbd360_store_overlap_all and the C++
surface (compile + link)."""
import os
import subprocess

import numpy as np
import pytest

from rgbd360_amd import store as S
from rgbd360_amd import synth
from tests import store_overlap_reference as R
from tests import warp_images_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN = F(np.nan)


def test_hand_made_case_every_class_invalid_invisible_and_nan_target():
    """Six source points onto a 2 x 3 target at the identity pose, tolerances 0.05 + 0.02 D.
      0  range 2.0 on D = 2.0              consistent
      1  range 3.0 on D = 2.0 (tol 0.09)   behind
      2  invalid point (x = -10000), which a warp never reports as visible
      3  range 1.0 on D = 4.0 (tol 0.13)   in front
      4  valid, not visible
      5  range 3.0 on D = NaN              visible, no target
    and one more consistent point exactly ON the boundary would be borderline: point 0 moved to range 2.09 on D = 2.0."""
    idx = np.array([[0, 0], [0, 0], [-1, -1], [1, 2], [-1, -1], [0, 1]], np.int32)
    lut = np.array([[2, 0, 0], [0, 3, 0], [-10000, 0, 0], [0, 0, 1], [5, 5, 5], [1, 2, 2]], F)
    depth_trg = np.array([[2.0, NAN, 7.0], [7.0, np.inf, 4.0]], F)
    got = R.counts(idx, lut, depth_trg, np.eye(4))
    assert {k: got[k] for k in R.FIELDS} == dict(n_valid=5, n_visible=4, n_target=3, n_consistent=1, n_behind=1, n_in_front=1)
    assert got["n_borderline"] == 0 and got["sure"] == dict(n_consistent=1, n_behind=1, n_in_front=1)
    R.check(dict(got), got, exact=True)
    R.check(dict(got), got, exact=False)
    # a target at +Inf is no target either; a translation moves the ranges: (2,0,0) + (0.5,0,0) has range 2.5 on D = 2: behind
    T = np.eye(4)
    T[0, 3] = 0.5
    got = R.counts(idx[:1], lut[:1], depth_trg, T)
    assert (got["n_consistent"], got["n_behind"], got["n_in_front"]) == (0, 1, 0)
    got = R.counts(np.array([[1, 1]], np.int32), lut[:1], depth_trg, np.eye(4))
    assert (got["n_visible"], got["n_target"]) == (1, 0)
    # on the boundary: | |diff| - tol | is a rounding error of the sum -> borderline, and the bracket of arithmetic 0 lets it fall on either side
    lut_b = np.array([[F(2.0) + (F(0.05) + F(0.02) * F(2.0)), 0, 0]], F)
    got = R.counts(idx[:1], lut_b, depth_trg, np.eye(4))
    assert got["n_borderline"] == 1 and got["n_target"] == 1
    for moved in (dict(n_consistent=1, n_behind=0), dict(n_consistent=0, n_behind=1)):
        R.check(dict(n_valid=1, n_visible=1, n_target=1, n_in_front=0, **moved), got, exact=False)
    with pytest.raises(AssertionError):
        R.check(dict(n_valid=1, n_visible=1, n_target=1, n_consistent=0, n_behind=0, n_in_front=1), got, exact=True)


@pytest.fixture(scope="module")
def frames6():
    return [synth.render(synth.trajectory_pose(k, 7), 256, 128, 7) for k in range(6)]


def _rel(t, s):
    return np.linalg.inv(synth.trajectory_pose(t, 7)) @ synth.trajectory_pose(s, 7)


@pytest.mark.parametrize("math_mode", [0, 1])
def test_gpu_test_inputs_are_not_vacuous(oracle_mod, frames6, math_mode):
    """What the GPU tests rely on, measured with the oracle (both math modes gave the same figures) on the 256 x 128 trajectory frames,
    pair (0, 3):
      true relative pose, level 2: 2 043 of 2 048 visible; 1 760 consistent, 161 behind, 122 in front
      pushed pose, level 2: 33 / 1 087 / 924;  level 0: 371 / 17 445 / 14 922
    Each at least half of that (and n_visible < n), so a later change of synth cannot hollow the GPU tests out.  The cap on the
    borderline points (1 % of the level) holds for every pair and pose of the GPU tests: the worst measured was 2 of 2 048."""
    O = oracle_mod
    ora = O.Oracle(n_pyr=3, math_mode=math_mode, reduce_mode=1)
    ora.set_target(*frames6[0])
    ora.set_source(*frames6[3])
    T = _rel(0, 3)
    c = R.from_context(ora, 2, T)
    print("true, level 2:", c)
    assert c["n_valid"] == 2048 and c["n_visible"] < 2048 and 2 * c["n_visible"] >= 2043
    assert 2 * c["n_consistent"] >= 1760 and 2 * c["n_behind"] >= 161 and 2 * c["n_in_front"] >= 122
    assert c["n_borderline"] * 100 <= 2048
    for level, quoted in ((2, (33, 1087, 924)), (0, (371, 17445, 14922))):
        c = R.from_context(ora, level, W.pushed(T))
        print("pushed, level", level, c)
        for k, v in zip(("n_consistent", "n_behind", "n_in_front"), quoted):
            assert 2 * c[k] >= v, (level, k, c[k], v)
        assert c["n_consistent"] + c["n_behind"] + c["n_in_front"] == c["n_target"]
        assert c["n_borderline"] * 100 <= (2048 if level == 2 else 32768)
    ora.close()


def test_borderline_cap_for_every_gpu_pair(oracle_mod, frames6):
    """The condition of the bracket check: at most 1 % of the level's pixels are borderline, for every pair, pose and level the GPU
    tests use."""
    O = oracle_mod
    from tests.test_store_overlap_gpu import LIST_PAIRS, pose_of
    for t, s in sorted(set(LIST_PAIRS)):
        ora = O.Oracle(n_pyr=3, math_mode=1, reduce_mode=1)
        ora.set_target(*frames6[t])
        ora.set_source(*frames6[s])
        for kind in ("true", "pushed", "identity"):
            for level in (0, 2):
                c = R.from_context(ora, level, pose_of(kind, t, s))
                assert c["n_borderline"] * 100 <= (32768 >> (2 * level)), (t, s, kind, level, c)
        ora.close()


def test_spoiled_depth_inputs_are_not_vacuous(oracle_mod):
    """The pair of synth.make_pair(256, 128, seed=1234, depth_f32=True) with synth.spoil_depth in both frames (NaN, +-Inf, negative,
    beyond maxDepth, zeros), level 0, true pose: 31 547 of 32 768 points valid, 31 473 visible, 30 970 of them on a finite target depth
    (503 are not).  At least half of each shortfall."""
    O = oracle_mod
    (rgbA, dA), (rgbB, dB), T = synth.make_pair(256, 128, seed=1234, depth_f32=True)
    ora = O.Oracle(n_pyr=3, math_mode=0, reduce_mode=1)
    ora.set_target(rgbA, synth.spoil_depth(dA, 4))
    ora.set_source(rgbB, synth.spoil_depth(dB, 3))
    c = R.from_context(ora, 0, T)
    print("spoiled, level 0:", c)
    assert 2 * (32768 - c["n_valid"]) >= 32768 - 31547
    assert 2 * (c["n_visible"] - c["n_target"]) >= 31473 - 30970
    assert c["n_valid"] > 16384 and c["n_target"] > 16384
    ora.close()


def _matrix(n, consistent, evaluated=None):
    m = np.zeros((n, n), S.OVERLAP_DTYPE)
    m["n_consistent"] = consistent
    m["evaluated"] = 1 - np.eye(n, dtype=np.int32) if evaluated is None else evaluated
    return m


def test_overlap_candidates_and_representative():
    n, px = 6, 100
    c = np.zeros((n, n), np.int32)

    def put(a, b, ab, ba):
        c[a, b], c[b, a] = ab, ba

    put(0, 5, 80, 60)      # score 0.6
    put(1, 5, 70, 90)      # 0.7
    put(2, 5, 60, 60)      # 0.6: ties with (0, 5), the smaller a first
    put(3, 5, 95, 99)      # 0.95, but b - a = 2 < min_gap 3
    put(0, 4, 50, 55)      # 0.5
    put(1, 4, 90, 90)      # 0.9, a known edge, given as (4, 1)
    put(0, 3, 20, 99)      # 0.2 < min_score
    m = _matrix(n, c)
    sc = S.overlap_score(m, px)
    assert sc.dtype == np.float32 and np.array_equal(sc, sc.T) and sc[0, 5] == F(0.6) and sc[5, 1] == F(0.7) and sc[2, 2] == 0
    a, b, s, found = S.overlap_candidates(m, px, min_score=0.4, min_gap=3, max_per_frame=0, known=[(4, 1)])
    assert found == 4
    assert list(zip(a.tolist(), b.tolist())) == [(0, 4), (1, 5), (0, 5), (2, 5)]           # b ascending; score descending, tie -> smaller a
    assert s.tolist() == [F(0.5), F(0.7), F(0.6), F(0.6)]
    # the known edge in the other orientation, and none known
    assert S.overlap_candidates(m, px, 0.4, 3, 0, known=[(1, 4)])[3] == 4
    a, b, s, found = S.overlap_candidates(m, px, 0.4, 3, 0)
    assert found == 5 and list(zip(a.tolist(), b.tolist()))[:2] == [(1, 4), (0, 4)]
    # max_per_frame keeps the best of every b; max_out truncates what is written, not what is counted
    a, b, s, found = S.overlap_candidates(m, px, 0.4, 3, 2, known=[(4, 1)])
    assert found == 3 and list(zip(a.tolist(), b.tolist())) == [(0, 4), (1, 5), (0, 5)]
    a, b, s, found = S.overlap_candidates(m, px, 0.4, 3, 0, known=[(4, 1)], max_out=2)
    assert found == 4 and list(zip(a.tolist(), b.tolist())) == [(0, 4), (1, 5)]
    # min_gap 1 lets (3, 5) in, at the front of b = 5
    a, b, s, found = S.overlap_candidates(m, px, 0.4, 1, 1, known=[(4, 1)])
    assert list(zip(a.tolist(), b.tolist())) == [(0, 4), (3, 5)]
    # one direction not evaluated: score 0, never a candidate (min_score 0 would take it otherwise)
    ev = 1 - np.eye(n, dtype=np.int32)
    ev[5, 1] = 0
    m1 = _matrix(n, c, ev)
    assert S.overlap_score(m1, px)[1, 5] == 0 and S.overlap_score(m1, px)[5, 1] == 0
    pairs = list(zip(*[x.tolist() for x in S.overlap_candidates(m1, px, 0.4, 3, 0, known=[(4, 1)])[:2]]))
    assert (1, 5) not in pairs and len(pairs) == 3
    # representative: row sums of the score over the subset; ties to the first named
    assert S.overlap_representative(m, px, [0, 1, 2, 5]) == 5          # 0.6 + 0.7 + 0.6
    assert S.overlap_representative(m, px, [0, 4, 1]) == 4             # 4: 0.5 + 0.9
    assert S.overlap_representative(m, px, [2, 0, 5]) == 5
    assert S.overlap_representative(m, px, [2, 3]) == 2                # all zero: the first
    assert S.overlap_representative(m, px, [3, 2]) == 3
    assert S.overlap_representative(m, px, [0, 2, 3]) == 0             # 0: 0.2 (with 3), 3: 0.2 -> tie, the first named
    assert S.overlap_representative(m, px, [3, 2, 0]) == 3
    with pytest.raises(S.Rgbd360Error):
        S.overlap_representative(m, px, [0, 9])
    with pytest.raises(S.Rgbd360Error):
        S.overlap_candidates(m, 0, 0.4)


def test_relative_pose_formula_restated():
    """T_ab = W_a^-1 W_b of the all-pairs entry, restated (store_overlap_reference.rel_pose): within float32 rounding of numpy's float64
    inverse and product, the last row exact, the identity for a == b, and the distance the float64 translation norm."""
    for a, b in ((0, 3), (3, 0), (1, 5), (2, 2)):
        Wa, Wb = synth.trajectory_pose(a, 7).astype(F), synth.trajectory_pose(b, 7).astype(F)
        T, dist = R.rel_pose(Wa, Wb)
        want = np.linalg.inv(Wa.astype(np.float64)) @ Wb.astype(np.float64)
        assert T.dtype == np.float32 and np.array_equal(T[3], [0, 0, 0, 1])
        assert np.abs(T.astype(np.float64) - want).max() < 1e-6      # the float32 inputs are rotations only to 1e-7
        assert abs(dist - np.linalg.norm(want[:3, 3])) < 1e-6
        if a == b:
            assert np.abs(T - np.eye(4, dtype=F)).max() < 3e-7 and dist < 1e-6
    # an exactly representable case: a quarter turn about z and integer translations
    Wa = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], F)
    Wb = np.array([[1, 0, 0, 4], [0, 1, 0, 6], [0, 0, 1, 3], [0, 0, 0, 1]], F)
    T, dist = R.rel_pose(Wa, Wb)
    assert np.array_equal(T, np.array([[0, 1, 0, 4], [-1, 0, 0, -3], [0, 0, 1, 0], [0, 0, 0, 1]], F)) and dist == 5.0


_SNIPPET = r'''
#include <cstdio>
#include <rgbd360/FrameStore.hpp>
int main(int argc, char**) {
    // host side: runs without a device
    std::vector<rgbd360_overlap> m(4);
    for (auto& r : m) { r = rgbd360_overlap(); r.evaluated = 1; }
    m[0].evaluated = m[3].evaluated = 0;
    m[1].n_consistent = 60; m[2].n_consistent = 80;
    const std::vector<rgbd360::OverlapCandidate> c = rgbd360::overlapCandidates(m, 2, 100, 0.5f, 1, 0, {});
    if (c.size() != 1 || c[0].a != 0 || c[0].b != 1 || c[0].score != 0.6f) return 5;
    if (rgbd360::overlapScore(m, 2, 100, 1, 0) != 0.6f) return 6;
    if (rgbd360::overlapRepresentative(m, 2, 100, {1, 0}) != 1) return 7;
    if (!rgbd360::overlapCandidates(m, 2, 100, 0.5f, 1, 0, {{1, 0}}).empty()) return 8;
    if (argc < 2) return 3;                       // (the rest is never run without a GPU: a compile + link check)
    rgbd360::RegisterPhotoICP align360;
    rgbd360::FrameStore store(align360, 4, 128, 256);
    rgbd360_overlap_params p = store.overlapDefaultParams();
    const std::vector<rgbd360_overlap> r = store.overlap({{0, 1}, {1, 0}}, {}, p);
    std::vector<rgbd360::Mat4f> world(2, rgbd360::Mat4f::Identity());
    const rgbd360::OverlapMatrix M = store.overlapMatrix({0, 1}, world, 0.f, p);
    printf("%d %zu %zu %d\n", r[0].n_consistent, M.records.size(), M.rel_poses.size(), M.at(0, 1).evaluated);
    return 0;
}
'''


def test_cpp_surface_compiles_links_and_selects_candidates(tmp_path):
    """FrameStore::overlap / overlapMatrix / overlapDefaultParams and the free functions overlapScore / overlapCandidates /
    overlapRepresentative against the C ABI; the host-side part runs here."""
    from rgbd360_amd import build
    lib = build.build()
    src = tmp_path / "store_overlap_snippet.cpp"
    src.write_text(_SNIPPET)
    exe = str(tmp_path / "store_overlap_snippet")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror=return-type", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + os.path.dirname(lib), "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    assert subprocess.call([exe]) == 3


def test_host_functions_under_sanitizers(tmp_path):
    """tools/overlap_host_check.cpp: rgbd360_overlap_candidates / _representative as a program of its own under AddressSanitizer and
    UBSan (argument checks, truncated and NULL outputs, the filters and tie rules on seeded random matrices against a restatement)."""
    import shutil
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tools/overlap_host_check.cpp"
    exe = str(tmp_path / "overlap_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "overlap_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_overlap_kernels_are_in_the_gfx950_code_object_and_bound():
    """Both kernels are device code of the library, for gfx950; the ABI is declared in the public headers, exported and bound."""
    import ctypes as C
    import re
    from rgbd360_amd import _lib, build
    lib = build.build()
    strings = subprocess.run(["strings", "-n", "8", lib], capture_output=True, text=True, check=True).stdout
    for name in ("k_store_overlapILi0E", "k_store_overlapILi2E", "k_store_overlap_allILi0E", "k_store_overlap_allILi2E"):
        assert name in strings, name
    assert "gfx950" in strings
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_overlap.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbd360_[a-z0-9_]+)\s*\(", txt)))
    assert declared == ["rgbd360_overlap_candidates", "rgbd360_overlap_representative", "rgbd360_store_overlap", "rgbd360_store_overlap_all",
                        "rgbd360_store_overlap_default_params"]
    assert '#include "rgbd360_overlap.h"' in open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read()
    L = C.CDLL(lib)
    for s in declared:
        assert hasattr(L, s) and s in _lib.SYMBOLS, s
    B = _lib.load()
    assert len(B.rgbd360_store_overlap.argtypes) == 7 and len(B.rgbd360_store_overlap_all.argtypes) == 8
    assert C.sizeof(_lib.OverlapParams) == 12 and S.OVERLAP_DTYPE.itemsize == 32
    # without a store nothing runs and nothing degrades to a host path
    assert B.rgbd360_store_overlap(None, 0, None, None, None, None, None) == -1
    assert B.rgbd360_store_overlap_all(None, 0, None, None, 0.0, None, None, None) == -1
