"""rgbd360_warp_images without a GPU: the reference builder (tests/warp_images_reference.py) on a hand-made case, the non-vacuity of
the inputs the GPU tests use (measured with the CPU oracle), and the C++ adapter's warpImages surface (compile + link)."""
import os
import subprocess

import numpy as np

from rgbd360_amd import synth
from tests import warp_images_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN = F(np.nan)


def test_hand_made_case_triple_collision_hole_and_ineligible_targets():
    """Six source pixels onto a 2 x 3 target at the identity pose.  Sources 0, 1, 3 collide on (0,0): 3 wins.  Source 2 is not visible.
    Source 5 lands on (0,1), whose target depth is NaN (no depth write for the spherical path, RPI.h:3064).  Source 4 lands on (1,2),
    whose gray gradient is below the threshold (no depth write with PHOTO_DEPTH only, RPI.h:3038-3039).  (0,2), (1,0), (1,1) are holes."""
    idx = np.array([[0, 0], [0, 0], [-1, -1], [0, 0], [1, 2], [0, 1]], np.int32)
    lut = np.array([[1, 0, 0], [0, 1, 0], [9, 9, 9], [3, 4, 0], [0, 0, 2], [1, 2, 2]], F)       # ranges 1, 1, -, 5, 2, 3; z 0, 0, -, 0, 2, 2
    gray_src = np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], F)
    gray_trg = np.array([[0.5, 0.25, 0.75], [1.0, 0.0, 0.125]], F)
    depth_trg = np.array([[4.0, NAN, 2.0], [1.0, np.inf, 3.0]], F)
    gx = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.001]], F)
    gy = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -0.002]], F)
    Z = F(0)
    want_winner = np.array([[3, 5, -1], [-1, -1, 4]], np.int32)
    want_gray = np.array([[0.4, 0.6, Z], [Z, Z, 0.5]], F)
    want_dgray = np.abs(gray_trg - want_gray)
    zeros = np.zeros((2, 3), F)
    want_depth = {1: np.array([[5, 0, 0], [0, 0, 2]], F), 2: np.array([[5, 0, 0], [0, 0, 0]], F)}
    want_ddepth = {1: np.array([[1, NAN, 2], [1, np.inf, 1]], F), 2: np.array([[1, NAN, 2], [1, np.inf, 3]], F)}
    for method in (0, 1, 2):
        got = W.planes_from(idx, lut, np.eye(4), method, gray_src, gray_trg, depth_trg, gx, gy, thres=F(0.01))
        assert np.array_equal(got["winner"], want_winner), method
        assert np.array_equal(got["warped_gray"], zeros if method == 1 else want_gray), method
        assert np.array_equal(got["diff_gray"], zeros if method == 1 else want_dgray), method
        assert np.array_equal(got["warped_depth"], zeros if method == 0 else want_depth[method]), method
        assert np.array_equal(got["diff_depth"], zeros if method == 0 else want_ddepth[method], equal_nan=True), method
    # the pinhole rules: the transformed z, and no test of the target depth (RPI.h:1051)
    got = W.planes_from(idx, lut, np.eye(4), 1, gray_src, gray_trg, depth_trg, gx, gy, pinhole=True, thres=F(0.01))
    assert np.array_equal(got["warped_depth"], np.array([[0, 2, 0], [0, 0, 2]], F))
    assert np.array_equal(got["diff_depth"], np.array([[4, NAN, 2], [1, np.inf, 1]], F), equal_nan=True)
    got = W.planes_from(idx, lut, np.eye(4), 2, gray_src, gray_trg, depth_trg, gx, gy, pinhole=True, thres=F(0.01))
    assert np.array_equal(got["warped_depth"], np.array([[0, 2, 0], [0, 0, 0]], F))
    assert np.array_equal(W.counts(idx, 2, 3), [3, 1, 0, 0, 0, 1])


def test_gpu_test_inputs_are_not_vacuous(oracle_mod, small_pair):
    """What the GPU tests rely on, measured with the oracle at 256 x 128, level 0, pose T_gt . translate(0.2, 0.3, 0.5): 23 503 of
    32 768 targets hit, 5 251 with >= 2 sources, 102 sources on one target, 9 265 holes, 8 415 targets where the method-2 depth plane
    differs from method 1; with spoiled float32 depth 823 visible pixels land on a non-finite target depth.  Each at least half of
    that, so a later change of synth cannot hollow the GPU tests out."""
    O = oracle_mod
    (rgbA, dA), (rgbB, dB), T_gt = small_pair
    P = W.pushed(T_gt)
    ora = O.Oracle(n_pyr=3, math_mode=0, reduce_mode=1)
    ora.set_target(rgbA, dA)
    ora.set_source(rgbB, dB)
    m1, m2 = W.from_oracle(ora, 0, P, 1), W.from_oracle(ora, 0, P, 2)
    c = W.counts(m1["idx"], 128, 256)
    figures = dict(hit=int((c > 0).sum()), multi=int((c >= 2).sum()), most=int(c.max()), holes=int((c == 0).sum()),
                   coupling=int((m1["warped_depth"] != m2["warped_depth"]).sum()))
    print(figures)
    assert figures["hit"] + figures["holes"] == 128 * 256
    quoted = dict(hit=23503, multi=5251, most=102, holes=9265, coupling=8415)
    for k, v in quoted.items():
        assert 2 * figures[k] >= v, (k, figures[k], v)
    ora.close()
    (rgbA, dA), (rgbB, dB), _ = synth.make_pair(256, 128, seed=1234, depth_f32=True)
    ora = O.Oracle(n_pyr=3, math_mode=0, reduce_mode=1)
    ora.set_target(rgbA, synth.spoil_depth(dA, 4))
    ora.set_source(rgbB, synth.spoil_depth(dB, 3))
    idx = ora.warp_indices(0, P)
    vis = idx[:, 0] >= 0
    n_nonfinite = int((~np.isfinite(ora.plane("depth_trg", 0)[idx[vis, 0], idx[vis, 1]])).sum())
    print("visible pixels on a non-finite target depth:", n_nonfinite)
    assert 2 * n_nonfinite >= 823
    ora.close()


_SNIPPET = r'''
#include <cstdio>
#include <rgbd360/RegisterPhotoICP.hpp>
int main(int argc, char**) {
    if (argc < 2) return 3;                       // (never run without a GPU: this is a compile + link check)
    rgbd360::RegisterPhotoICP align360;
    align360.setNumPyr(1);
    const rgbd360::WarpedImages w = align360.warpImages(rgbd360::Mat4f::Identity(), rgbd360::RegisterPhotoICP::PHOTO_DEPTH);
    const rgbd360::WarpedImages p = align360.warpImagesPinhole(rgbd360::Mat4f::Identity(), rgbd360::RegisterPhotoICP::DEPTH_CONSISTENCY, 0);
    const std::vector<float>* planes[4] = {&w.gray, &w.depth, &w.diffGray, &w.diffDepth};
    const std::vector<int32_t>& winner = p.winner;
#if defined(EXPECT_OPENCV) && !defined(RGBD360_HAVE_OPENCV)
#error "the mock OpenCV headers were not picked up"
#endif
#ifdef RGBD360_HAVE_OPENCV
    cv::Mat& g = align360.warped_source_grayImage;      // RPI.h:163-166
    cv::Mat& d = align360.warped_source_depthImage;
    if (g.type() != CV_32FC1 || d.rows != w.rows) return 4;
#endif
    printf("%d %d %zu %zu\n", w.rows, w.cols, planes[3]->size(), winner.size());
    return 0;
}
'''


def test_adapter_warp_images_compiles_and_links(tmp_path):
    """RegisterPhotoICP::warpImages / warpImagesPinhole and the WarpedImages POD against the C ABI, without and with the mock Eigen /
    OpenCV headers (the cv::Mat members warped_source_grayImage / warped_source_depthImage, RPI.h:163-166)."""
    from rgbd360_amd import build
    lib = build.build()
    src = tmp_path / "warp_images_snippet.cpp"
    src.write_text(_SNIPPET)
    for name, extra in (("plain", []), ("mock", ["-I" + os.path.join(ROOT, "tests", "mock_headers"), "-DEXPECT_OPENCV"])):
        exe = str(tmp_path / ("warp_images_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror=return-type"] + extra +
                              ["-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.dirname(lib), "-lrgbd360_hip",
                               "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
        assert subprocess.call([exe]) == 3
