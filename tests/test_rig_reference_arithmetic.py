"""rgbd360_rig_set_index_arithmetic(rig, 1): the 8-sensor dense registration (RegisterRGBD360::RegisterDensePhotoICP, csrc/rig_dense.h)
with the warp in the reference's own arithmetic -- the error pass through relPoseCam, the H / g pass through Rt^-1 (T (Rt p)), Eigen's
product order, double projection, round half away from zero.  The device is held to the numpy restatement of both chains
(tests/rig_reference.py, itself proven against the CPU oracle's math_mode 0 by test_rig_reference_cpu.py) pixel for pixel, and to
RigOracle(math_mode=0, reduce_mode=1) on the sums, the normal equations and the Levenberg-Marquardt sequence."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rgbd360_amd import synth
import rig_reference as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HG_RTOL, ERR2_RTOL = 2e-5, 2e-6              # as test_rig_dense.py
POSE_TOL_DEV = (5e-5, 2e-4)                  # as test_rig_dense.py
QVGA_K = (262.5, 262.5, 159.5, 119.5)        # 525 * 320 / 640 (RegisterRGBD360.h:357-365)


@pytest.fixture(scope="module")
def rig_pair():
    return synth.make_rig_pair(160, 120, seed=3, trans=0.04, rot_deg=1.5)


@pytest.fixture(scope="module")
def full_pair():
    return synth.make_rig_pair(320, 240, seed=9, trans=0.05, rot_deg=2.0)


def _oracle(oracle_mod, pair, mm, n_pyr=3, K=None):
    f1, f2, M, Rt, K0 = pair
    rig = oracle_mod.RigOracle(Rt, K or K0, n_pyr=n_pyr, math_mode=mm[0], reduce_mode=mm[1])
    for s in range(len(Rt)):
        rig.set_frame(s, True, *f1[s])
        rig.set_frame(s, False, *f2[s])
    return rig


def _gpu_rig(pair, n_pyr=3, mode=1, K=None):
    from rgbd360_amd.rig import RegisterDensePhotoICP
    f1, f2, M, Rt, K0 = pair
    reg = RegisterDensePhotoICP(Rt, K or K0, n_pyr=n_pyr)
    reg.set_index_arithmetic(mode)
    reg.setTargetFrame(f1)
    reg.setSourceFrame(f2)
    return reg


def test_warp_indices_equal_the_restatement_on_every_pixel(hip_lib, oracle_mod, full_pair):
    """Eight 320x240 sensors, 4 levels, 16 poses per level: in mode 1 both chains' indices equal the restatement on every pixel of every
    sensor.  The sweep discriminates: it holds pixels where the device definition (mode 0) lands elsewhere, and pixels where the two
    chains disagree."""
    f1, f2, M, Rt, K = full_pair
    n_pyr = 4
    reg = _gpu_rig(full_pair, n_pyr=n_pyr, mode=1)
    reg0 = _gpu_rig(full_pair, n_pyr=n_pyr, mode=0)
    sens = [rr.sensor_oracle(oracle_mod, f1[s], f2[s], K, n_pyr) for s in range(len(Rt))]
    rng = np.random.default_rng(21)
    n_dev_diff = n_chain_diff = n_vis = 0
    for level in range(n_pyr):
        rows, cols = sens[0].level_dims(level)
        luts = [o.lut_pinhole(level) for o in sens]
        Kl = rr.level_intrinsics(K, level)
        poses = [np.eye(4), M] + rr.random_poses(rng, 15, rot=0.05, trans=0.08)[1:]
        for T in poses:
            got = [reg.warp_indices(level, T, chain) for chain in (0, 1)]
            dev0 = reg0.warp_indices(level, T, 0)
            assert np.array_equal(dev0, reg0.warp_indices(level, T, 1))          # one chain in the device definition
            for s in range(len(Rt)):
                want0 = rr.warp_chain(T, Rt[s], luts[s], Kl, rows, cols, 0)[0]
                want1 = rr.warp_chain(T, Rt[s], luts[s], Kl, rows, cols, 1)[0]
                assert np.array_equal(got[0][s], want0), (level, s, int(np.any(got[0][s] != want0, axis=1).sum()))
                assert np.array_equal(got[1][s], want1), (level, s, int(np.any(got[1][s] != want1, axis=1).sum()))
                n_dev_diff += int(np.any(dev0[s] != want0, axis=1).sum())
                n_chain_diff += int(np.any(want0 != want1, axis=1).sum())
                n_vis += int((want0[:, 0] >= 0).sum())
    print(f"{n_vis} visible pixel warps; device definition differs on {n_dev_diff}, the two chains on {n_chain_diff}")
    assert n_dev_diff > 0 and n_chain_diff > 0


@pytest.mark.parametrize("salient", [False, True])
@pytest.mark.parametrize("method", [0, 1, 2])
def test_rig_eval_matches_the_oracle_math_mode_0(hip_lib, oracle_mod, rig_pair, method, salient):
    M = rig_pair[2]
    reg = _gpu_rig(rig_pair)
    ora = _oracle(oracle_mod, rig_pair, (0, 1))
    if salient:
        reg.useSaliency(True)
        ora.use_saliency(True, 0.01)
    rng = np.random.default_rng(4)
    poses = [np.eye(4), M, synth.make_pose(synth.rodrigues(rng.normal(size=3), 0.03), rng.normal(size=3) * 0.03)]
    for level in range(3):
        for T in poses:
            e = reg.eval(level, T, method)
            err, sums = ora.error(level, T, method)
            H, g, Hd, gd, n = ora.hessgrad(level, T, method)
            assert list(e["n_split"]) == [int(sums[2]), int(sums[3])] and e["n_rows"] == n, (level, e["n_split"], sums, e["n_rows"], n)
            assert abs(e["err2"] - err) <= ERR2_RTOL * max(err, 1.0)
            assert np.abs(e["H64"] - Hd).max() <= HG_RTOL * np.abs(Hd).max()
            assert np.abs(e["g64"] - gd).max() <= HG_RTOL * max(np.abs(gd).max(), 1e-3 * np.abs(Hd).max())


@pytest.mark.parametrize("method", [0, 1, 2])
def test_rig_align_matches_the_oracle_math_mode_0(hip_lib, oracle_mod, rig_pair, method):
    reg = _gpu_rig(rig_pair)
    ok = reg.align(np.eye(4), method)
    ora = _oracle(oracle_mod, rig_pair, (0, 1))
    st, pose_ref = ora.align(np.eye(4), method)
    assert ok and st == 0 and reg.num_iterations == ora.iters
    rot, trans = synth.pose_error(reg.getPose(), pose_ref)
    assert rot <= POSE_TOL_DEV[0] and trans <= POSE_TOL_DEV[1], (rot, trans)


@pytest.mark.parametrize("method", [0, 2])
def test_sample_pair_rig_align_in_the_reference_arithmetic(hip_lib, oracle_mod, method):
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import config1_samples as c1
    f1, f10 = c1.frames(1, "fixture"), c1.frames(10, "fixture")
    pair = (f1, f10, None, c1.extrinsics("fixture"), QVGA_K)
    reg = _gpu_rig(pair)
    ok = reg.align(np.eye(4), method)
    ora = _oracle(oracle_mod, pair, (0, 1))
    st, pose_ref = ora.align(np.eye(4), method)
    rot, trans = synth.pose_error(reg.getPose(), pose_ref)
    print(f"sample pair, method {method}: iters {reg.num_iterations} / {ora.iters}; vs oracle (0, 1) {rot:.2e} rad {trans:.2e} m")
    assert ok and st == 0 and reg.num_iterations == ora.iters == [10, 10, 10]
    assert rot <= POSE_TOL_DEV[0] and trans <= POSE_TOL_DEV[1], (rot, trans)


def test_seeded_motions_follow_the_reference_arithmetic(hip_lib, oracle_mod):
    """12 random rig motions, method 2: how many follow the (0, 1) oracle's accept / reject sequence and how many the (0, 0) one's.  Every
    motion must follow (0, 1) -- same status, iterations, and pose within POSE_TOL_DEV -- or its exception must be explained by the
    oracle's own trace: the step where the iteration counts part is a coin toss, a candidate whose error differs from the current one by
    less than MARGINAL of it (the device sums its float32 rows in another order, so such a step's update, and the sign of the error
    change, can flip; the indices are bit-equal, test_warp_indices_equal_the_restatement_on_every_pixel).  The pose stays within
    POSE_TOL_DEV either way."""
    MARGINAL = 1e-4
    follow01 = follow00 = 0
    explained = []
    for seed in range(40, 52):
        pair = synth.make_rig_pair(160, 120, seed=seed, trans=0.05, rot_deg=2.0)
        reg = _gpu_rig(pair)
        ok = reg.align(np.eye(4), 2)
        res = {}
        for mm in ((0, 1), (0, 0)):
            ora = _oracle(oracle_mod, pair, mm)
            st, pose = ora.align(np.eye(4), 2)
            res[mm] = (st, list(ora.iters), pose, ora.trace())
        st, iters, pose_ref, trace = res[(0, 1)]
        rot, trans = synth.pose_error(reg.getPose(), pose_ref)
        assert ok == (st == 0) and rot <= POSE_TOL_DEV[0] and trans <= POSE_TOL_DEV[1], (seed, rot, trans)
        follow00 += reg.num_iterations == res[(0, 0)][1]
        if reg.num_iterations == iters:
            follow01 += 1
            continue
        level = max(l for l in range(len(iters)) if reg.num_iterations[l] != iters[l])      # the first level (coarse to fine) that parts
        it = min(reg.num_iterations[level], iters[level])
        step = [t for t in trace if t[0] == level and t[1] == it]
        assert step, (seed, level, it)
        rel = max(abs(t[3] - t[4]) / t[3] for t in step)
        print(f"seed {seed}: iterations {reg.num_iterations} vs the (0, 1) oracle's {iters}; level {level} step {it}: error {step[0][3]:.10g}, "
              f"candidate {step[0][4]:.10g} (relative change {rel:.2e}); pose {rot:.2e} rad {trans:.2e} m")
        assert rel <= MARGINAL, (seed, step)
        explained.append(seed)
    print(f"12 motions: {follow01} follow the (0, 1) oracle's sequence, {follow00} the (0, 0) oracle's iteration counts; "
          f"explained coin tosses: {explained}")
    assert follow01 + len(explained) == 12 and len(explained) <= 2


def test_switching_back_restores_the_device_definition(hip_lib, rig_pair):
    from rgbd360_amd.register import Rgbd360Error
    M = rig_pair[2]
    reg = _gpu_rig(rig_pair, mode=0)
    assert reg.get_index_arithmetic() == 0
    e0 = reg.eval(1, M, 2)
    assert reg.align(np.eye(4), 2)
    p0, it0 = reg.getPose(), list(reg.num_iterations)
    reg.set_index_arithmetic(1)
    assert reg.get_index_arithmetic() == 1
    e1 = reg.eval(1, M, 2)
    assert reg.align(np.eye(4), 2)
    reg.set_index_arithmetic(0)
    e2 = reg.eval(1, M, 2)
    assert reg.align(np.eye(4), 2)
    assert np.array_equal(reg.getPose(), p0) and reg.num_iterations == it0
    for k in ("err2_split", "n_split", "H", "g", "H64", "g64"):
        assert np.array_equal(e0[k], e2[k]), k
    assert e0["n_rows"] == e2["n_rows"]
    assert not all(np.array_equal(e0[k], e1[k]) for k in ("err2_split", "H64"))      # mode 1 is another arithmetic
    for bad in (-1, 2, 7):
        with pytest.raises(Rgbd360Error):
            reg.set_index_arithmetic(bad)
    assert reg.get_index_arithmetic() == 0
    with pytest.raises(Rgbd360Error):
        reg.warp_indices(0, M, 2)                                    # chains are 0 and 1


# ---- the C++ adapter: RegisterRGBD360::setReferenceArithmetic(true) + RegisterDensePhotoICP -------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rgbd360/RegisterRGBD360.hpp"
using namespace rgbd360;
// argv: dir S rows cols n_pyr method reference(0/1).  dir holds rt.bin (S x 16 float, column-major), {1,2}_{s}.rgb / .dep (u8x3 / u16)
int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const std::string dir = argv[1];
    const int S = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), n_pyr = atoi(argv[5]), method = atoi(argv[6]), ref = atoi(argv[7]);
    auto load = [](const std::string& p, std::vector<unsigned char>& v) {
        FILE* f = fopen(p.c_str(), "rb");
        if (!f) return false;
        const bool ok = fread(v.data(), 1, v.size(), f) == v.size();
        fclose(f);
        return ok;
    };
    std::vector<unsigned char> rt(S * 16 * sizeof(float));
    if (!load(dir + "/rt.bin", rt)) return 3;
    std::vector<Mat4f> Rt(S);
    for (int s = 0; s < S; ++s) memcpy(Rt[s].m, rt.data() + s * 16 * sizeof(float), 16 * sizeof(float));
    std::vector<std::vector<unsigned char>> img(4 * S);
    std::vector<ImageView> views[4];
    for (int k = 0; k < 4; ++k)
        for (int s = 0; s < S; ++s) {
            const bool depth = k & 1;
            std::vector<unsigned char>& v = img[k * S + s];
            v.resize((size_t)rows * cols * (depth ? 2 : 3));
            if (!load(dir + "/" + std::to_string(k / 2 + 1) + "_" + std::to_string(s) + (depth ? ".dep" : ".rgb"), v)) return 3;
            ImageView iv;
            iv.data = v.data(); iv.rows = rows; iv.cols = cols;
            iv.step = (size_t)cols * (depth ? 2 : 3);
            iv.type = depth ? ImageView::U16C1 : ImageView::U8C3;
            views[k].push_back(iv);
        }
    RegisterRGBD360 reg;
    if (ref) reg.setReferenceArithmetic(true);
    const bool ok = reg.RegisterDensePhotoICP(views[0], views[1], views[2], views[3], Rt, Mat4f::Identity(),
                                              (RegisterPhotoICP::costFuncType)method, n_pyr);
    printf("status %d %d\n", ok ? 1 : 0, reg.status());
    const Mat4f P = reg.getPose();
    for (int k = 0; k < 16; ++k) printf("%a\n", P.m[k]);
    return 0;
}
"""


def _build_driver(tmp_path):
    from rgbd360_amd import build
    lib = build.build()
    src = tmp_path / "rig_reference_driver.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "rig_reference_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + os.path.dirname(lib), "-lrgbd360_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    return exe


@pytest.mark.parametrize("reference", [1, 0])
def test_cpp_adapter_reference_arithmetic_equals_the_python_mirror(hip_lib, tmp_path, rig_pair, reference):
    from rgbd360_amd.register import pose_from_cm, pose_to_cm
    f1, f2, M, Rt, K = rig_pair
    assert K == synth.pinhole_intrinsics(160, 120)                     # the adapter's own intrinsics (RegisterRGBD360.h:357-365)
    exe = _build_driver(tmp_path)
    np.concatenate([pose_to_cm(T) for T in Rt]).astype(np.float32).tofile(tmp_path / "rt.bin")
    for k, frame in ((1, f1), (2, f2)):
        for s, (rgb, dep) in enumerate(frame):
            np.ascontiguousarray(rgb, np.uint8).tofile(tmp_path / f"{k}_{s}.rgb")
            np.ascontiguousarray(dep, np.uint16).tofile(tmp_path / f"{k}_{s}.dep")
    out = subprocess.check_output([exe, str(tmp_path), str(len(Rt)), "120", "160", "3", "2", str(reference)], text=True).split("\n")
    assert out[0] == "status 1 0", out[0]
    pose_cpp = pose_from_cm(np.array([float.fromhex(x) for x in out[1:17]], np.float32))
    reg = _gpu_rig(rig_pair, mode=reference)
    assert reg.align(np.eye(4), 2)
    assert np.array_equal(pose_cpp, reg.getPose())
