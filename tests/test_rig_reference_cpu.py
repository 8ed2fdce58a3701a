"""tests/rig_reference.py -- the numpy restatement of the rig's warp in the reference's arithmetic (both chains) -- against the CPU
oracle's math_mode 0 (oracle/photo_icp_ref.cpp warp_robot): a one-sensor RigOracle(math_mode=0, reduce_mode=1) on several sensors,
poses and every level.  Chain 0's visible counts are error()'s nP / nD and its error sums match to float rounding; chain 1's indices
give hessgrad()'s Jacobian-row count.  This is the checker the GPU test (test_rig_reference_arithmetic.py) holds the device to."""
import numpy as np
import pytest

from rgbd360_amd import synth
import rig_reference as rr

N_PYR = 3


@pytest.fixture(scope="module")
def pair():
    return synth.make_rig_pair(160, 120, seed=5, trans=0.04, rot_deg=1.5)


def test_round_half_away_from_zero():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, -0.49999999999999994, 3.0, -3.0, 1e9])
    assert rr.round_half_away(x).tolist() == [1, 2, 3, -1, -2, -3, 0, 0, 3, -3, 1e9]
    assert np.round(2.5) == 2.0            # why np.round is not C round()


@pytest.mark.parametrize("sensor", [0, 3, 6])
def test_restatement_equals_the_oracle_math_mode_0(oracle_mod, pair, sensor):
    f1, f2, M, Rt, K = pair
    o = rr.sensor_oracle(oracle_mod, f1[sensor], f2[sensor], K, N_PYR)
    rig = oracle_mod.RigOracle([Rt[sensor]], K, n_pyr=N_PYR, math_mode=0, reduce_mode=1)
    rig.set_frame(0, True, *f1[sensor])
    rig.set_frame(0, False, *f2[sensor])
    prm = o.params
    poses = rr.random_poses(np.random.default_rng(100 + sensor), 5) + [M]
    n_chain_diff = 0
    for level in range(N_PYR):
        rows, cols = o.level_dims(level)
        lut = o.lut_pinhole(level)
        Kl = rr.level_intrinsics(K, level)
        planes = {k: o.plane(k, level) for k in ("gray_src", "gray_trg", "depth_trg", "gx", "gy", "dgx", "dgy")}
        for T in poses:
            rc0, P0, _ = rr.warp_chain(T, Rt[sensor], lut, Kl, rows, cols, 0)
            rc1, _, _ = rr.warp_chain(T, Rt[sensor], lut, Kl, rows, cols, 1)
            n_chain_diff += int(np.any(rc0 != rc1, axis=1).sum())
            for method in (0, 1, 2):
                err, sums = rig.error(level, T, method)
                e2p, e2d, nP, nD = rr.error_sums(rc0, P0, planes["gray_src"], planes["gray_trg"], planes["depth_trg"], prm.sigma_photo,
                                                 prm.sigma_depth, method)
                assert (nP, nD) == (int(sums[2]), int(sums[3])), (level, method, nP, nD, sums)
                assert abs(e2p - sums[0]) <= 1e-6 * max(sums[0], 1.0) and abs(e2d - sums[1]) <= 1e-6 * max(sums[1], 1.0), (e2p, e2d, sums)
                n_rows = rr.row_count(rc1, planes["depth_trg"], planes["gx"], planes["gy"], planes["dgx"], planes["dgy"], prm.thres_sal_photo,
                                      prm.thres_sal_depth, method)
                assert n_rows == rig.hessgrad(level, T, method)[4], (level, method)
    print(f"sensor {sensor}: {n_chain_diff} pixels where the two chains disagree")


def test_chains_differ_on_a_fine_sweep(oracle_mod, pair):
    """The two chains are not the same warp: over a sweep of poses some pixels land on different targets (or are visible in one only)."""
    f1, f2, M, Rt, K = pair
    o = rr.sensor_oracle(oracle_mod, f1[1], f2[1], K, N_PYR)
    lut, (rows, cols) = o.lut_pinhole(0), o.level_dims(0)
    n = 0
    for T in rr.random_poses(np.random.default_rng(7), 12):
        rc0, _, _ = rr.warp_chain(T, Rt[1], lut, rr.level_intrinsics(K, 0), rows, cols, 0)
        rc1, _, _ = rr.warp_chain(T, Rt[1], lut, rr.level_intrinsics(K, 0), rows, cols, 1)
        n += int(np.any(rc0 != rc1, axis=1).sum())
    assert n > 0


def test_cpp_adapter_with_reference_arithmetic_compiles_and_links(tmp_path):
    """RegisterRGBD360::setReferenceArithmetic + RegisterDensePhotoICP compile and link against the library (no GPU: the driver stops
    at its missing input files, exit 3)."""
    import subprocess
    from test_rig_reference_arithmetic import _build_driver
    exe = _build_driver(tmp_path)
    assert subprocess.call([exe, str(tmp_path / "missing"), "8", "120", "160", "3", "2", "1"]) == 3
