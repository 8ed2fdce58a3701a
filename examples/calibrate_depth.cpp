// calibrate_depth.cpp -- the CLAMS loop on a recorded sequence of the 8-sensor rig: map from trusted short-range data, train the eight
// sensors' depth-distortion models against that map, save them where Calib360::loadIntrinsicCalibration reads them (Calib360.h:104-119).
// The training half of clams::DiscreteDepthDistortionModel (OpenNI2_Grabber/third_party/CLAMS/discrete_depth_distortion_model.cpp:21-36,
// 193-217) on the device: include/rgbd360/DepthTrainer.hpp, rgbd360_depth_trainer_* (rgbd360_hip.h, "training the depth model").  The
// models are then applied and judged on the device too (rgbd360_depth_models_*, "applying the depth models on the device"): every fifth
// frame is held out of the training, and its raw against corrected RMS and bias to the map are printed.
//
// Build:  g++ -std=c++17 -O2 -Iinclude examples/calibrate_depth.cpp -Lrgbd360_amd/lib -lrgbd360_hip
//             -Wl,-rpath,$PWD/rgbd360_amd/lib -o calibrate_depth
// Usage:  calibrate_depth <frames_dir> <n_frames> <poses.txt> <extrinsics_dir> <out_dir> [--near R] [--leaf L] [--bin-depth D]
//   <frames_dir>/sphere_images_<k>.bin   the frames (Frame360::loadFrame), k = 0 .. n_frames - 1
//   <poses.txt>                          one corrected pose per frame (world <- rig), 16 numbers row by row: a pose graph's output
//   <extrinsics_dir>/Rt_0N.txt           the rig's extrinsics (Calib360::loadExtrinsicCalibration)
//   <out_dir>/distortion_model1..8       the result
//   --near R      only measurements with z <= R metres build the map (default 2.0: where the sensors are trusted); all train
//   --leaf L      the map's voxel size (default 0.03)
//   --bin-depth D the slices' depth (default 2.0, CLAMS')
// Exit codes: 0 done, 2 usage, 3 an input is missing or unreadable, 4 no training example.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rgbd360/DepthTrainer.hpp"

using namespace rgbd360;

static bool read_poses(const char* path, int n, std::vector<Mat4f>& poses) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) return false;
    poses.assign((size_t)n, Mat4f::Identity());
    bool ok = true;
    for (int k = 0; k < n && ok; ++k)
        for (int r = 0; r < 4 && ok; ++r)
            for (int c = 0; c < 4 && ok; ++c) ok = std::fscanf(f, "%f", &poses[(size_t)k](r, c)) == 1;
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <frames_dir> <n_frames> <poses.txt> <extrinsics_dir> <out_dir> [--near R] [--leaf L] [--bin-depth D]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], out_dir = argv[5];
    const int n_frames = std::atoi(argv[2]);
    float near_range = 2.0f, leaf = 0.03f;
    double bin_depth = 2.0;
    for (int a = 6; a + 1 < argc; a += 2) {
        if (!std::strcmp(argv[a], "--near")) near_range = (float)std::atof(argv[a + 1]);
        else if (!std::strcmp(argv[a], "--leaf")) leaf = (float)std::atof(argv[a + 1]);
        else if (!std::strcmp(argv[a], "--bin-depth")) bin_depth = std::atof(argv[a + 1]);
        else {
            std::fprintf(stderr, "unknown option %s\n", argv[a]);
            return 2;
        }
    }
    if (n_frames < 1 || !(near_range > 0.f) || !(leaf > 0.f) || !(bin_depth > 0.0)) return 2;
    std::vector<Mat4f> poses;
    Calib360 calib;
    if (!read_poses(argv[3], n_frames, poses) || !calib.loadExtrinsicCalibration(argv[4])) {
        std::fprintf(stderr, "cannot read the poses or the extrinsics\n");
        return 3;
    }
    try {
        std::vector<std::unique_ptr<Frame360>> frames;
        for (int k = 0; k < n_frames; ++k) {
            frames.emplace_back(new Frame360(&calib));
            frames.back()->loadFrame(dir + "/sphere_images_" + std::to_string(k) + ".bin");
        }
        const int rows = frames[0]->sensorRows(), cols = frames[0]->sensorCols();
        const std::array<float, 4> K = calib.K();

        // 1 the map from trusted short-range data: every sensor's points with z <= near_range (a box in the sensor's frame), at the
        //   corrected poses
        RegisterPhotoICP align;
        FilterPointCloud filter(leaf);
        filter.lo[0] = filter.lo[1] = -near_range, filter.lo[2] = 0.f;
        filter.hi[0] = filter.hi[1] = filter.hi[2] = near_range;
        GlobalMap map(align, filter);
        std::vector<float> xyz((size_t)rows * cols * 3);
        for (int k = 0; k < n_frames; ++k) {
            for (int s = 0; s < 8; ++s) {
                const ImageView d = frames[(size_t)k]->sensorDepth(s);
                long long n = 0;
                for (int v = 0; v < rows; ++v) {
                    const uint16_t* row = (const uint16_t*)((const unsigned char*)d.data + (size_t)v * d.step);
                    for (int u = 0; u < cols; ++u) {
                        if (!row[u]) continue;
                        const float z = 0.001f * (float)row[u];
                        xyz[3 * n] = ((float)u - K[2]) / K[0] * z, xyz[3 * n + 1] = ((float)v - K[3]) / K[1] * z, xyz[3 * n + 2] = z;
                        ++n;
                    }
                }
                if (!map.insert(xyz.data(), nullptr, n, DepthTrainerRig::multiply(poses[(size_t)k], calib.Rt_[(size_t)s]))) {
                    std::fprintf(stderr, "the map is full: a larger --leaf or a shorter sequence\n");
                    return 3;
                }
            }
        }
        std::printf("map: %lld voxels of %.3f m from measurements within %.2f m\n", (long long)map.size(), leaf, near_range);

        // 2 train: all eight sensors of every frame against the map (4 x 3-pixel bins on the rig's half-size images: the files' 8 x 6)
        DepthTrainerRig rig(align, cols, rows, 4, 3, bin_depth, 1);
        rgbd360_depth_train_stats total{};
        //   every fifth frame is held out of the training and judges the models in step 3
        const auto held_out = [&](int k) { return n_frames >= 5 && k % 5 == 4; };
        for (int k = 0; k < n_frames; ++k)
            if (!held_out(k)) rig.accumulate(*frames[(size_t)k], poses[(size_t)k], map, nullptr, &total);
        std::printf("pixels %lld: no measurement %lld, no hit %lld, off plane %lld, grazing %lld, out of range %lld, multiplier rejected %lld, examples %lld\n",
                    total.n_pixels, total.n_no_measurement, total.n_no_hit, total.n_off_plane, total.n_grazing, total.n_out_of_range, total.n_mult_rejected,
                    total.n_examples);
        if (total.n_examples == 0) return 4;

        // 3 the eight files, in the full-resolution form Calib360::loadIntrinsicCalibration halves; then undistort with them
        rig.saveIntrinsicCalibration(out_dir);
        if (!calib.loadIntrinsicCalibration(out_dir)) {
            std::fprintf(stderr, "cannot read back the models written to %s\n", out_dir.c_str());
            return 3;
        }
        std::printf("wrote %s/distortion_model1..8\n", out_dir.c_str());
        //   on the device: the models resident (DepthModels), the first frame's eight images corrected in one launch, and the held-out
        //   frames' raw against corrected error to the map (rgbd360_depth_evaluate_map), sensor by sensor
        DepthModels models(align, calib);
        frames[0]->undistortOnDevice(align.context(), models.handle());
        rgbd360_depth_eval_sums sums{};
        for (int k = 0; k < n_frames; ++k) {
            if (n_frames >= 5 && !held_out(k)) continue;
            for (int s = 0; s < 8; ++s)
                DepthModels::add(sums, models.evaluate(map, s, frames[(size_t)k]->sensorDepth(s), K, DepthTrainerRig::multiply(poses[(size_t)k], calib.Rt_[(size_t)s])));
        }
        std::printf("%s frames against the map, %lld examples: RMS %.4f m raw, %.4f m corrected; bias %+.4f m raw, %+.4f m corrected\n",
                    n_frames >= 5 ? "held-out" : "training", sums.n, DepthModels::rms(sums.raw_ee, sums.n), DepthModels::rms(sums.cor_ee, sums.n),
                    DepthModels::bias(sums.raw_e, sums.n), DepthModels::bias(sums.cor_e, sums.n));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
