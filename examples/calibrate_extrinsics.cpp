// calibrate_extrinsics.cpp -- the extrinsic half of the CLAMS loop on a recorded sequence of the 8-sensor rig: map with the extrinsics at
// hand, calibrate the eight rig <- sensor poses (and, with --refine, the rig poses of the window) against that map, move the frames in the
// map to the new poses, repeat; save Rt_01.txt .. Rt_08.txt where Calib360::loadExtrinsicCalibration reads them (Calib360.h:122-131).
// The intrinsic half -- the sensors' depth models trained against the same map -- is examples/calibrate_depth.cpp (DepthTrainerRig);
// the two alternate: map -> intrinsics + extrinsics -> re-map.  rgbd360_map_calibrate_rig_* (rgbd360_hip.h, "the rig's extrinsics").
//
// Build:  g++ -std=c++17 -O2 -Iinclude examples/calibrate_extrinsics.cpp -Lrgbd360_amd/lib -lrgbd360_hip
//             -Wl,-rpath,$PWD/rgbd360_amd/lib -o calibrate_extrinsics
// Usage:  calibrate_extrinsics <frames_dir> <n_frames> <poses.txt> <extrinsics_dir> <out_dir> [--rounds N] [--leaf L] [--refine]
//   <frames_dir>/sphere_images_<k>.bin   the frames (Frame360::loadFrame), k = 0 .. n_frames - 1
//   <poses.txt>                          one pose per frame (world <- rig), 16 numbers row by row: a pose graph's output
//   <extrinsics_dir>/Rt_0N.txt           the extrinsics to start from
//   <out_dir>/Rt_0N.txt                  the result, and next to it distortion_model1..8 trained against the re-mapped map
//   --rounds N    calibrate / re-map rounds (default 3)
//   --leaf L      the map's voxel size (default 0.05)
//   --refine      also refine the rig poses; sensor 0 then stays fixed (the gauge)
// Exit codes: 0 done, 2 usage, 3 an input is missing or unreadable, 4 the calibration is ill-posed or found no points.
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

// the packed cloud of a sensor's depth image: the ray of rgbd360_map_calibrate_rig_depth
static void sensor_cloud(const ImageView& d, const std::array<float, 4>& K, std::vector<float>& xyz) {
    xyz.clear();
    for (int v = 0; v < d.rows; ++v) {
        const uint16_t* row = (const uint16_t*)((const unsigned char*)d.data + (size_t)v * d.step);
        for (int u = 0; u < d.cols; ++u) {
            if (!row[u]) continue;
            const float z = 0.001f * (float)row[u];
            xyz.push_back(((float)u - K[2]) / K[0] * z);
            xyz.push_back(((float)v - K[3]) / K[1] * z);
            xyz.push_back(z);
        }
    }
}

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <frames_dir> <n_frames> <poses.txt> <extrinsics_dir> <out_dir> [--rounds N] [--leaf L] [--refine]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], out_dir = argv[5];
    const int n_frames = std::atoi(argv[2]);
    int rounds = 3, refine = 0;
    float leaf = 0.05f;
    for (int a = 6; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--refine")) refine = 1;
        else if (!std::strcmp(argv[a], "--rounds") && a + 1 < argc) rounds = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--leaf") && a + 1 < argc) leaf = (float)std::atof(argv[++a]);
        else {
            std::fprintf(stderr, "unknown option %s\n", argv[a]);
            return 2;
        }
    }
    if (n_frames < 1 || n_frames * 8 > RGBD360_MAP_BATCH_MAX || rounds < 1 || !(leaf > 0.f)) return 2;
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
        const std::array<float, 4> K = calib.K();
        std::vector<Mat4f> extrinsics(calib.Rt_.begin(), calib.Rt_.end());
        std::vector<ImageView> depths;
        std::vector<std::vector<float>> clouds((size_t)n_frames * 8);
        for (int k = 0; k < n_frames; ++k)
            for (int s = 0; s < 8; ++s) {
                depths.push_back(frames[(size_t)k]->sensorDepth(s));
                sensor_cloud(depths.back(), K, clouds[(size_t)k * 8 + s]);
            }

        // 1 the map with the extrinsics at hand: every sensor's cloud at frame pose x Rt_[s]
        RegisterPhotoICP align;
        GlobalMap map(align, FilterPointCloud(leaf, 1e3f));
        std::vector<Mat4f> at((size_t)n_frames * 8);
        for (int k = 0; k < n_frames; ++k)
            for (int s = 0; s < 8; ++s) {
                const size_t i = (size_t)k * 8 + s;
                at[i] = DepthTrainerRig::multiply(poses[(size_t)k], extrinsics[(size_t)s]);
                if (!map.insert(clouds[i].data(), nullptr, (long long)(clouds[i].size() / 3), at[i])) {
                    std::fprintf(stderr, "the map is full: a larger --leaf or a shorter sequence\n");
                    return 3;
                }
            }

        rgbd360_rig_calib_params p = map.rigCalibParams();
        p.refine_poses = refine;
        p.fixed_sensor = refine ? 0 : -1;
        for (int round = 0; round < rounds; ++round) {
            // 2 calibrate against the map as it is ...
            const int status = map.calibrateRigDepth(depths, K, poses, extrinsics, &p);
            const rgbd360_rig_calib_result& r = map.rigCalibResult();
            std::printf("round %d: status %d, %d steps, %d inputs, %lld points, rms %.4f m\n", round, status, r.iterations, r.n_inputs_used, r.n_matched,
                        std::sqrt(r.fitness));
            if (status != RGBD360_OK) return 4;
            // 3 ... and re-map: every cloud moves from the pose it was inserted at to its new one
            for (int k = 0; k < n_frames; ++k)
                for (int s = 0; s < 8; ++s) {
                    const size_t i = (size_t)k * 8 + s;
                    const Mat4f now = DepthTrainerRig::multiply(poses[(size_t)k], extrinsics[(size_t)s]);
                    if (!map.move(clouds[i].data(), nullptr, (long long)(clouds[i].size() / 3), at[i], now)) {
                        std::fprintf(stderr, "the map lost track of a cloud (%lld points missing)\n", (long long)map.editStats().n_missing);
                        return 3;
                    }
                    at[i] = now;
                }
        }
        if (!GlobalMap::saveExtrinsics(extrinsics, out_dir)) {
            std::fprintf(stderr, "cannot write %s/Rt_0N.txt\n", out_dir.c_str());
            return 3;
        }
        for (int s = 0; s < 8; ++s) calib.setRt_id(s, extrinsics[(size_t)s]);      // (or calib.loadExtrinsicCalibration(out_dir))
        std::printf("wrote %s/Rt_01.txt .. Rt_08.txt\n", out_dir.c_str());

        // 4 the other half of the alternation: the depth models trained against the re-mapped map with the new extrinsics (the frames hold
        //   `calib`), as examples/calibrate_depth.cpp does; a caller undistorts, re-maps and starts over
        DepthTrainerRig rig(align, frames[0]->sensorCols(), frames[0]->sensorRows(), 4, 3, 2.0, 1);
        rgbd360_depth_train_stats total{};
        for (int k = 0; k < n_frames; ++k) rig.accumulate(*frames[(size_t)k], poses[(size_t)k], map, nullptr, &total);
        if (total.n_examples > 0) {
            rig.saveIntrinsicCalibration(out_dir);
            std::printf("wrote %s/distortion_model1..8 from %lld examples\n", out_dir.c_str(), total.n_examples);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
