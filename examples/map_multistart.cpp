// map_multistart.cpp -- relocalisation against the voxel map from a lattice of guesses in ONE call, through rgbd360/GlobalMap.hpp
// (rgbd360_map_align_batch_cloud / rgbd360_map_align_plane_batch_cloud, rgbd360_map_align_best).  The basin of one alignment against the
// map is about a voxel wide (max_dist <= the voxel size); a guess a few voxels off is recovered by starting from a 3 x 3 x 3 lattice of
// guesses around it, all aligned in lock step, and keeping the start that ends with the most matches.
//
// The scene is made here: a room corner (three walls of `size` metres, sampled every 2 cm) is the map, the same corner sampled every 4 cm
// and seen from a pose is the cloud, the guess is that pose moved by `offset`.
// Build:  g++ -std=c++17 -O2 -Iinclude examples/map_multistart.cpp -Lrgbd360_amd/lib -lrgbd360_hip
//             -Wl,-rpath,$PWD/rgbd360_amd/lib -o map_multistart
// Usage:  map_multistart [voxel size = 0.1] [lattice spacing = 0.2] [offset x y z = 0.21 -0.17 0.19] [plane = 0]
// Prints: centre status <s> matched <n> error <m>                 the single alignment from the wrong guess
//         job <j> status <s> iterations <i> matched <n> fitness <f> error <m>      per lattice guess
//         winner <j> matched <n> error <m>  (or "winner none")
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rgbd360/GlobalMap.hpp"

// the three walls x = 0, y = 0, z = 0 of a corner on a grid of `step` metres, moved into the frame of `pose` (world <- frame: a rotation
// about z by `yaw` and a translation)
static std::vector<float> corner(float size, float step, float yaw, const float t[3]) {
    std::vector<float> xyz;
    const float c = std::cos(yaw), s = std::sin(yaw);
    for (int axis = 0; axis < 3; ++axis)
        for (float u = 0.5f * step; u < size; u += step)
            for (float v = 0.5f * step; v < size; v += step) {
                float p[3] = {0.f, 0.f, 0.f};
                p[(axis + 1) % 3] = u;
                p[(axis + 2) % 3] = v;
                const float d[3] = {p[0] - t[0], p[1] - t[1], p[2] - t[2]};      // R^T (p - t)
                xyz.push_back(c * d[0] + s * d[1]);
                xyz.push_back(-s * d[0] + c * d[1]);
                xyz.push_back(d[2]);
            }
    return xyz;
}

static float distance(const rgbd360::Mat4f& a, const rgbd360::Mat4f& b) {
    return std::sqrt((a.m[12] - b.m[12]) * (a.m[12] - b.m[12]) + (a.m[13] - b.m[13]) * (a.m[13] - b.m[13]) + (a.m[14] - b.m[14]) * (a.m[14] - b.m[14]));
}

template <class Result>
static void report(const rgbd360::Mat4f& truth, const std::vector<rgbd360::Mat4f>& poses, const std::vector<Result>& results) {
    for (size_t j = 0; j < results.size(); ++j)
        printf("job %zu status %d iterations %d matched %lld fitness %.3e error %.4f\n", j, results[j].status, results[j].iterations, results[j].n_matched,
               results[j].fitness, distance(poses[j], truth));
    const int best = rgbd360::GlobalMap::bestJob(results, 6);
    if (best < 0) printf("winner none\n");
    else printf("winner %d matched %lld error %.4f\n", best, results[best].n_matched, distance(poses[best], truth));
}

int main(int argc, char** argv) {
    const float leaf = argc > 1 ? (float)atof(argv[1]) : 0.1f, spacing = argc > 2 ? (float)atof(argv[2]) : 0.2f;
    const float offset[3] = {argc > 5 ? (float)atof(argv[3]) : 0.21f, argc > 5 ? (float)atof(argv[4]) : -0.17f, argc > 5 ? (float)atof(argv[5]) : 0.19f};
    const bool plane = argc > 6 && atoi(argv[6]) != 0;
    try {
        rgbd360::RegisterPhotoICP align360;
        rgbd360::FilterPointCloud filter(leaf);
        for (int k = 0; k < 3; ++k) filter.lo[k] = -100.f, filter.hi[k] = 100.f;
        rgbd360::GlobalMap map(align360, filter, 1 << 16);
        const float zero[3] = {0.f, 0.f, 0.f};
        const std::vector<float> walls = corner(2.f, 0.02f, 0.f, zero);
        if (!map.insert(walls.data(), nullptr, (long long)(walls.size() / 3), rgbd360::Mat4f::Identity())) throw std::runtime_error("the map's table is full");

        const float yaw = 0.3f, t[3] = {0.8f, 0.6f, 0.7f};
        rgbd360::Mat4f truth = rgbd360::Mat4f::Identity();
        truth(0, 0) = std::cos(yaw), truth(0, 1) = -std::sin(yaw), truth(1, 0) = std::sin(yaw), truth(1, 1) = std::cos(yaw);
        for (int k = 0; k < 3; ++k) truth(k, 3) = t[k];
        const std::vector<float> cloud = corner(2.f, 0.04f, yaw, t);
        rgbd360::Mat4f centre = truth;
        for (int k = 0; k < 3; ++k) centre(k, 3) += offset[k];

        rgbd360::Mat4f pose;
        const int rc = plane ? map.alignCloudPlane(cloud.data(), (long long)(cloud.size() / 3), centre, pose)
                             : map.alignCloud(cloud.data(), (long long)(cloud.size() / 3), centre, pose);
        printf("centre status %d matched %lld error %.4f\n", rc, plane ? map.alignPlaneResult().n_matched : map.alignResult().n_matched, distance(pose, truth));

        const std::vector<rgbd360_map_batch_cloud> clouds = {{cloud.data(), (long long)(cloud.size() / 3)}};
        std::vector<rgbd360_map_batch_job> jobs;
        for (int i = -1; i <= 1; ++i)
            for (int j = -1; j <= 1; ++j)
                for (int k = -1; k <= 1; ++k) {
                    rgbd360::Mat4f guess = centre;
                    guess(0, 3) += spacing * i, guess(1, 3) += spacing * j, guess(2, 3) += spacing * k;
                    jobs.push_back(rgbd360::GlobalMap::batchJob(0, guess));
                }
        std::vector<rgbd360::Mat4f> poses;
        if (plane) {
            std::vector<rgbd360_map_align_plane_result> results;
            map.alignBatchCloudPlane(clouds, jobs, poses, results);
            report(truth, poses, results);
        } else {
            std::vector<rgbd360_map_align_result> results;
            map.alignBatchCloud(clouds, jobs, poses, results);
            report(truth, poses, results);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    return 0;
}
