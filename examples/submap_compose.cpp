// submap_compose.cpp -- a global map composed from submaps, and one submap re-posed after a pose-graph correction, through
// rgbd360/GlobalMap.hpp (rgbd360_map_merge / _unmerge / _records).  One small map is built per window of W frames, each frame inserted at
// its pose inside the window; the global map is the merge of the submaps at the windows' poses; a corrected window leaves the global map
// by unmerge at its old pose and comes back by merge at its new one -- exactly, and without the frames that built it.
//
// Frames: raw files written by tools/dump_sequence.py, frame_%03d.rgb (H*W*3 uint8), frame_%03d.depth (H*W uint16 mm).
// Poses:  a text file of numbers: n_frames x 16 (each frame in its window, column-major), then n_submaps x 16 (each window in the global
//         map), then the index of the submap to re-pose and its 16 new numbers.  n_submaps = ceil(n_frames / W).
// Build:  g++ -std=c++17 -O2 -Iinclude examples/submap_compose.cpp -Lrgbd360_amd/lib -lrgbd360_hip
//             -Wl,-rpath,$PWD/rgbd360_amd/lib -o submap_compose
// Usage:  submap_compose <dir> <n_frames> <width> <height> <W> <poses file> [submap voxel size = 0.05] [global voxel size = 0.05]
// Prints: submap <s> frames <first> <last> voxels <n>                       per submap
//         composed voxels <n> points <p> crc <CRC-32 of records(), 8 hex digits>
//         reposed submap <s> emptied <voxels emptied> voxels <n> points <p> tombstones <t> crc <...>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "rgbd360/GlobalMap.hpp"

struct Frame {
    std::vector<uint8_t> rgb;
    std::vector<uint16_t> depth;
    rgbd360::ImageView sphereRGB, sphereDepth;
    bool load(const std::string& dir, int k, int w, int h) {
        char name[512];
        rgb.resize((size_t)w * h * 3);
        depth.resize((size_t)w * h);
        snprintf(name, sizeof(name), "%s/frame_%03d.rgb", dir.c_str(), k);
        std::ifstream f1(name, std::ios::binary);
        if (!f1.read((char*)rgb.data(), rgb.size())) return false;
        snprintf(name, sizeof(name), "%s/frame_%03d.depth", dir.c_str(), k);
        std::ifstream f2(name, std::ios::binary);
        if (!f2.read((char*)depth.data(), depth.size() * 2)) return false;
        sphereRGB = {rgb.data(), h, w, (size_t)w * 3, rgbd360::ImageView::U8C3};
        sphereDepth = {depth.data(), h, w, (size_t)w * 2, rgbd360::ImageView::U16C1};
        return true;
    }
};

// CRC-32 (the polynomial of zlib and PNG) of the records' bytes
static uint32_t crc32(const std::vector<uint64_t>& words) {
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        table[i] = c;
    }
    uint32_t crc = 0xFFFFFFFFu;
    const uint8_t* p = (const uint8_t*)words.data();
    for (size_t i = 0; i < words.size() * sizeof(uint64_t); ++i) crc = table[(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
    return crc ^ 0xFFFFFFFFu;
}

static bool read_pose(std::ifstream& f, rgbd360::Mat4f& pose) {
    for (int k = 0; k < 16; ++k)
        if (!(f >> pose.m[k])) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: %s <dir> <n_frames> <width> <height> <W> <poses file> [submap voxel size] [global voxel size]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int n = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]), window = atoi(argv[5]);
    const float sub_leaf = argc > 7 ? (float)atof(argv[7]) : 0.05f, leaf = argc > 8 ? (float)atof(argv[8]) : 0.05f;
    if (n < 1 || window < 1) return 2;
    const int n_sub = (n + window - 1) / window;
    std::ifstream pf(argv[6]);
    std::vector<rgbd360::Mat4f> frame_pose(n), sub_pose(n_sub);
    for (rgbd360::Mat4f& p : frame_pose)
        if (!read_pose(pf, p)) return 3;
    for (rgbd360::Mat4f& p : sub_pose)
        if (!read_pose(pf, p)) return 3;
    int moved = 0;
    rgbd360::Mat4f new_pose;
    if (!(pf >> moved) || moved < 0 || moved >= n_sub || !read_pose(pf, new_pose)) return 3;
    try {
        rgbd360::RegisterPhotoICP align360;
        std::vector<std::unique_ptr<rgbd360::GlobalMap>> submaps;
        for (int s = 0; s < n_sub; ++s) {
            submaps.emplace_back(new rgbd360::GlobalMap(align360, rgbd360::FilterPointCloud(sub_leaf), 1 << 17));
            const int first = s * window, last = std::min(n, first + window) - 1;
            for (int k = first; k <= last; ++k) {
                Frame f;
                if (!f.load(dir, k, w, h)) return 3;
                if (!submaps[s]->insert(f.sphereRGB, f.sphereDepth, frame_pose[k], 2)) throw std::runtime_error("a submap's table is full");
            }
            printf("submap %d frames %d %d voxels %lld\n", s, first, last, submaps[s]->size());
        }
        rgbd360::GlobalMap global(align360, rgbd360::FilterPointCloud(leaf), 1 << 19);
        for (int s = 0; s < n_sub; ++s)
            if (!global.merge(*submaps[s], &sub_pose[s])) throw std::runtime_error("the global map's table is full");
        rgbd360_map_census_counts c = global.census();
        printf("composed voxels %lld points %lld crc %08x\n", global.size(), c.n_points, crc32(global.records()));
        // the correction: the window leaves at its old pose and comes back at its new one
        if (!global.unmerge(*submaps[moved], &sub_pose[moved])) throw std::runtime_error("unmerge: the global map does not hold the submap");
        const long long emptied = global.mergeStats().n_voxels_new;
        if (!global.merge(*submaps[moved], &new_pose)) throw std::runtime_error("the global map's table is full");
        c = global.census();
        printf("reposed submap %d emptied %lld voxels %lld points %lld tombstones %lld crc %08x\n", moved, emptied, global.size(), c.n_points,
               c.n_tombstones, crc32(global.records()));
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    return 0;
}
