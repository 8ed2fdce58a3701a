// keyframe_odometry.cpp -- the keyframe loop of the reference's Registration/OdometryKeyFrame360.cpp:212-300 through the resident
// frame store (rgbd360/FrameStore.hpp): the keyframe is the TARGET of every alignment, each new frame a SOURCE, the guess is the
// previous dense result against the same keyframe, and the keyframe stays while the alignment's avDepthResidual is below the
// threshold (0.9 there).  A frame that fails the test becomes the next keyframe.
//
// Frames are processed in windows: the frames of a window are put into the store together (one fused set-up) and aligned against
// the keyframe by ONE rgbd360_store_align call, all from the last result of the previous window.  When a frame of the window becomes
// the keyframe, the frames behind it stay resident and are aligned again, against the new keyframe, with the next window: no frame is
// prepared twice.
//
// Frames: raw files written by tools/dump_sequence.py, frame_%03d.rgb (H*W*3 uint8), frame_%03d.depth (H*W uint16 mm).
// Build:  g++ -std=c++17 -O2 -Iinclude examples/keyframe_odometry.cpp -Lrgbd360_amd/lib -lrgbd360_hip
//             -Wl,-rpath,$PWD/rgbd360_amd/lib -o keyframe_odometry
// Usage:  keyframe_odometry <dir> <n_frames> <width> <height> [window = 4] [max avDepthResidual = 0.9] [--warp-images <prefix>]
//         --warp-images: after the last alignment, the last frame warped into its keyframe at the solved pose and the photometric
//         difference (RegisterPhotoICP::warpImages, level 0) as <prefix>_warped_gray.pgm and <prefix>_diff_gray.pgm (binary PGM)
// Prints per frame:  frame <i> kf <keyframe> status <s> pose <16 floats, column-major: the frame in its keyframe> res <avDepthResidual> sso <SSO>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "rgbd360/FrameStore.hpp"

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

// float plane in [0, 1] -> 8-bit binary PGM
static bool write_pgm(const std::string& path, const std::vector<float>& v, int rows, int cols) {
    std::vector<uint8_t> px(v.size());
    for (size_t i = 0; i < v.size(); ++i) px[i] = (uint8_t)(255.f * (v[i] < 0.f ? 0.f : (v[i] > 1.f ? 1.f : v[i])) + 0.5f);
    std::ofstream f(path, std::ios::binary);
    f << "P5\n" << cols << " " << rows << "\n255\n";
    f.write((const char*)px.data(), px.size());
    return (bool)f;
}

int main(int argc, char** argv) {
    std::string warp_prefix;
    for (int a = 1; a + 1 < argc; ++a)
        if (!strcmp(argv[a], "--warp-images")) {      // taken out of the positional arguments
            warp_prefix = argv[a + 1];
            for (int b = a; b + 2 < argc; ++b) argv[b] = argv[b + 2];
            argc -= 2;
            break;
        }
    if (argc < 5) {
        fprintf(stderr, "usage: %s <dir> <n_frames> <width> <height> [window] [max avDepthResidual]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int n = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]);
    const int window = argc > 5 ? atoi(argv[5]) : 4;
    const double max_residual = argc > 6 ? atof(argv[6]) : 0.9;
    if (n < 1 || window < 1 || window > 64) return 2;
    Frame first;
    if (!first.load(dir, 0, w, h)) return 3;
    try {
        rgbd360::RegisterPhotoICP align360;
        align360.setNumPyr(4);
        align360.useSaliency(false);
        rgbd360::FrameStore store(align360, window + 1, h, w);
        std::vector<int> free_entries;
        for (int e = window; e >= 1; --e) free_entries.push_back(e);
        int kf = 0, kf_entry = 0;
        store.put(kf_entry, first.sphereRGB, first.sphereDepth);
        rgbd360::Mat4f guess = rgbd360::Mat4f::Identity();
        struct Pending {
            int frame, entry;
        };
        std::vector<Pending> pending;      // resident frames waiting for their alignment against the current keyframe
        int next = 1;
        int last_kf = -1, last_frame = -1;      // the last alignment that succeeded, for --warp-images
        rgbd360::Mat4f last_pose = rgbd360::Mat4f::Identity();
        while (next < n || !pending.empty()) {
            std::vector<Frame> fresh;
            std::vector<int> entries;
            std::vector<rgbd360::ImageView> rgb, depth;
            fresh.reserve(window);
            while ((int)pending.size() < window && next < n) {
                fresh.emplace_back();
                if (!fresh.back().load(dir, next, w, h)) return 3;
                entries.push_back(free_entries.back());
                free_entries.pop_back();
                rgb.push_back(fresh.back().sphereRGB);
                depth.push_back(fresh.back().sphereDepth);
                pending.push_back({next++, entries.back()});
            }
            store.put(entries, rgb, depth);
            std::vector<rgbd360::FrameStore::Pair> pairs;
            for (const Pending& p : pending) pairs.push_back({kf_entry, p.entry});
            std::vector<rgbd360_result> res;
            const std::vector<rgbd360::Mat4f> poses =
                store.align(pairs, std::vector<rgbd360::Mat4f>(pairs.size(), guess), RGBD360_PHOTO_DEPTH, 32, &res);
            size_t j = 0;
            for (; j < pending.size(); ++j) {
                printf("frame %d kf %d status %d pose", pending[j].frame, kf, res[j].status);
                for (int k = 0; k < 16; ++k) printf(" %.9g", poses[j].m[k]);
                printf(" res %.9g sso %.9g\n", res[j].rms_depth, (double)res[j].sso);
                if (res[j].status == 0) { last_kf = kf; last_frame = pending[j].frame; last_pose = poses[j]; }
                if (res[j].status == 0 && res[j].rms_depth < max_residual) {      // "skip frame": the keyframe stays
                    guess = poses[j];
                    free_entries.push_back(pending[j].entry);
                    continue;
                }
                free_entries.push_back(kf_entry);      // this frame is the new keyframe; the frames behind it are aligned again
                kf = pending[j].frame;
                kf_entry = pending[j].entry;
                guess = rgbd360::Mat4f::Identity();
                ++j;
                break;
            }
            pending.erase(pending.begin(), pending.begin() + j);
        }
        if (!warp_prefix.empty() && last_frame >= 0) {
            // a one-pair object of its own (the store's frames are not the context's target / source): the pair is read again
            Frame trg, src;
            if (!trg.load(dir, last_kf, w, h) || !src.load(dir, last_frame, w, h)) return 3;
            rgbd360::RegisterPhotoICP viz;
            viz.setNumPyr(4);
            viz.setTargetFrame(trg.sphereRGB, trg.sphereDepth);
            viz.setSourceFrame(src.sphereRGB, src.sphereDepth);
            const rgbd360::WarpedImages wi = viz.warpImages(last_pose, rgbd360::RegisterPhotoICP::PHOTO_DEPTH, 0);
            if (!write_pgm(warp_prefix + "_warped_gray.pgm", wi.gray, wi.rows, wi.cols) ||
                !write_pgm(warp_prefix + "_diff_gray.pgm", wi.diffGray, wi.rows, wi.cols)) return 3;
            fprintf(stderr, "warp-images: frame %d into keyframe %d, %d x %d\n", last_frame, last_kf, wi.cols, wi.rows);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    return 0;
}
