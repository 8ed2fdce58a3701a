// odometry_replay.cpp -- replays the call sequence of Registration/OdometryRGBD360.cpp:141-297 of the reference
// (per frame: set target / set source / alignFrames360(PHOTO_DEPTH) / accumulate currentPose) through the C++
// adapter, on frames read from raw files written by tools/dump_sequence.py:
//     frame_%03d.rgb  (H*W*3 uint8)   frame_%03d.depth (H*W uint16 mm)
// Build:  g++ -std=c++17 -O2 -Iinclude examples/odometry_replay.cpp -Lrgbd360_amd/lib -lrgbd360_hip
//             -Wl,-rpath,$PWD/rgbd360_amd/lib -o odometry_replay
// Usage:  odometry_replay <dir> <n_frames> <width> <height> [--sequence | --multi <n_gpus> | --pbmap | --link] [--map FILE [--leaf L] [--refine-on-map | --refine-on-map-plane | --refine-on-map-colour | --refine-on-map-c2f SHIFT [--plane]] [--map-robust KIND DELTA] [--render-map PREFIX] [--raycast-map PREFIX] [--map-normals OUT] [--raycast-surface PREFIX] [--map-planes OUT] [--map-window N | --carve]]
//         --sequence: all frames are loaded first and the frame loop runs inside the library (alignSequence)
//         --multi N:  the same sequence sharded over N GPUs of this node from this one process (rgbd360_multi_*: one host thread
//                     per device, contiguous shards of pairs, one ncclAllGather of the solved poses over xGMI); prints the
//                     lines of --sequence
//         --pbmap:    every pair is first registered from its planes (RegisterRGBD360::RegisterPbMap, ODOMETRY_6DoF, as
//                     SphereGraphSLAM.cpp:180 / KFsphere_SLAM.cpp:314 do) and that pose seeds alignFrames360
//                     (KFsphere_SLAM.cpp:149); prints one extra "pbmap" line per pair
//         --link:     the same per pair through the one-call form rgbd360::RegisterFrames (planes, RegisterPbMap, seeded dense
//                     alignment, the reference's isApprox(1e-1) validity test); prints "link <pair> <ok> rel_t ..."
//         --map FILE: (frame loop and --pbmap only; ignored with a warning otherwise) the global map of OdometryRGBD360.cpp:242-268
//                     -- every frame is inserted at currentPose into a resident voxel grid (rgbd360::GlobalMap: filterEuclidean's box, transformPointCloud, globalMap +=,
//                     filterVoxel) and the map is written to FILE as "x y z r g b count" lines; --leaf L: the voxel size (0.05 m)
//         --refine-on-map: (with --map) before a frame is inserted its pose is refined against the map by point-to-point ICP
//                     (GlobalMap::alignSphere; the cloud ICP of OdometryRGBD360.cpp:98-114, 210-222 with the map as its target): a
//                     correction against everything seen so far.  An accepted refinement (status 0) replaces currentPose; prints one
//                     extra "refine" line per frame.  Without the option the output is what it was.
//         --refine-on-map-plane: the same with the point-to-plane form (GlobalMap::alignSpherePlane: the plane cost of the GICP those call
//                     sites use); prints one "refine-plane" line per frame with the contributing points, the unsupported and nonplanar
//                     ones and both fitness values.  Takes precedence over --refine-on-map.
//         --refine-on-map-colour: the same with coloured ICP (GlobalMap::alignSphereColour: point-to-plane on the map's normals plus a photometric
//                     term on its intensity gradients, which holds the pose along a corridor or a floor); one line per frame "refine-colour ..."
//                     with the dropped and zero-gradient counts and both rms values.  Takes precedence over the two above.
//         --refine-on-map-c2f SHIFT [--plane]: the same through the map pyramid (GlobalMap::alignSphereCoarseToFine): the ICP runs on the maps of
//                     leaf * 2^SHIFT .. leaf, merged out of the resident table, each level from the pose of the one before -- a capture range of
//                     2^SHIFT leaves where the two options above have one; --plane: the point-to-plane form on every level.  Prints one
//                     "refine-c2f" line per frame and one "  level" line per level.  Takes precedence over both.
//         --map-robust KIND DELTA: (with a refine option) the robust kernel of whichever method refines (GlobalMap::setAlignRobust): KIND huber,
//                     cauchy or geman_mcclure, DELTA in metres (the colour method: in the units of the square root of its joint cost); one
//                     extra "  robust" line per frame with sum w, the contributing points and those with w < 1 (GlobalMap::robustInfo).
//         --render-map PREFIX: (needs --map) after the replay the map is rendered as a spherical frame of the input's size at the last
//                     pose (GlobalMap::renderSphere: the reference's viewer.globalMap, OdometryRGBD360.cpp:242-268, as a panorama) and
//                     written as PREFIX_rgb.ppm (P6) and PREFIX_depth.pfm (Pf, metres, 0 in holes, rows bottom to top); prints one
//                     "render" line with the counters.
//         --raycast-map PREFIX: (needs --map) the same two images by ray casting through the map (GlobalMap::raycastSphere: per pixel the
//                     first occupied voxel along the pixel's ray); prints one "raycast" line with the counters.
//         --map-normals OUT: (needs --map) the map as an oriented cloud, one line "x y z nx ny nz curvature status" per voxel
//                     (GlobalMap::normals: a normal per voxel fitted to the centroids around it, facing the last pose; status RGBD360_NORMAL_*).
//         --raycast-surface PREFIX: (needs --map) the ray-cast panorama with the surface (GlobalMap::raycastSurfaceSphere): the depth on the
//                     plane fitted around each hit voxel and PREFIX_normal.pfm, the world-frame normal per pixel.
//         --map-planes OUT: (needs --map) the map's planar regions (GlobalMap::planes: connected voxels of like normals, the plane set a lost
//                     frame is registered against, GlobalMap::relocalize), one line "ix iy iz N P cx cy cz nx ny nz d area curvature" per plane
//                     by root key: the root voxel's key, the voxels and points of the region, its centroid, normal, offset, hull area and
//                     curvature; prints one "planes" line with the counters.
//         --map-window N: (needs --map) a bounded local map, the usual odometry target: the loop keeps the images and poses of the last N
//                     frames, and when frame k goes in, frame k - N leaves (GlobalMap::remove: the integer sums make that exact).  The
//                     table is rebuilt (GlobalMap::rehash) when a census shows more tombstones than occupied voxels.  Prints one "window"
//                     line per inserted frame: the frame, the occupied voxels and tombstones after it, the voxels its removal emptied,
//                     whether the table was rebuilt, and the pose the frame went in at (16 hexadecimal floats, column-major: exact, so
//                     that a reader can rebuild the window's map bit for bit).  Without the option the output is what it was.
//         --carve: (needs --map, not with --map-window) after each insert the same frame observes the map (GlobalMap::observe: every pixel
//                     is a line of sight) and the voxels it looks straight through and does not measure are erased (GlobalMap::carve): what
//                     an earlier frame left in space that this one sees to be free.  Prints one "carve" line per inserted frame with the
//                     votes given and the voxels and points erased.  A lossy edit, hence not with the window, whose removals are exact.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "rgbd360/GlobalMap.hpp"
#include "rgbd360/RegisterPhotoICP.hpp"
#include "rgbd360/RegisterRGBD360.hpp"

struct Frame {   // the two members of Frame360 the dense path reads (Frame360.h:104-111)
    std::vector<uint8_t> rgb;
    std::vector<uint16_t> depth;
    int rows, cols;
    rgbd360::ImageView sphereRGB, sphereDepth;
    bool load(const std::string& dir, int k, int w, int h) {
        rows = h; cols = w;
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

static rgbd360::Mat4f mul(const rgbd360::Mat4f& A, const rgbd360::Mat4f& B) {
    rgbd360::Mat4f C{};
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            float s = 0;
            for (int k = 0; k < 4; ++k) s += A(r, k) * B(k, c);
            C(r, c) = s;
        }
    return C;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s <dir> <n_frames> <width> <height> [--sequence | --pbmap]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int n = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]);
    rgbd360::RegisterPhotoICP align360;      // OdometryRGBD360.cpp:91-95
    align360.setNumPyr(4);
    align360.useSaliency(false);
    rgbd360::Mat4f currentPose = rgbd360::Mat4f::Identity();
    if (argc > 5) {      // only the frame loop below builds the map
        const std::string mode = argv[5];
        if (mode == "--sequence" || mode == "--multi" || mode == "--link")
            for (int a = 6; a < argc; ++a)
                if (std::string(argv[a]) == "--map") fprintf(stderr, "warning: --map is ignored with %s\n", mode.c_str());
    }
    if (argc > 5 && std::string(argv[5]) == "--sequence") {
        std::vector<Frame> frames(n);
        std::vector<rgbd360::ImageView> rgb, depth;
        for (int k = 0; k < n; ++k) {
            if (!frames[k].load(dir, k, w, h)) return 3;
            rgb.push_back(frames[k].sphereRGB);
            depth.push_back(frames[k].sphereDepth);
        }
        std::vector<rgbd360_result> res;
        const std::vector<rgbd360::Mat4f> rels = align360.alignSequence(rgb, depth, rgbd360::RegisterPhotoICP::PHOTO_DEPTH, 0, 3,
                                                                        rgbd360::Mat4f::Identity(), &res);
        for (size_t j = 0; j < rels.size(); ++j) {
            currentPose = mul(currentPose, rels[j]);
            printf("pair %zu status %d sso %.4f rel_t %.5f %.5f %.5f pose_t %.5f %.5f %.5f\n", j, res[j].status, res[j].sso,
                   rels[j](0, 3), rels[j](1, 3), rels[j](2, 3), currentPose(0, 3), currentPose(1, 3), currentPose(2, 3));
        }
        return 0;
    }
    if (argc > 6 && std::string(argv[5]) == "--multi") {
        const int n_gpus = atoi(argv[6]);
        std::vector<Frame> frames(n);
        std::vector<const uint8_t*> rgb(n);
        std::vector<const void*> depth(n);
        for (int k = 0; k < n; ++k) {
            if (!frames[k].load(dir, k, w, h)) return 3;
            rgb[k] = frames[k].rgb.data();
            depth[k] = frames[k].depth.data();
        }
        rgbd360_params p;
        rgbd360_default_params(&p);
        p.n_pyr = 4;
        rgbd360_multi* m = nullptr;
        int rc = rgbd360_multi_create(&p, n_gpus, nullptr, &m);
        if (rc != 0) {
            fprintf(stderr, "rgbd360_multi_create(%d GPUs) failed: %d\n", n_gpus, rc);
            return 4;
        }
        std::vector<float> poses((size_t)(n - 1) * 16);
        std::vector<rgbd360_result> res(n - 1);
        rc = rgbd360_multi_align_sequence(m, n, rgb.data(), (size_t)w * 3, depth.data(), (size_t)w * 2, 0, h, w, nullptr, 2, 0, 3, poses.data(),
                                          res.data());
        if (rc != 0) {
            fprintf(stderr, "rgbd360_multi_align_sequence: %s (%d)\n", rgbd360_multi_last_error(m), rc);
            rgbd360_multi_destroy(m);
            return 5;
        }
        for (int j = 0; j + 1 < n; ++j) {
            rgbd360::Mat4f rel{};
            for (int k = 0; k < 16; ++k) rel.m[k] = poses[(size_t)j * 16 + k];
            currentPose = mul(currentPose, rel);                                                // OdometryRGBD360.cpp:257
            printf("pair %d status %d sso %.4f rel_t %.5f %.5f %.5f pose_t %.5f %.5f %.5f\n", j, res[j].status, res[j].sso, rel(0, 3), rel(1, 3),
                   rel(2, 3), currentPose(0, 3), currentPose(1, 3), currentPose(2, 3));
        }
        rgbd360_multi_destroy(m);
        return 0;
    }
    if (argc > 5 && std::string(argv[5]) == "--link") {
        rgbd360::RegisterRGBD360 registerer(/*odometry_config=*/true);
        rgbd360::SegmentParams seg;
        seg.max_depth_change_factor = 0.05f;
        seg.min_inliers = 40;
        seg.angular_threshold = 0.03f;
        seg.distance_threshold = 0.05f;
        Frame a, b;
        if (!a.load(dir, 0, w, h)) return 3;
        for (int k = 1; k < n; ++k) {
            if (!b.load(dir, k, w, h)) return 3;
            rgbd360::Mat4f rel = rgbd360::Mat4f::Identity();
            const bool ok = rgbd360::RegisterFrames(a, b, rel, [](const rgbd360::ImageView& v) { return v; }, align360, registerer,
                                                    rgbd360::RegisterRGBD360::ODOMETRY_6DoF, 25, seg);
            printf("link %d ok %d matched %zu rel_t %.5f %.5f %.5f\n", k - 1, ok ? 1 : 0, registerer.getMatchedPlanes().size(), rel(0, 3),
                   rel(1, 3), rel(2, 3));
            std::swap(a, b);
        }
        return 0;
    }
    const bool use_pbmap = argc > 5 && std::string(argv[5]) == "--pbmap";
    std::string map_file, render_prefix, raycast_prefix, normals_file, surface_prefix, planes_file;
    float leaf = 0.05f;
    bool refine_on_map = false, refine_on_map_plane = false, refine_on_map_colour = false, c2f_plane = false;
    int c2f_shift = -1;
    int robust_kind = RGBD360_MAP_ROBUST_NONE;
    double robust_delta = 0.0;
    int map_window = 0;
    bool carve = false;
    for (int a = 5; a < argc; ++a) {
        if (std::string(argv[a]) == "--carve") carve = true;
        if (a + 1 < argc && std::string(argv[a]) == "--map") map_file = argv[a + 1];
        if (a + 1 < argc && std::string(argv[a]) == "--leaf") leaf = (float)atof(argv[a + 1]);
        if (a + 1 < argc && std::string(argv[a]) == "--render-map") render_prefix = argv[a + 1];
        if (a + 1 < argc && std::string(argv[a]) == "--raycast-map") raycast_prefix = argv[a + 1];
        if (a + 1 < argc && std::string(argv[a]) == "--map-window") map_window = atoi(argv[a + 1]);
        if (a + 1 < argc && std::string(argv[a]) == "--map-normals") normals_file = argv[a + 1];
        if (a + 1 < argc && std::string(argv[a]) == "--raycast-surface") surface_prefix = argv[a + 1];
        if (a + 1 < argc && std::string(argv[a]) == "--map-planes") planes_file = argv[a + 1];
        if (std::string(argv[a]) == "--refine-on-map") refine_on_map = true;
        if (std::string(argv[a]) == "--refine-on-map-plane") refine_on_map_plane = true;
        if (std::string(argv[a]) == "--refine-on-map-colour") refine_on_map_colour = true;
        if (a + 1 < argc && std::string(argv[a]) == "--refine-on-map-c2f") c2f_shift = atoi(argv[a + 1]);
        if (std::string(argv[a]) == "--plane") c2f_plane = true;
        if (a + 2 < argc && std::string(argv[a]) == "--map-robust") {
            const std::string kind = argv[a + 1];
            robust_kind = kind == "huber" ? RGBD360_MAP_ROBUST_HUBER : kind == "cauchy" ? RGBD360_MAP_ROBUST_CAUCHY
                        : kind == "geman_mcclure" ? RGBD360_MAP_ROBUST_GEMAN_MCCLURE : -1;
            robust_delta = atof(argv[a + 2]);
        }
    }
    if (robust_kind < 0 || (robust_kind != RGBD360_MAP_ROBUST_NONE && (map_file.empty() || !(robust_delta > 0.0)))) {
        fprintf(stderr, "--map-robust needs --map, a kind (huber, cauchy, geman_mcclure) and a positive delta\n");
        return 2;
    }
    if (!render_prefix.empty() && map_file.empty()) {
        fprintf(stderr, "--render-map needs --map\n");
        return 2;
    }
    if (!raycast_prefix.empty() && map_file.empty()) {
        fprintf(stderr, "--raycast-map needs --map\n");
        return 2;
    }
    if ((!normals_file.empty() || !surface_prefix.empty()) && map_file.empty()) {
        fprintf(stderr, "--map-normals and --raycast-surface need --map\n");
        return 2;
    }
    if (!planes_file.empty() && map_file.empty()) {
        fprintf(stderr, "--map-planes: need --map\n");
        return 2;
    }
    if (map_window != 0 && (map_file.empty() || map_window < 0)) {
        fprintf(stderr, "--map-window needs --map and a positive number of frames\n");
        return 2;
    }
    if (carve && (map_file.empty() || map_window != 0)) {
        fprintf(stderr, "--carve needs --map and does not go with --map-window\n");
        return 2;
    }
    std::unique_ptr<rgbd360::GlobalMap> globalMap;      // declared behind align360: destroyed before its context
    struct Kept {        // a frame of the window: what its removal needs
        std::vector<uint8_t> rgb;
        std::vector<uint16_t> depth;
        rgbd360::Mat4f pose;
    };
    std::deque<Kept> window;
    int n_inserted = 0;
    auto add_to_map = [&](const Frame& f) {                                                      // :242, 266-268
        if (!globalMap->insert(f.sphereRGB, f.sphereDepth, currentPose, /*convention=*/0))
            fprintf(stderr, "map full: %lld points dropped\n", globalMap->stats().n_dropped_full);
        const int k = n_inserted++;
        if (carve) {      // the frame just inserted protects what it measures (end-votes) and erases what it looks through
            globalMap->observe(f.sphereDepth, currentPose, /*convention=*/0);
            const rgbd360_map_observe_stats& o = globalMap->observeStats();
            globalMap->carve();
            const rgbd360_map_carve_stats& c = globalMap->carveStats();
            printf("carve %d rays %lld through %lld end %lld voted %lld carved %lld points %lld protected %lld live %lld\n", k, o.n_valid, o.n_through, o.n_end,
                   c.n_voted, c.n_voxels_carved, c.n_points_carved, c.n_protected_end, c.n_voxels);
        }
        if (map_window == 0) return;
        window.push_back({f.rgb, f.depth, currentPose});
        long long emptied = 0;
        if ((int)window.size() > map_window) {      // frame k - N leaves as it came
            const Kept& old = window.front();
            const rgbd360::ImageView rgb = {old.rgb.data(), f.rows, f.cols, (size_t)f.cols * 3, rgbd360::ImageView::U8C3};
            const rgbd360::ImageView depth = {old.depth.data(), f.rows, f.cols, (size_t)f.cols * 2, rgbd360::ImageView::U16C1};
            if (!globalMap->remove(rgb, depth, old.pose, /*convention=*/0))
                fprintf(stderr, "map mismatch: %lld points missing, %lld refused\n", globalMap->editStats().n_missing, globalMap->editStats().n_underflow);
            emptied = globalMap->editStats().n_voxels_emptied;
            window.pop_front();
        }
        rgbd360_map_census_counts c = globalMap->census();
        const bool rebuild = c.n_tombstones > c.n_live;
        if (rebuild && globalMap->rehash()) c = globalMap->census();
        printf("window %d live %lld tombstones %lld emptied %lld rehashed %d pose", k, c.n_live, c.n_tombstones, emptied, rebuild ? 1 : 0);
        for (int q = 0; q < 16; ++q) printf(" %a", currentPose.m[q]);
        printf("\n");
    };
    rgbd360::RegisterRGBD360 registerer(/*odometry_config=*/true);
    rgbd360::SegmentParams seg;
    seg.max_depth_change_factor = 0.05f;        // the synthetic frames are full spheres: Frame360_stereo.h:854-882 set-up
    seg.min_inliers = 40;
    seg.angular_threshold = 0.03f;
    seg.distance_threshold = 0.05f;
    std::vector<rgbd360_plane> planes1, planes2;
    Frame frame1, frame2;
    if (!frame1.load(dir, 0, w, h)) return 3;
    if (use_pbmap) planes1 = rgbd360::segmentPlanes(align360, frame1.sphereDepth, seg);
    if (!map_file.empty()) {
        globalMap.reset(new rgbd360::GlobalMap(align360, rgbd360::FilterPointCloud(leaf)));
        if (robust_kind != RGBD360_MAP_ROBUST_NONE) {       // of the method that refines
            const int method = c2f_shift >= 0 ? (c2f_plane ? RGBD360_MAP_METHOD_PLANE : RGBD360_MAP_METHOD_POINT)
                             : refine_on_map_colour ? RGBD360_MAP_METHOD_COLOUR : refine_on_map_plane ? RGBD360_MAP_METHOD_PLANE : RGBD360_MAP_METHOD_POINT;
            globalMap->setAlignRobust(method, robust_kind, robust_delta);
        }
        add_to_map(frame1);                                                                     // the first frame, at the identity
    }
    for (int k = 1; k < n; ++k) {
        if (!frame2.load(dir, k, w, h)) return 3;
        rgbd360::Mat4f guess = rgbd360::Mat4f::Identity();
        if (use_pbmap) {
            planes2 = rgbd360::segmentPlanes(align360, frame2.sphereDepth, seg);
            rgbd360::PlaneList ref{planes1.data(), (int)planes1.size()}, trg{planes2.data(), (int)planes2.size()};
            const bool good = registerer.RegisterPbMap(&ref, &trg, 25, rgbd360::RegisterRGBD360::ODOMETRY_6DoF);
            if (good) guess = registerer.getPose();
            printf("pbmap %d good %d matched %zu t %.5f %.5f %.5f\n", k - 1, good ? 1 : 0, registerer.getMatchedPlanes().size(), guess(0, 3),
                   guess(1, 3), guess(2, 3));
        }
        if (k == 1) align360.setTargetFrame(frame1.sphereRGB, frame1.sphereDepth);              // :189
        else align360.promoteSourceToTarget();          // frame1 is last step's frame2: already on the device
        align360.setSourceFrame(frame2.sphereRGB, frame2.sphereDepth);                          // :190
        align360.alignFrames360(guess, rgbd360::RegisterPhotoICP::PHOTO_DEPTH);                 // :192
        const rgbd360::Mat4f rel = align360.getOptimalPosePod();                                  // :193
        currentPose = mul(currentPose, rel);                                                    // :257
        printf("pair %d status %d sso %.4f rel_t %.5f %.5f %.5f pose_t %.5f %.5f %.5f\n", k - 1, align360.status(), align360.SSO,
               rel(0, 3), rel(1, 3), rel(2, 3), currentPose(0, 3), currentPose(1, 3), currentPose(2, 3));
        fprintf(stderr, "entropy %d %.5f\n", k - 1, align360.calcEntropy());                     // :207 (commented out in the source)
        if (globalMap && c2f_shift >= 0) {
            rgbd360::Mat4f refined = currentPose;
            rgbd360_map_c2f_params p = globalMap->c2fParams();
            p.top_shift = c2f_shift;
            p.kind = c2f_plane ? 1 : 0;
            const int status = globalMap->alignSphereCoarseToFine(frame2.sphereDepth, currentPose, refined, /*convention=*/0, &p);
            const rgbd360_map_c2f_result& r = globalMap->c2fResult();
            const rgbd360_map_c2f_level& last = r.levels[r.n_levels - 1];
            printf("refine-c2f %d status %d levels %d kind %d matched %lld fitness %.6f pose_t %.5f %.5f %.5f pyramid_bytes %zu\n", k - 1, status, r.n_levels,
                   p.kind, last.n_matched, last.fitness, refined(0, 3), refined(1, 3), refined(2, 3), globalMap->pyramidBytes());
            for (int l = 0; l < r.n_levels; ++l)
                printf("  level %d shift %d status %d iterations %d converged %d matched %lld fitness %.6f pose_t %.5f %.5f %.5f\n", k - 1, r.levels[l].shift,
                       r.levels[l].status, r.levels[l].iterations, r.levels[l].converged, r.levels[l].n_matched, r.levels[l].fitness, r.levels[l].pose[12],
                       r.levels[l].pose[13], r.levels[l].pose[14]);
            if (status == RGBD360_OK) currentPose = refined;
        } else if (globalMap && refine_on_map_colour) {
            rgbd360::Mat4f refined = currentPose;
            const int status = globalMap->alignSphereColour(frame2.sphereRGB, frame2.sphereDepth, currentPose, refined, /*convention=*/0);
            const rgbd360_map_align_colour_result& r = globalMap->alignColourResult();
            printf("refine-colour %d status %d iterations %d matched %lld fitness %.6g pose_t %.5f %.5f %.5f no_normal %lld no_gradient %lld rms_geometric %.6f "
                   "rms_colour %.6f\n",
                   k - 1, status, r.iterations, r.n_matched, r.fitness, refined(0, 3), refined(1, 3), refined(2, 3), r.n_no_normal, r.n_no_gradient,
                   r.rms_geometric, r.rms_colour);
            if (status == RGBD360_OK) currentPose = refined;
        } else if (globalMap && refine_on_map_plane) {
            rgbd360::Mat4f refined = currentPose;
            const int status = globalMap->alignSpherePlane(frame2.sphereDepth, currentPose, refined, /*convention=*/0);
            const rgbd360_map_align_plane_result& r = globalMap->alignPlaneResult();
            printf("refine-plane %d status %d iterations %d matched %lld fitness %.6f pose_t %.5f %.5f %.5f unsupported %lld nonplanar %lld fitness_point %.6f\n",
                   k - 1, status, r.iterations, r.n_matched, r.fitness, refined(0, 3), refined(1, 3), refined(2, 3), r.n_unsupported, r.n_nonplanar,
                   r.fitness_point);
            if (status == RGBD360_OK) currentPose = refined;
        } else if (globalMap && refine_on_map) {
            rgbd360::Mat4f refined = currentPose;
            const int status = globalMap->alignSphere(frame2.sphereDepth, currentPose, refined, /*convention=*/0);
            const rgbd360_map_align_result& r = globalMap->alignResult();
            printf("refine %d status %d iterations %d matched %lld fitness %.6f pose_t %.5f %.5f %.5f\n", k - 1, status, r.iterations, r.n_matched, r.fitness,
                   refined(0, 3), refined(1, 3), refined(2, 3));
            if (status == RGBD360_OK) currentPose = refined;
        }
        if (globalMap && robust_kind != RGBD360_MAP_ROBUST_NONE && (refine_on_map || refine_on_map_plane || refine_on_map_colour || c2f_shift >= 0)) {
            const rgbd360_map_robust_info ri = globalMap->robustInfo();
            printf("  robust %d method %d kind %d delta %.6g sum_w %.3f contributing %lld downweighted %lld\n", k - 1, ri.method, ri.kind, ri.delta_eff, ri.sum_w,
                   ri.n, ri.n_downweighted);
        }
        if (globalMap) add_to_map(frame2);
        std::swap(frame1, frame2);
        std::swap(planes1, planes2);
    }
    if (globalMap) {
        FILE* f = fopen(map_file.c_str(), "w");
        if (!f) return 6;
        for (const rgbd360::MapPoint& p : globalMap->points()) fprintf(f, "%.6f %.6f %.6f %d %d %d %d\n", p.x, p.y, p.z, p.r, p.g, p.b, p.count);
        fclose(f);
    }
    // a view of the map as PREFIX_rgb.ppm and PREFIX_depth.pfm; false: a file could not be written
    auto write_view = [&](const std::string& prefix, const std::vector<float>& depth, const std::vector<uint8_t>& rgb) {
        FILE* f = fopen((prefix + "_rgb.ppm").c_str(), "wb");
        if (!f) return false;
        fprintf(f, "P6\n%d %d\n255\n", w, h);
        fwrite(rgb.data(), 1, rgb.size(), f);
        fclose(f);
        f = fopen((prefix + "_depth.pfm").c_str(), "wb");
        if (!f) return false;
        fprintf(f, "Pf\n%d %d\n-1.0\n", w, h);            // little-endian floats, the bottom row first
        for (int r = h - 1; r >= 0; --r) fwrite(depth.data() + (size_t)r * w, sizeof(float), (size_t)w, f);
        fclose(f);
        return true;
    };
    if (globalMap && !render_prefix.empty()) {
        std::vector<float> depth;
        std::vector<uint8_t> rgb;
        globalMap->renderSphere(h, w, currentPose, depth, rgb);
        const rgbd360_map_render_stats& st = globalMap->renderStats();
        printf("render voxels %lld below_min_count %lld near %lld splatted %lld pixels_covered %lld\n", st.n_voxels, st.n_below_min_count, st.n_near,
               st.n_splatted, st.n_pixels_covered);
        if (!write_view(render_prefix, depth, rgb)) return 7;
    }
    if (globalMap && !raycast_prefix.empty()) {
        std::vector<float> depth;
        std::vector<uint8_t> rgb;
        globalMap->raycastSphere(h, w, currentPose, depth, rgb);
        const rgbd360_map_raycast_stats& st = globalMap->raycastStats();
        printf("raycast rays %lld hits %lld miss_box %lld left_box %lld t_max %lld max_steps %lld bad_rays %lld steps %lld lookups %lld\n", st.n_rays, st.n_hits,
               st.n_miss_box, st.n_left_box, st.n_t_max, st.n_max_steps, st.n_bad_rays, st.n_steps, st.n_lookups);
        if (!write_view(raycast_prefix, depth, rgb)) return 7;
    }
    if (globalMap && !normals_file.empty()) {      // the oriented cloud: the normals face the last pose
        std::vector<float> xyz, normal, curvature;
        std::vector<int32_t> status;
        const float viewpoint[3] = {currentPose(0, 3), currentPose(1, 3), currentPose(2, 3)};
        const long long nv = globalMap->normals(xyz, normal, &curvature, &status, nullptr, nullptr, viewpoint);
        const rgbd360_map_normal_stats& st = globalMap->normalStats();
        printf("normals voxels %lld below_min_count %lld unsupported %lld nonplanar %lld normals %lld\n", st.n_voxels, st.n_below_min_count, st.n_unsupported,
               st.n_nonplanar, st.n_normals);
        FILE* f = fopen(normals_file.c_str(), "w");
        if (!f) return 6;
        for (long long k = 0; k < nv; ++k)
            fprintf(f, "%.6f %.6f %.6f %.6f %.6f %.6f %.6g %d\n", xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2], normal[3 * k], normal[3 * k + 1], normal[3 * k + 2],
                    curvature[k], status[k]);
        fclose(f);
    }
    if (globalMap && !surface_prefix.empty()) {      // PREFIX_rgb.ppm, PREFIX_depth.pfm and PREFIX_normal.pfm (a colour PFM: x, y, z)
        std::vector<float> depth, normal;
        std::vector<uint8_t> rgb;
        globalMap->raycastSurfaceSphere(h, w, currentPose, depth, normal, rgb);
        const rgbd360_map_raycast_stats& st = globalMap->raycastStats();
        printf("raycast-surface rays %lld hits %lld on_plane %lld steps %lld lookups %lld\n", st.n_rays, st.n_hits, globalMap->onPlane(), st.n_steps,
               st.n_lookups);
        if (!write_view(surface_prefix, depth, rgb)) return 7;
        FILE* f = fopen((surface_prefix + "_normal.pfm").c_str(), "wb");
        if (!f) return 7;
        fprintf(f, "PF\n%d %d\n-1.0\n", w, h);
        for (int r = h - 1; r >= 0; --r) fwrite(normal.data() + (size_t)r * w * 3, sizeof(float), (size_t)w * 3, f);
        fclose(f);
    }
    if (globalMap && !planes_file.empty()) {      // the map's planar regions: what a lost frame is registered against (GlobalMap::relocalize)
        std::vector<int32_t> root_key3, key3, label_key3, plane_index;
        const std::vector<rgbd360_plane> planes = globalMap->planes(&root_key3);
        const rgbd360_map_plane_seg_stats st = globalMap->planeSegStats();
        globalMap->planeLabels(key3, label_key3, plane_index);
        std::vector<long long> n_voxels(planes.size(), 0);      // N of a plane: the voxels that carry its index
        for (const int32_t a : plane_index)
            if (a >= 0 && (size_t)a < n_voxels.size()) ++n_voxels[(size_t)a];
        printf("planes voxels %lld eligible %lld links %lld regions %lld available %lld planes %zu in_planes %lld\n", st.n_voxels, st.n_eligible, st.n_links,
               st.n_regions, st.n_planes_available, planes.size(), st.n_voxels_in_planes);
        FILE* f = fopen(planes_file.c_str(), "w");
        if (!f) return 6;
        for (size_t k = 0; k < planes.size(); ++k) {
            const rgbd360_plane& P = planes[k];
            fprintf(f, "%d %d %d %lld %d %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6g\n", root_key3[3 * k], root_key3[3 * k + 1], root_key3[3 * k + 2], n_voxels[k],
                    P.count, P.centroid[0], P.centroid[1], P.centroid[2], P.normal[0], P.normal[1], P.normal[2], P.d, P.area, P.curvature);
        }
        fclose(f);
    }
    return 0;
}
