// pose_graph_slam.cpp -- keyframe SLAM end to end on the library, the loop of the reference's SLAM/KFsphere_SLAM.cpp: the keyframe loop
// of keyframe_odometry.cpp (the keyframe is the TARGET of every alignment, a frame whose avDepthResidual fails the threshold becomes the
// next keyframe), extended by the three steps the reference does in g2o and PCL:
//   1 every new keyframe is a vertex; the alignment against its predecessor is an odometry edge, and ONE store.align round of the new
//     keyframe against the earlier keyframes within a radius gives the closure edges (KFsphere_SLAM.cpp:262-265, 542-550, 630): the relative
//     pose is the edge, the Hessian of the alignment its information matrix;
//     with a minimum overlap score (8th argument) the keyframes within the radius are first ranked and cut by their sensed-space overlap
//     with the new keyframe at the current graph poses (FrameStore::overlapMatrix at the coarsest level + overlapCandidates; the
//     reference scores connections by the SSO of a finished alignment, LoopClosure360.h:321, 360), so that alignments are only spent
//     on pairs that share space;
//     with radius sigmas k (10th argument) the radius grows with what the graph knows about the pair: one relativeCovariances call of all
//     earlier keyframes against the new one gives C_ab, and a keyframe is a candidate when |t_ab| <= radius + k sigma_t with
//     sigma_t = sqrt(variance_factor * lambda_max(translation block of C_ab)) -- after a long odometry chain the new keyframe's pose relative
//     to the old ones has drifted, which is exactly when a fixed radius around the current estimate misses the closure;
//   2 optimizeGraph() (KFsphere_SLAM.cpp:679-689) on the device (rgbd360/PoseGraph.hpp);
//     with a robust delta (9th argument) every closure edge gets a Cauchy kernel of that delta (g2o's setRobustKernel; the odometry edges
//     stay quadratic), closures whose weight ends below 0.1 are switched off and the graph is optimised once more, so that an alignment
//     that converged on the wrong surface is not baked into the map (delta is in units of sqrt(r^T Omega r).  With the alignment's
//     Hessian as Omega that is a large number even for a good closure: on the synthetic ring of tools/dump_sequence.py s is in the
//     thousands, and delta = 6 switches every closure off; choose delta from the `weight` lines of a first run);
//   3 GlobalMap::move for every keyframe whose pose changed: the map follows the optimised poses without being rebuilt.
//
// Frames: raw files written by tools/dump_sequence.py, frame_%03d.rgb (H*W*3 uint8), frame_%03d.depth (H*W uint16 mm).
// Build:  g++ -std=c++17 -O2 -Iinclude examples/pose_graph_slam.cpp -Lrgbd360_amd/lib -lrgbd360_hip
//             -Wl,-rpath,$PWD/rgbd360_amd/lib -o pose_graph_slam
// Usage:  pose_graph_slam <dir> <n_frames> <width> <height> [max avDepthResidual = 0.9] [closure radius in m = 1.0] [closures per keyframe = 3]
//         [minimum overlap score = 0: the radius rule alone] [robust delta = 0: quadratic closures] [radius sigmas = 0: the fixed radius]
// Prints  keyframe <frame> vertex <v> status <s> pose <16 floats, column-major, world <- keyframe, before any optimisation>
//         uncertainty <a> <b> <sigma_t in m>   (only with radius sigmas: every earlier keyframe a against the new keyframe b)
//         candidate <a> <b> score <x>          (only with a minimum overlap score)
//         closure <from> <to> status <s>
//         weight <from> <to> <w>               (only with a robust delta: every closure after each optimisation, 0 for one switched off)
//         rejected <from> <to>                 (only with a robust delta: a closure switched off now)
//         optimise status <s> iterations <i> chi2 <before> <after> moved <keyframes re-posed in the map>
//         graph vertices <V> edges <E> status <s of the last optimisation> voxels <map size>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "rgbd360/FrameStore.hpp"
#include "rgbd360/GlobalMap.hpp"
#include "rgbd360/PoseGraph.hpp"

using rgbd360::Mat4f;

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

static Mat4f mul(const Mat4f& A, const Mat4f& B) {
    Mat4f C{};
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += (double)A(r, k) * (double)B(k, c);
            C(r, c) = (float)s;
        }
    return C;
}

static Mat4f rigidInverse(const Mat4f& T) {
    Mat4f I = Mat4f::Identity();
    for (int r = 0; r < 3; ++r) {
        double s = 0.0;
        for (int c = 0; c < 3; ++c) {
            I(r, c) = T(c, r);
            s -= (double)T(c, r) * (double)T(c, 3);
        }
        I(r, 3) = (float)s;
    }
    return I;
}

static double distance(const Mat4f& A, const Mat4f& B) {
    double s = 0.0;
    for (int r = 0; r < 3; ++r) s += ((double)A(r, 3) - B(r, 3)) * ((double)A(r, 3) - B(r, 3));
    return std::sqrt(s);
}

// the largest eigenvalue of the symmetric 3x3 translation block of a covariance (cyclic Jacobi rotations)
static double largestTranslationVariance(const rgbd360::PoseGraph::Mat6d& C) {
    double A[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A[r][c] = C(r, c);
    for (int sweep = 0; sweep < 16; ++sweep)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double th = 0.5 * std::atan2(2.0 * A[p][q], A[q][q] - A[p][p]), c = std::cos(th), s = std::sin(th);
                for (int k = 0; k < 3; ++k) {      // A <- A G, then A <- G^T A
                    const double a = A[k][p], b = A[k][q];
                    A[k][p] = c * a - s * b;
                    A[k][q] = s * a + c * b;
                }
                for (int k = 0; k < 3; ++k) {
                    const double a = A[p][k], b = A[q][k];
                    A[p][k] = c * a - s * b;
                    A[q][k] = s * a + c * b;
                }
            }
    return std::max(A[0][0], std::max(A[1][1], A[2][2]));
}

struct KeyFrame {
    int frame;
    std::unique_ptr<Frame> images;      // kept: the map is re-posed from them
    Mat4f pose;                         // world <- keyframe, as the map holds it
};

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s <dir> <n_frames> <width> <height> [max avDepthResidual] [closure radius] [closures per keyframe] [min overlap score] [robust delta] [radius sigmas]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int n = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]);
    const double max_residual = argc > 5 ? atof(argv[5]) : 0.9;
    const double radius = argc > 6 ? atof(argv[6]) : 1.0;
    const int max_closures = argc > 7 ? atoi(argv[7]) : 3;
    const double min_overlap = argc > 8 ? atof(argv[8]) : 0.0;
    const double robust_delta = argc > 9 ? atof(argv[9]) : 0.0;
    const double radius_sigmas = argc > 10 ? atof(argv[10]) : 0.0;
    if (n < 1 || n > 4096 || max_closures < 0 || !(robust_delta >= 0.0) || !(radius_sigmas >= 0.0)) return 2;
    try {
        rgbd360::RegisterPhotoICP align360;
        align360.setNumPyr(4);
        align360.useSaliency(false);
        rgbd360::FrameStore store(align360, n, h, w);      // entry v holds keyframe v; the entry behind the last keyframe holds the current frame
        rgbd360::GlobalMap globalMap(align360, rgbd360::FilterPointCloud(), 1 << 20);
        rgbd360::PoseGraph graph(align360);
        std::vector<KeyFrame> keyframes;
        struct Closure { int edge, from, to; bool rejected; };
        std::vector<Closure> closure_edges;      // (only filled with a robust delta)
        int last_status = 0;

        auto add_keyframe = [&](int frame, std::unique_ptr<Frame> images, const Mat4f& pose, int status) {
            const int v = graph.addVertex(pose);
            printf("keyframe %d vertex %d status %d pose", frame, v, status);
            for (int k = 0; k < 16; ++k) printf(" %.9g", pose.m[k]);
            printf("\n");
            globalMap.insert(images->sphereRGB, images->sphereDepth, pose);
            keyframes.push_back({frame, std::move(images), pose});
            return v;
        };

        std::unique_ptr<Frame> first(new Frame);
        if (!first->load(dir, 0, w, h)) return 3;
        store.put(0, first->sphereRGB, first->sphereDepth);
        add_keyframe(0, std::move(first), Mat4f::Identity(), 0);
        Mat4f guess = Mat4f::Identity();      // the last frame in the current keyframe
        for (int f = 1; f < n; ++f) {
            std::unique_ptr<Frame> cur(new Frame);
            if (!cur->load(dir, f, w, h)) return 3;
            const int kf = (int)keyframes.size() - 1, entry = kf + 1;
            store.put(entry, cur->sphereRGB, cur->sphereDepth);
            std::vector<rgbd360_result> res;
            const std::vector<Mat4f> rel = store.align({{kf, entry}}, {guess}, RGBD360_PHOTO_DEPTH, 32, &res);
            if (res[0].status == 0 && res[0].rms_depth < max_residual) {      // "skip frame": the keyframe stays, the entry is reused
                guess = rel[0];
                continue;
            }
            // step 1: the frame becomes keyframe `entry`; odometry edge from its predecessor
            const Mat4f in_kf = res[0].status == 0 ? rel[0] : guess;
            const int v = add_keyframe(f, std::move(cur), mul(keyframes[kf].pose, in_kf), res[0].status);
            if (res[0].status == 0) graph.addEdge(kf, v, rel[0], rgbd360::PoseGraph::information(res[0]));
            guess = Mat4f::Identity();
            // ... and one round against the nearest earlier keyframes within the radius, each from the pose the graph gives it now
            std::vector<std::pair<double, int>> near;
            std::vector<double> slack(kf > 0 ? kf : 0, 0.0);      // per earlier keyframe: radius sigmas x the 1-sigma translation uncertainty of the pair
            if (radius_sigmas > 0.0 && kf > 0) {
                std::vector<int> from(kf), to(kf, v);
                for (int u = 0; u < kf; ++u) from[u] = u;
                const std::vector<rgbd360::PoseGraph::Mat6d> C = graph.relativeCovariances(from, to);      // (all zeros when the call is ill-posed)
                for (int u = 0; u < kf; ++u) {
                    const double var = graph.covResult().variance_factor * largestTranslationVariance(C[u]);
                    const double sigma_t = var > 0.0 ? std::sqrt(var) : 0.0;
                    printf("uncertainty %d %d %.6g\n", u, v, sigma_t);
                    slack[u] = radius_sigmas * sigma_t;
                }
            }
            for (int u = 0; u < kf; ++u) {
                const double d = distance(keyframes[u].pose, keyframes[v].pose);
                if (d <= radius + slack[u]) near.push_back({d, u});
            }
            std::sort(near.begin(), near.end());
            if (min_overlap > 0.0 && !near.empty()) {      // rank and cut by overlap instead of by distance
                std::vector<int> entries;
                std::vector<Mat4f> world;
                for (const auto& c : near) entries.push_back(c.second);
                std::sort(entries.begin(), entries.end());
                entries.push_back(v);                      // the new keyframe last: it is the `b` of every candidate wanted here
                for (int e : entries) world.push_back(keyframes[e].pose);
                const rgbd360_overlap_params op = store.overlapDefaultParams();
                const rgbd360::OverlapMatrix M = store.overlapMatrix(entries, world, 0.f, op);
                const int level_px = (h >> op.level) * (w >> op.level);
                near.clear();
                for (const rgbd360::OverlapCandidate& c : rgbd360::overlapCandidates(M.records, M.n, level_px, (float)min_overlap, 1, max_closures, {})) {
                    if (c.b != M.n - 1) continue;          // pairs among the old keyframes are not this round's business
                    printf("candidate %d %d score %.6f\n", entries[c.a], v, c.score);
                    near.push_back({-(double)c.score, entries[c.a]});
                }
            }
            if ((int)near.size() > max_closures) near.resize(max_closures);
            std::vector<rgbd360::FrameStore::Pair> pairs;
            std::vector<Mat4f> guesses;
            for (const auto& c : near) {
                pairs.push_back({c.second, v});
                guesses.push_back(mul(rigidInverse(keyframes[c.second].pose), keyframes[v].pose));
            }
            const std::vector<Mat4f> closures = store.align(pairs, guesses, RGBD360_PHOTO_DEPTH, 32, &res);
            int added = 0;
            for (size_t k = 0; k < pairs.size(); ++k) {
                printf("closure %d %d status %d\n", pairs[k].target, pairs[k].source, res[k].status);
                if (res[k].status != 0) continue;
                graph.addEdge(pairs[k].target, pairs[k].source, closures[k], rgbd360::PoseGraph::information(res[k]));
                if (robust_delta > 0.0) {
                    graph.setRobustKernel(graph.lastEdge(), RGBD360_GRAPH_ROBUST_CAUCHY, robust_delta);
                    closure_edges.push_back({graph.lastEdge(), pairs[k].target, pairs[k].source, false});
                }
                ++added;
            }
            if (!added) continue;
            // step 2: optimise; step 3: re-pose the map
            const double before = graph.chi2();
            graph.optimizeGraph();
            if (robust_delta > 0.0) {
                std::vector<double> weights;
                graph.edgeWeights(weights);
                int rejected = 0;
                for (Closure& c : closure_edges) printf("weight %d %d %.6f\n", c.from, c.to, weights[c.edge]);
                for (Closure& c : closure_edges) {
                    if (c.rejected || !(weights[c.edge] < 0.1)) continue;
                    graph.setEdgeEnabled(c.edge, false);
                    c.rejected = true;
                    ++rejected;
                    printf("rejected %d %d\n", c.from, c.to);
                }
                if (rejected) graph.optimizeGraph();
            }
            last_status = graph.result().status;
            std::vector<Mat4f> poses;
            graph.getPoses(poses);
            int moved = 0;
            for (size_t u = 0; u < keyframes.size(); ++u) {
                if (!memcmp(poses[u].m, keyframes[u].pose.m, sizeof(poses[u].m))) continue;
                globalMap.move(keyframes[u].images->sphereRGB, keyframes[u].images->sphereDepth, keyframes[u].pose, poses[u]);
                keyframes[u].pose = poses[u];
                ++moved;
            }
            printf("optimise status %d iterations %d chi2 %.9g %.9g moved %d\n", last_status, graph.result().iterations, before,
                   graph.result().chi2_final, moved);
        }
        printf("graph vertices %d edges %d status %d voxels %lld\n", graph.numVertices(), graph.numEdges(), last_status, globalMap.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    return 0;
}
