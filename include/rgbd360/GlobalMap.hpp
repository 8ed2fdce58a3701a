// rgbd360/GlobalMap.hpp -- the global point-cloud map of the reference's odometry and SLAM programs as a resident voxel grid
// (rgbd360_map_*, ../rgbd360_hip.h).  Header-only, depends on the C ABI and on the PODs of RegisterPhotoICP.hpp; no Eigen, OpenCV
// or PCL.  What it replaces, per frame (OdometryRGBD360.cpp:242-268; OdometryKeyFrame360.cpp:316-343, SphereGraphSLAM.cpp:116-137,
// 193-209, KFsphere_SLAM.cpp:236, 558):
//     filter.filterEuclidean(frame->sphereCloud);                            FilterPointCloud.h:78-89
//     pcl::transformPointCloud(*frame->sphereCloud, *tc, currentPose);
//     *viewer.globalMap += *tc;
//     filter.filterVoxel(viewer.globalMap);                                  FilterPointCloud.h:92-99
// becomes   globalMap.insert(frame.sphereRGB, frame.sphereDepth, currentPose);   and   globalMap.points()   when the map is wanted.
// Two deliberate differences (rgbd360_hip.h): every inserted point has weight one -- the map is the voxel filter applied ONCE to the
// concatenation of all inserted clouds, where the reference's per-frame re-filter makes the order of the frames decide the result --
// and the sums are integers instead of PCL's float accumulators.
// The cloud ICP of the same programs (OdometryRGBD360.cpp:98-114, 210-222: filterVoxel, icp.setInputSource / setInputTarget / align(guess);
// RegisterPairRGBD360.cpp:111-118, MethodsRegisterRGBD360.cpp:294-320, OdometryKeyFrame360.cpp:124-140) with the map as its target:
//     globalMap.alignSphere(frame.sphereDepth, guess, pose)     point-to-point, nearest voxel centroid within max_dist <= leaf
//     globalMap.alignSpherePlane(frame.sphereDepth, guess, pose)   point-to-plane: the same match, the plane fitted to the centroids around it
//                                                                  (the call sites use pcl::GeneralizedIterativeClosestPoint, a plane cost)
//     globalMap.alignCloudGICP(xyz, normals, n, guess, pose)      generalized ICP (rgbd360_map_align_gicp_*): the same match weighted by the
//     globalMap.alignMapGICP(otherMap, guess, pose)               inverse of both sides' covariances -- the map's per-voxel normals and
//     globalMap.alignSphereGICP(frame.sphereDepth, guess, pose)   the source's normals, which may be another map's: "filterVoxel both, then GICP"
//     globalMap.alignSphereColour(frame.sphereRGB, frame.sphereDepth, guess, pose)   coloured ICP (rgbd360_map_align_colour_*): point-to-plane
//                                                                  on the map's normals plus a photometric term on its intensity gradients
//                                                                  (globalMap.colours), which holds the pose along a corridor or a floor
// All match within one voxel; a guess further off goes through the map pyramid (rgbd360_map_level, rgbd360_map_align_c2f_*: the maps of
// 2, 4, 8 .. times the voxel size are merged out of the table, exactly, and the ICP runs from the coarsest down),
//     globalMap.alignSphereCoarseToFine(frame.sphereDepth, guess, pose)     c2fResult().levels[k]: what each level did
// or starts from many guesses at once (rgbd360_map_align_batch_*: many clouds or guesses in lock step, each job the single call's bytes),
//     globalMap.alignBatchCloud(clouds, jobs, poses, results); GlobalMap::bestJob(results)     examples/map_multistart.cpp
// The rig's extrinsics, and optionally the rig poses of a window, against the map (rgbd360_map_calibrate_rig_*),
//     globalMap.calibrateRigDepth(depths, calib.K(), poses, extrinsics); GlobalMap::saveExtrinsics(extrinsics, dir)     examples/calibrate_extrinsics.cpp
// The map as a spherical RGB-D frame (rgbd360_map_render_*: the reference shows viewer.globalMap in a PCL window, OdometryRGBD360.cpp:242-268,
// and aligns against keyframes, OdometryKeyFrame360.cpp): a z-buffered splat of the table into the panorama of the dense alignment,
//     globalMap.renderSphere(rows, cols, pose, depth, rgb)     whose outputs RegisterPhotoICP::setTargetFrame takes as they are
// Ray casting through the map (rgbd360_map_raycast*): the first occupied voxel along a ray -- the same panorama as a per-pixel first hit,
// or any list of rays (pinhole views, single beams, the line of sight between two keyframe poses),
//     globalMap.raycastSphere(rows, cols, pose, depth, rgb)    globalMap.raycast(origins, dirs, t, &key3, &count, &rgb, &status)
// Surface normals (rgbd360_map_normals, rgbd360_map_raycast_surface*): one normal per voxel, fitted to the centroids around it and kept with
// the map -- the map as an oriented cloud, and the ray cast with the depth on the fitted plane and a normal per hit,
//     globalMap.normals(xyz, normal, &curvature, &status)      globalMap.raycastSurfaceSphere(rows, cols, pose, depth, normal, rgb)
// Editing (rgbd360_map_remove_* / _move_* / _rehash / _census): the SLAM programs optimise their keyframe poses continuously and redraw the
// map from them (SphereGraphSLAM.cpp, KFsphere_SLAM.cpp: optimizer.optimizeGraph(), getPoses(Map.vOptimizedPoses)); the sums are integers,
// so a frame leaves the map exactly as it came,
//     globalMap.remove(frame.sphereRGB, frame.sphereDepth, pose)            globalMap.move(rgb, depth, oldPose, optimisedPose)
//     if (c.n_tombstones > c.n_live) globalMap.rehash();      with c = globalMap.census(); rehash(capacity) grows or shrinks the table
// Free space (rgbd360_map_observe_* / _votes / _carve): what lets the map react to what a new frame sees -- an object that moved away, a
// ghost wall left by a pose corrected later.  Every pixel of a posed frame is a line of sight; the voxels it passes through well in front
// of the measured point collect through-votes, the voxel it ends in an end-vote, and carve() erases the voxels seen through and not measured.
// A lossy edit: a carved voxel forgets its points, and a later remove() of a frame that fed it returns false,
//     globalMap.observe(frame.sphereDepth, pose);   globalMap.carve();      votes(key3, through, end) reads the counts out instead
// Relocalisation (rgbd360_map_planes, rgbd360_map_plane_labels): the reference's Relocalizer360 (Relocalizer360.h:78-93) places a lost frame
// with  registerer.RegisterPbMap(keyframe, lostFrame, ..)  against the planes of what it has mapped, without an initial guess.  The map
// segmented into planar regions under its per-voxel normals is that plane set for the whole map,
//     globalMap.planes()      int status = globalMap.relocalize(framePlanes, pose)     0: accepted, pose = world <- frame
// (the loop over keyframes and its thresholds -- at least 5 matched planes, matched area above 10 -- stay the caller's policy)
// Submaps (rgbd360_map_merge / _unmerge / _records / _add_records): what a pose graph can move is a window of frames, not every frame.  A
// small map per keyframe window is composed into the global map at the window's pose and, after a correction, taken out and put back at
// the new one -- without the original frames, one launch each; the sums are integers, so both directions are exact,
//     globalMap.merge(submap, &pose);      globalMap.unmerge(submap, &oldPose); globalMap.merge(submap, &newPose);
//     globalMap.merge(other)               pose == nullptr: the union of two maps of one voxel size, word for word
//     copy.addRecords(globalMap.records())    a map copied, or written out and read back, with its bits intact
#pragma once

#include <algorithm>
#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "RegisterPhotoICP.hpp"
#include "../rgbd360_hip_diag.h"      // rgbd360_map_align_batch_trace (batchTrace)

namespace rgbd360 {

// The two parameter sets of the reference's filter class (FilterPointCloud.h:63-74): the voxel size, and the box
// x in [-2, 1] (the vertical axis of the sphere clouds), y and z in [-euclideanBox, euclideanBox].
struct FilterPointCloud {
    float voxelSize, lo[3], hi[3];
    explicit FilterPointCloud(float voxelSize_ = 0.05f, float euclideanBox = 4.0f)
        : voxelSize(voxelSize_), lo{-2.0f, -euclideanBox, -euclideanBox}, hi{1.0f, euclideanBox, euclideanBox} {}
};

struct MapPoint {      // one voxel: centroid, mean colour (bytes in the order of the inserted images), points it averages
    float x, y, z;
    uint8_t r, g, b;
    int count;
};

class GlobalMap {
   public:
    // The map lives on align's context (device, stream): keep `align` alive and its setters untouched while the map exists.
    // capacity: voxels the table has room for (rounded up to a power of two, 64 bytes each).
    GlobalMap(RegisterPhotoICP& align, const FilterPointCloud& filter = FilterPointCloud(), long long capacity = 1 << 22) {
        rgbd360_ctx* ctx = align.context();
        const int rc = rgbd360_map_create(ctx, filter.voxelSize, capacity, &map_);
        if (rc != 0) throw std::runtime_error("rgbd360_map_create (" + std::to_string(rc) + "): " + rgbd360_last_error(ctx));
        check(rgbd360_map_set_box(map_, filter.lo, filter.hi), "rgbd360_map_set_box");
    }
    ~GlobalMap() { rgbd360_map_destroy(map_); }
    GlobalMap(const GlobalMap&) = delete;
    GlobalMap& operator=(const GlobalMap&) = delete;

    // A sphere frame at `pose` (world <- frame).  rgb may be an empty view (data == nullptr): the colours stay 0.  convention as in
    // rgbd360_sphere_cloud: 0 Frame360 (Frame360.h:555-612), 1 Frame360_stereo, 2 RegisterPhotoICP.  Returns false when the table was
    // full and points of new voxels were dropped (stats().n_dropped_full); everything else throws.
    bool insert(const ImageView& rgb, const ImageView& depth, const Mat4f& pose, int convention = 0) {
        checkImages(rgb, depth, "GlobalMap::insert");
        return full(rgbd360_map_insert_sphere(map_, (const uint8_t*)rgb.data, rgb.step, depth.data, depth.step, depthType(depth),
                                              depth.rows, depth.cols, convention, pose.m, 0, &stats_),
                    "rgbd360_map_insert_sphere");
    }
    // Any cloud in its frame's coordinates: xyz[3 n], rgb3[3 n] or nullptr.
    bool insert(const float* xyz, const uint8_t* rgb3, long long n, const Mat4f& pose) {
        return full(rgbd360_map_insert_cloud(map_, xyz, rgb3, n, pose.m, 0, &stats_), "rgbd360_map_insert_cloud");
    }

    // Undoes insert() of the same arguments (the same box, the same voxel size; that insert must have returned true), bit for bit and whatever
    // was inserted in between.  Returns false when points were asked to leave that the map does not hold (editStats().n_missing /
    // n_underflow): its content is then unspecified, clear() it.  Everything else throws.
    bool remove(const ImageView& rgb, const ImageView& depth, const Mat4f& pose, int convention = 0) {
        checkImages(rgb, depth, "GlobalMap::remove");
        return matched(rgbd360_map_remove_sphere(map_, (const uint8_t*)rgb.data, rgb.step, depth.data, depth.step, depthType(depth),
                                                 depth.rows, depth.cols, convention, pose.m, 0, &edit_),
                       "rgbd360_map_remove_sphere");
    }
    bool remove(const float* xyz, const uint8_t* rgb3, long long n, const Mat4f& pose) {
        return matched(rgbd360_map_remove_cloud(map_, xyz, rgb3, n, pose.m, 0, &edit_), "rgbd360_map_remove_cloud");
    }
    // The frame inserted at oldPose moves to newPose (a pose-graph correction): removed and inserted over one upload.  false: a mismatch as
    // in remove(), or the table was full as in insert() -- editStats() and stats() tell which; the insertion happens either way.
    bool move(const ImageView& rgb, const ImageView& depth, const Mat4f& oldPose, const Mat4f& newPose, int convention = 0) {
        checkImages(rgb, depth, "GlobalMap::move");
        const int rc = rgbd360_map_move_sphere(map_, (const uint8_t*)rgb.data, rgb.step, depth.data, depth.step, depthType(depth),
                                               depth.rows, depth.cols, convention, oldPose.m, newPose.m, 0, &edit_, &stats_);
        check(rc, "rgbd360_map_move_sphere");
        return rc == 0;
    }
    bool move(const float* xyz, const uint8_t* rgb3, long long n, const Mat4f& oldPose, const Mat4f& newPose) {
        const int rc = rgbd360_map_move_cloud(map_, xyz, rgb3, n, oldPose.m, newPose.m, 0, &edit_, &stats_);
        check(rc, "rgbd360_map_move_cloud");
        return rc == 0;
    }
    const rgbd360_map_edit_stats& editStats() const { return edit_; }      // of the last remove / move
    // The table rebuilt without tombstones into `capacity` voxels (0: its current size): compaction, growing, shrinking.  A second table exists
    // during the call.  false: a voxel found no slot in the new table and the map is unchanged; a capacity below size() throws.
    bool rehash(long long capacity = 0) { return full(rgbd360_map_rehash(map_, capacity), "rgbd360_map_rehash"); }
    // Slots, occupied voxels, tombstones, points and inconsistent slots of a read-only scan of the table.
    rgbd360_map_census_counts census() const {
        rgbd360_map_census_counts c{};
        check(rgbd360_map_census(map_, &c), "rgbd360_map_census");
        return c;
    }

    // Point-to-point ICP of a sphere frame, or of a cloud in its frame's coordinates, against the map from `guess` (rgbd360_map_align_*:
    // the nearest neighbour is the nearest voxel centroid in the 27 cells around the point, max_dist in (0, leaf]).  The map is not changed.
    // Returns the status (RGBD360_OK / ILL_POSED / NO_VALID_PIXELS); alignResult() has the iterations, matches, fitness, hessian.
    rgbd360_map_align_params alignParams() const {
        rgbd360_map_align_params p;
        rgbd360_map_default_align_params(map_, &p);
        return p;
    }
    int alignSphere(const ImageView& depth, const Mat4f& guess, Mat4f& pose, int convention = 0, const rgbd360_map_align_params* params = nullptr) {
        if (depth.type == ImageView::U8C3) throw std::runtime_error("GlobalMap::alignSphere: a 16UC1 / 32FC1 depth image");
        const int rc = rgbd360_map_align_sphere(map_, depth.data, depth.step, depthType(depth), depth.rows, depth.cols, convention, guess.m, 0,
                                                params, pose.m, &align_);
        check(rc, "rgbd360_map_align_sphere");
        return rc;
    }
    int alignCloud(const float* xyz, long long n, const Mat4f& guess, Mat4f& pose, const rgbd360_map_align_params* params = nullptr) {
        const int rc = rgbd360_map_align_cloud(map_, xyz, n, guess.m, 0, params, pose.m, &align_);
        check(rc, "rgbd360_map_align_cloud");
        return rc;
    }
    const rgbd360_map_align_result& alignResult() const { return align_; }      // of the last alignSphere / alignCloud call

    // Point-to-plane ICP against the map (rgbd360_map_align_plane_*): the matches of alignSphere / alignCloud, the residual along the normal
    // of the plane fitted to the centroids of the occupied cells around the point; corners and edges (no plane) contribute nothing.
    rgbd360_map_align_plane_params alignPlaneParams() const {
        rgbd360_map_align_plane_params p;
        rgbd360_map_default_align_plane_params(map_, &p);
        return p;
    }
    int alignSpherePlane(const ImageView& depth, const Mat4f& guess, Mat4f& pose, int convention = 0, const rgbd360_map_align_plane_params* params = nullptr) {
        if (depth.type == ImageView::U8C3) throw std::runtime_error("GlobalMap::alignSpherePlane: a 16UC1 / 32FC1 depth image");
        const int rc = rgbd360_map_align_plane_sphere(map_, depth.data, depth.step, depthType(depth), depth.rows, depth.cols, convention,
                                                      guess.m, 0, params, pose.m, &alignPlane_);
        check(rc, "rgbd360_map_align_plane_sphere");
        return rc;
    }
    int alignCloudPlane(const float* xyz, long long n, const Mat4f& guess, Mat4f& pose, const rgbd360_map_align_plane_params* params = nullptr) {
        const int rc = rgbd360_map_align_plane_cloud(map_, xyz, n, guess.m, 0, params, pose.m, &alignPlane_);
        check(rc, "rgbd360_map_align_plane_cloud");
        return rc;
    }
    const rgbd360_map_align_plane_result& alignPlaneResult() const { return alignPlane_; }      // of the last alignSpherePlane / alignCloudPlane call

    // Robust kernels (rgbd360_map_set_align_robust): a setting of the map per method (RGBD360_MAP_METHOD_*), kind RGBD360_MAP_ROBUST_*, delta in
    // the units of the square root of the method's cost term (metres for point and plane).  Every align* call of the method, the batches,
    // alignSphereCoarseToFine and alignMapGICP honour it; RGBD360_MAP_ROBUST_NONE (the default) is the quadratic call.  robustInfo(): what the
    // last single alignment did with it (sum w, the contributing points, those with w < 1); robustInfo(job): a job of the last batch.
    void setAlignRobust(int method, int kind, double delta = 0.0, bool scaleWithLevel = false) {
        const rgbd360_map_robust r = {kind, scaleWithLevel ? 1 : 0, delta};
        check(rgbd360_map_set_align_robust(map_, method, &r), "rgbd360_map_set_align_robust");
    }
    rgbd360_map_robust alignRobust(int method) {
        rgbd360_map_robust r = {};
        check(rgbd360_map_get_align_robust(map_, method, &r), "rgbd360_map_get_align_robust");
        return r;
    }
    rgbd360_map_robust_info robustInfo() {
        rgbd360_map_robust_info info = {};
        check(rgbd360_map_align_robust_info(map_, &info), "rgbd360_map_align_robust_info");
        return info;
    }
    rgbd360_map_robust_info robustInfo(int job) {
        rgbd360_map_robust_info info = {};
        check(rgbd360_map_align_batch_robust_info(map_, job, &info), "rgbd360_map_align_batch_robust_info");
        return info;
    }

    // Many alignments in lock step (rgbd360_map_align_batch_* / rgbd360_map_align_plane_batch_*): inputs of one form and jobs (input index,
    // guess); per job poses[j] and results[j] are exactly what alignCloud / alignSphere (their Plane forms) return for that input from that
    // guess, with 2 max_iters + 3 launches and one synchronisation for the whole batch.  The frames of a batch share one size and depth type.
    // batchTrace(j): the steps of job j of the last batch;
    // bestJob: the job of most matches (then the smaller fitness, then the smaller index) among those that ended OK with at least
    // minMatched matches, -1 if none -- a policy for the jobs of one input from several guesses, not part of the alignment.
    static rgbd360_map_batch_job batchJob(int input, const Mat4f& guess) {
        rgbd360_map_batch_job j;
        j.input = input;
        std::copy(guess.m, guess.m + 16, j.guess);
        return j;
    }
    void alignBatchCloud(const std::vector<rgbd360_map_batch_cloud>& clouds, const std::vector<rgbd360_map_batch_job>& jobs, std::vector<Mat4f>& poses,
                         std::vector<rgbd360_map_align_result>& results, const rgbd360_map_align_params* params = nullptr) {
        poses.resize(jobs.size());
        results.assign(jobs.size(), rgbd360_map_align_result());
        check(rgbd360_map_align_batch_cloud(map_, clouds.data(), (int)clouds.size(), 0, jobs.data(), (int)jobs.size(), params, posesOut(poses), results.data()),
              "rgbd360_map_align_batch_cloud");
    }
    void alignBatchCloudPlane(const std::vector<rgbd360_map_batch_cloud>& clouds, const std::vector<rgbd360_map_batch_job>& jobs, std::vector<Mat4f>& poses,
                              std::vector<rgbd360_map_align_plane_result>& results, const rgbd360_map_align_plane_params* params = nullptr) {
        poses.resize(jobs.size());
        results.assign(jobs.size(), rgbd360_map_align_plane_result());
        check(rgbd360_map_align_plane_batch_cloud(map_, clouds.data(), (int)clouds.size(), 0, jobs.data(), (int)jobs.size(), params, posesOut(poses),
                                                  results.data()),
              "rgbd360_map_align_plane_batch_cloud");
    }
    void alignBatchSphere(const std::vector<ImageView>& depths, const std::vector<rgbd360_map_batch_job>& jobs, std::vector<Mat4f>& poses,
                          std::vector<rgbd360_map_align_result>& results, int convention = 0, const rgbd360_map_align_params* params = nullptr) {
        const std::vector<rgbd360_map_batch_frame> frames = batchFrames(depths, "GlobalMap::alignBatchSphere");
        poses.resize(jobs.size());
        results.assign(jobs.size(), rgbd360_map_align_result());
        check(rgbd360_map_align_batch_sphere(map_, frames.data(), (int)frames.size(), depthType(depths[0]), depths[0].rows, depths[0].cols, convention, 0,
                                             jobs.data(), (int)jobs.size(), params, posesOut(poses), results.data()),
              "rgbd360_map_align_batch_sphere");
    }
    void alignBatchSpherePlane(const std::vector<ImageView>& depths, const std::vector<rgbd360_map_batch_job>& jobs, std::vector<Mat4f>& poses,
                               std::vector<rgbd360_map_align_plane_result>& results, int convention = 0,
                               const rgbd360_map_align_plane_params* params = nullptr) {
        const std::vector<rgbd360_map_batch_frame> frames = batchFrames(depths, "GlobalMap::alignBatchSpherePlane");
        poses.resize(jobs.size());
        results.assign(jobs.size(), rgbd360_map_align_plane_result());
        check(rgbd360_map_align_plane_batch_sphere(map_, frames.data(), (int)frames.size(), depthType(depths[0]), depths[0].rows, depths[0].cols, convention,
                                                   0, jobs.data(), (int)jobs.size(), params, posesOut(poses), results.data()),
              "rgbd360_map_align_plane_batch_sphere");
    }
    std::vector<rgbd360_map_align_trace> batchTrace(int job) {
        int n = 0;
        check(rgbd360_map_align_batch_trace(map_, job, 0, &n, nullptr), "rgbd360_map_align_batch_trace");
        std::vector<rgbd360_map_align_trace> trace((size_t)n);
        check(rgbd360_map_align_batch_trace(map_, job, n, nullptr, trace.data()), "rgbd360_map_align_batch_trace");
        return trace;
    }
    static int bestJob(const std::vector<rgbd360_map_align_result>& results, long long minMatched = 0) {
        return rgbd360_map_align_best(results.data(), (int)results.size(), minMatched);
    }
    static int bestJob(const std::vector<rgbd360_map_align_plane_result>& results, long long minMatched = 0) {
        return rgbd360_map_align_plane_best(results.data(), (int)results.size(), minMatched);
    }

    // The rig's extrinsics against the map (rgbd360_map_calibrate_rig_*): clouds[k S + s] the cloud of sensor s in frame k in the sensor's
    // coordinates, poses (K, world <- rig) and extrinsics (S, rig <- sensor: Calib360::Rt_) in/out.  One unknown per free sensor shared
    // over all frames; with refine_poses (which needs a fixed_sensor) also one per frame: a small bundle adjustment of a keyframe window.
    // Returns the status; rigCalibResult() and rigCalibSensors() have the final evaluation.  The map is not changed: re-map with move().
    rgbd360_rig_calib_params rigCalibParams() const {
        rgbd360_rig_calib_params p;
        rgbd360_map_default_rig_calib_params(map_, &p);
        return p;
    }
    int calibrateRigClouds(const std::vector<rgbd360_map_batch_cloud>& clouds, std::vector<Mat4f>& poses, std::vector<Mat4f>& extrinsics,
                           const rgbd360_rig_calib_params* params = nullptr) {
        if (clouds.size() != poses.size() * extrinsics.size()) throw std::runtime_error("GlobalMap::calibrateRigClouds: one cloud per frame and sensor");
        rigSensors_.assign(extrinsics.size(), rgbd360_rig_calib_sensor());
        const int rc = rgbd360_map_calibrate_rig_clouds(map_, clouds.data(), (int)poses.size(), (int)extrinsics.size(), 0, posesOut(poses), posesOut(extrinsics),
                                                        params, &rigCalib_, rigSensors_.data());
        check(rc, "rgbd360_map_calibrate_rig_clouds");
        return rc;
    }
    // The same from K S pinhole depth images of one size and type (depths[k S + s]); K4 = {fx, fy, cx, cy} (Calib360::K()).
    int calibrateRigDepth(const std::vector<ImageView>& depths, const std::array<float, 4>& K4, std::vector<Mat4f>& poses, std::vector<Mat4f>& extrinsics,
                          const rgbd360_rig_calib_params* params = nullptr) {
        return calibrateRigDepth(nullptr, depths, K4, poses, extrinsics, params);
    }
    // ... with every image corrected on the device by its sensor's depth model first (DepthModels::handle(), DepthTrainer.hpp; null: none)
    int calibrateRigDepth(const rgbd360_depth_models* models, const std::vector<ImageView>& depths, const std::array<float, 4>& K4, std::vector<Mat4f>& poses,
                          std::vector<Mat4f>& extrinsics, const rgbd360_rig_calib_params* params = nullptr) {
        if (depths.empty() || depths.size() != poses.size() * extrinsics.size())
            throw std::runtime_error("GlobalMap::calibrateRigDepth: one image per frame and sensor");
        std::vector<rgbd360_map_batch_frame> in(depths.size());
        for (size_t k = 0; k < depths.size(); ++k) {
            if (depths[k].rows != depths[0].rows || depths[k].cols != depths[0].cols || depths[k].type != depths[0].type)
                throw std::runtime_error("GlobalMap::calibrateRigDepth: the images of a call share one size and depth type");
            in[k].depth = depths[k].data;
            in[k].depth_step = depths[k].step;
        }
        rigSensors_.assign(extrinsics.size(), rgbd360_rig_calib_sensor());
        const int rc = rgbd360_map_calibrate_rig_depth_models(map_, models, in.data(), depthType(depths[0]), depths[0].rows, depths[0].cols, K4[0], K4[1], K4[2],
                                                              K4[3], (int)poses.size(), (int)extrinsics.size(), 0, posesOut(poses), posesOut(extrinsics), params,
                                                              &rigCalib_, rigSensors_.data());
        check(rc, "rgbd360_map_calibrate_rig_depth_models");
        return rc;
    }
    const rgbd360_rig_calib_result& rigCalibResult() const { return rigCalib_; }
    const std::vector<rgbd360_rig_calib_sensor>& rigCalibSensors() const { return rigSensors_; }
    // Rt_01.txt .. in `dir`, where Calib360::loadExtrinsicCalibration reads them
    static bool saveExtrinsics(const std::vector<Mat4f>& extrinsics, const std::string& dir) {
        std::vector<float> flat(16 * extrinsics.size());
        for (size_t s = 0; s < extrinsics.size(); ++s) std::copy(extrinsics[s].m, extrinsics[s].m + 16, flat.begin() + 16 * s);
        return rgbd360_rig_save_extrinsics(flat.data(), (int)extrinsics.size(), dir.c_str()) == 0;
    }

    // Generalized ICP against the map (rgbd360_map_align_gicp_*): the matches of alignSphere / alignCloud, each weighted by
    // (C_B + C_A)^-1 -- C_B from the matched voxel's resident normal, C_A from the source point's normal (`normals`: 3 n floats in the
    // frame's coordinates, or nullptr).  A pair without a planar side counts as point-to-point.  alignGicpResult() has the counts.
    rgbd360_map_align_gicp_params alignGicpParams() const {
        rgbd360_map_align_gicp_params p;
        rgbd360_map_default_align_gicp_params(map_, &p);
        return p;
    }
    int alignCloudGICP(const float* xyz, const float* normals, long long n, const Mat4f& guess, Mat4f& pose, const rgbd360_map_align_gicp_params* params = nullptr) {
        const int rc = rgbd360_map_align_gicp_cloud(map_, xyz, normals, n, guess.m, 0, params, pose.m, &alignGicp_);
        check(rc, "rgbd360_map_align_gicp_cloud");
        return rc;
    }
    int alignSphereGICP(const ImageView& depth, const Mat4f& guess, Mat4f& pose, int convention = 0, const rgbd360_map_align_gicp_params* params = nullptr) {
        if (depth.type == ImageView::U8C3) throw std::runtime_error("GlobalMap::alignSphereGICP: a 16UC1 / 32FC1 depth image");
        const int rc = rgbd360_map_align_gicp_sphere(map_, depth.data, depth.step, depthType(depth), depth.rows, depth.cols, convention, guess.m, 0,
                                                     params, pose.m, &alignGicp_);
        check(rc, "rgbd360_map_align_gicp_sphere");
        return rc;
    }
    // Another map as the source (guess, pose: this map's world <- the source's world): the source's voxels with their normals, fitted under
    // this call's min_count / min_support / max_flatness, in ascending (i_z, i_y, i_x) order so that the sums are the same from run to run.
    int alignMapGICP(GlobalMap& source, const Mat4f& guess, Mat4f& pose, const rgbd360_map_align_gicp_params* params = nullptr) {
        const rgbd360_map_align_gicp_params p = params ? *params : alignGicpParams();
        rgbd360_map_normal_params np;
        rgbd360_map_default_normal_params(source.map_, &np);
        np.min_count = p.min_count, np.min_support = p.min_support, np.max_flatness = p.max_flatness;
        std::vector<float> xyz, normal;
        std::vector<int32_t> key3;
        const size_t n = (size_t)source.normals(xyz, normal, nullptr, nullptr, nullptr, &key3, nullptr, &np);
        std::vector<size_t> order(n);
        for (size_t k = 0; k < n; ++k) order[k] = k;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            for (int q = 2; q >= 0; --q)
                if (key3[3 * a + q] != key3[3 * b + q]) return key3[3 * a + q] < key3[3 * b + q];
            return false;
        });
        std::vector<float> sx(3 * n), sn(3 * n);
        for (size_t o = 0; o < n; ++o)
            for (int q = 0; q < 3; ++q) sx[3 * o + q] = xyz[3 * order[o] + q], sn[3 * o + q] = normal[3 * order[o] + q];
        return alignCloudGICP(sx.data(), sn.data(), (long long)n, guess, pose, &p);
    }
    const rgbd360_map_align_gicp_result& alignGicpResult() const { return alignGicp_; }      // of the last align*GICP call

    // Coloured ICP against the map (rgbd360_map_align_colour_*): the matches of alignSphere / alignCloud, the point-to-plane residual along the
    // matched voxel's resident normal (weight lambda_geometric) joined with the difference between the map's intensity, carried along its
    // resident tangent-plane gradient (colours()) to the point, and the point's own (weight 1 - lambda_geometric): the texture holds the pose
    // where geometry slides.  The colours are required: rgb an 8UC3 image of the depth image's size, rgb3 n x 3 bytes.
    rgbd360_map_align_colour_params alignColourParams() const {
        rgbd360_map_align_colour_params p;
        rgbd360_map_default_align_colour_params(map_, &p);
        return p;
    }
    int alignSphereColour(const ImageView& rgb, const ImageView& depth, const Mat4f& guess, Mat4f& pose, int convention = 0,
                          const rgbd360_map_align_colour_params* params = nullptr) {
        if (rgb.type != ImageView::U8C3 || depth.type == ImageView::U8C3 || rgb.rows != depth.rows || rgb.cols != depth.cols)
            throw std::runtime_error("GlobalMap::alignSphereColour: an 8UC3 image and a 16UC1 / 32FC1 depth image of one size");
        const int rc = rgbd360_map_align_colour_sphere(map_, static_cast<const uint8_t*>(rgb.data), rgb.step, depth.data, depth.step, depthType(depth),
                                                       depth.rows, depth.cols, convention, guess.m, 0, params, pose.m, &alignColour_);
        check(rc, "rgbd360_map_align_colour_sphere");
        return rc;
    }
    int alignCloudColour(const float* xyz, const uint8_t* rgb3, long long n, const Mat4f& guess, Mat4f& pose,
                         const rgbd360_map_align_colour_params* params = nullptr) {
        const int rc = rgbd360_map_align_colour_cloud(map_, xyz, rgb3, n, guess.m, 0, params, pose.m, &alignColour_);
        check(rc, "rgbd360_map_align_colour_cloud");
        return rc;
    }
    const rgbd360_map_align_colour_result& alignColourResult() const { return alignColour_; }      // of the last align*Colour call

    // Coarse-to-fine ICP (rgbd360_map_align_c2f_*): alignSphere / alignCloud (kind 0) or their Plane forms (kind 1) on the levels
    // top_shift .. 0 of the map pyramid, level s being the map at voxelSize * 2^s merged out of the table; each level starts from the pose the
    // one before ended on and matches within max_dist_leaves of ITS voxel size, so top_shift 3 captures eight voxel sizes.  The levels are
    // built or refreshed by the call (device memory beside the table: pyramidBytes(); releaseLevels() frees it).  The map is not changed.
    // Returns level 0's status; c2fResult() has every level's status, iterations, matches, fitness and pose.
    rgbd360_map_c2f_params c2fParams() const {
        rgbd360_map_c2f_params p;
        rgbd360_map_default_c2f_params(map_, &p);
        return p;
    }
    int alignSphereCoarseToFine(const ImageView& depth, const Mat4f& guess, Mat4f& pose, int convention = 0, const rgbd360_map_c2f_params* params = nullptr) {
        if (depth.type == ImageView::U8C3) throw std::runtime_error("GlobalMap::alignSphereCoarseToFine: a 16UC1 / 32FC1 depth image");
        const int rc = rgbd360_map_align_c2f_sphere(map_, depth.data, depth.step, depthType(depth), depth.rows, depth.cols, convention, guess.m, 0,
                                                    params, pose.m, &c2f_);
        check(rc, "rgbd360_map_align_c2f_sphere");
        return rc;
    }
    int alignCloudCoarseToFine(const float* xyz, long long n, const Mat4f& guess, Mat4f& pose, const rgbd360_map_c2f_params* params = nullptr) {
        const int rc = rgbd360_map_align_c2f_cloud(map_, xyz, n, guess.m, 0, params, pose.m, &c2f_);
        check(rc, "rgbd360_map_align_c2f_cloud");
        return rc;
    }
    const rgbd360_map_c2f_result& c2fResult() const { return c2f_; }      // of the last alignSphereCoarseToFine / alignCloudCoarseToFine call
    size_t pyramidBytes() const { return rgbd360_map_pyramid_bytes(map_); }
    void releaseLevels() { check(rgbd360_map_release_levels(map_), "rgbd360_map_release_levels"); }

    // Composing maps (rgbd360_map_merge / _unmerge / _records / _add_records).  merge: the live voxels of `source` added to this map --
    // pose nullptr: sum mode (equal voxel sizes, the keys kept, the seven words added: the map that received both maps' insertions, bit for
    // bit); a pose (this map's world <- the source's world): each source voxel enters as its count of coincident points at its posed centroid,
    // its colour sums kept.  Returns false when the table was full as insert() does (mergeStats().n_voxels_dropped).  unmerge: the same terms
    // taken off again -- the same unchanged source, pose and params, and that merge returned true: then this map is, bit for bit, the map
    // that never saw the merge.  Returns false on a mismatch as remove() does (mergeStats().n_missing / n_underflow).  records: the live slots
    // as they are, 8 words per voxel {key, count, Sx, Sy, Sz, Sr, Sg, Sb}, ascending key; addRecords adds such a list in sum mode (equal keys
    // add up; a bad record throws and leaves the map unchanged) and returns false when the table was full.
    rgbd360_map_merge_params mergeParams() const {
        rgbd360_map_merge_params p;
        rgbd360_map_default_merge_params(map_, &p);
        return p;
    }
    bool merge(GlobalMap& source, const Mat4f* pose = nullptr, const rgbd360_map_merge_params* params = nullptr) {
        return full(rgbd360_map_merge(map_, source.map_, pose ? pose->m : nullptr, params, &merge_), "rgbd360_map_merge");
    }
    bool unmerge(GlobalMap& source, const Mat4f* pose = nullptr, const rgbd360_map_merge_params* params = nullptr) {
        return matched(rgbd360_map_unmerge(map_, source.map_, pose ? pose->m : nullptr, params, &merge_), "rgbd360_map_unmerge");
    }
    std::vector<uint64_t> records() const {
        const long long n = size();
        std::vector<uint64_t> out((size_t)n * 8);
        const long long got = n ? rgbd360_map_records(map_, n, out.data()) : 0;
        if (got != n) throw std::runtime_error(std::string("rgbd360_map_records: ") + rgbd360_map_last_error(map_));
        return out;
    }
    bool addRecords(const std::vector<uint64_t>& records) {
        if (records.size() % 8 != 0) throw std::runtime_error("GlobalMap::addRecords: 8 words per record");
        return full(rgbd360_map_add_records(map_, records.data(), (long long)(records.size() / 8), 0, &merge_), "rgbd360_map_add_records");
    }
    const rgbd360_map_merge_stats& mergeStats() const { return merge_; }      // of the last merge / unmerge / addRecords

    // The map splatted into the full-sphere panorama of rows x cols at `pose` (world <- frame), the nearest voxel winning a pixel
    // (rgbd360_map_render_sphere; defaults: min_count 1, near = leaf, splat 1.0, max_half 8).  The vectors are resized; depth is float32
    // metres with 0 in holes, rgb 8UC3, count (may be nullptr) the winner's points with 0 in holes, key3 (may be nullptr) its (i_x, i_y, i_z).
    // The map is not changed.  renderStats() has the counters of the last call.
    rgbd360_map_render_params renderParams() const {
        rgbd360_map_render_params p;
        rgbd360_map_default_render_params(map_, &p);
        return p;
    }
    void renderSphere(int rows, int cols, const Mat4f& pose, std::vector<float>& depth, std::vector<uint8_t>& rgb, std::vector<int32_t>* count = nullptr,
                      std::vector<int32_t>* key3 = nullptr, const rgbd360_map_render_params* params = nullptr) {
        const size_t n = rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0;
        depth.assign(n, 0.f);
        rgb.assign(3 * n, 0);
        if (count) count->assign(n, 0);
        if (key3) key3->assign(3 * n, 0);
        check(rgbd360_map_render_sphere(map_, rows, cols, pose.m, params, depth.data(), rgb.data(), count ? count->data() : nullptr,
                                        key3 ? key3->data() : nullptr, &render_),
              "rgbd360_map_render_sphere");
    }
    const rgbd360_map_render_stats& renderStats() const { return render_; }      // of the last renderSphere call

    // Ray casting (rgbd360_map_raycast*; defaults: min_count 1, t_min = leaf, t_max and max_offset +inf, max_steps 8192): per ray the first
    // voxel with count >= min_count along o + t d.  raycast: origins and dirs hold 3 floats per ray (world coordinates); t is resized, 0 on a
    // miss; key3, count, rgb, status (RGBD360_RAY_*) may be nullptr.  raycastSphere: the panorama of renderSphere, each pixel the first hit of
    // its ray; depth and rgb are what RegisterPhotoICP::setTargetFrame takes.  The map is not changed.  raycastStats() has the counters of the
    // last call of either.
    rgbd360_map_raycast_params raycastParams() const {
        rgbd360_map_raycast_params p;
        rgbd360_map_default_raycast_params(map_, &p);
        return p;
    }
    void raycast(const std::vector<float>& origins, const std::vector<float>& dirs, std::vector<float>& t, std::vector<int32_t>* key3 = nullptr,
                 std::vector<int32_t>* count = nullptr, std::vector<uint8_t>* rgb = nullptr, std::vector<int32_t>* status = nullptr,
                 const rgbd360_map_raycast_params* params = nullptr) {
        if (origins.size() != dirs.size() || origins.size() % 3 != 0) throw std::runtime_error("GlobalMap::raycast: origins and dirs must hold 3 floats per ray");
        const size_t n = origins.size() / 3;
        t.assign(n, 0.f);
        if (key3) key3->assign(3 * n, 0);
        if (count) count->assign(n, 0);
        if (rgb) rgb->assign(3 * n, 0);
        if (status) status->assign(n, 0);
        check(rgbd360_map_raycast(map_, (long long)n, origins.data(), dirs.data(), 0, params, t.data(), key3 ? key3->data() : nullptr,
                                  count ? count->data() : nullptr, rgb ? rgb->data() : nullptr, status ? status->data() : nullptr, &raycast_),
              "rgbd360_map_raycast");
    }
    void raycastSphere(int rows, int cols, const Mat4f& pose, std::vector<float>& depth, std::vector<uint8_t>& rgb, std::vector<int32_t>* count = nullptr,
                       std::vector<int32_t>* key3 = nullptr, const rgbd360_map_raycast_params* params = nullptr) {
        const size_t n = rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0;
        depth.assign(n, 0.f);
        rgb.assign(3 * n, 0);
        if (count) count->assign(n, 0);
        if (key3) key3->assign(3 * n, 0);
        check(rgbd360_map_raycast_sphere(map_, rows, cols, pose.m, params, depth.data(), rgb.data(), count ? count->data() : nullptr,
                                         key3 ? key3->data() : nullptr, &raycast_),
              "rgbd360_map_raycast_sphere");
    }
    const rgbd360_map_raycast_stats& raycastStats() const { return raycast_; }      // of the last raycast / raycastSphere call, plain or surface

    // Surface normals (rgbd360_map_normals, rgbd360_map_raycast_surface*; defaults: min_count 1, min_support 5, max_flatness 0.05, max_shift
    // 2.0 leaves): one normal per voxel, fitted to the centroids of the 27 cells around it and kept resident with the map.  normals: one
    // record per voxel in no specified order; xyz is resized, the others may be nullptr; status is RGBD360_NORMAL_*, the normal is zero unless
    // it is RGBD360_NORMAL_OK; with a viewpoint (3 floats, world) the normals face it.  Returns the voxel count; normalStats() has the counts.
    // raycastSurface / raycastSurfaceSphere: raycast / raycastSphere with, per hit, the voxel's normal (3 floats, world, facing the ray's
    // origin) and the depth on the plane through the voxel's centroid where it is taken; onPlane() counts those rays.
    rgbd360_map_normal_params normalParams() const {
        rgbd360_map_normal_params p;
        rgbd360_map_default_normal_params(map_, &p);
        return p;
    }
    long long normals(std::vector<float>& xyz, std::vector<float>& normal, std::vector<float>* curvature = nullptr, std::vector<int32_t>* status = nullptr,
                      std::vector<int32_t>* count = nullptr, std::vector<int32_t>* key3 = nullptr, const float* viewpoint = nullptr,
                      const rgbd360_map_normal_params* params = nullptr) {
        const size_t n = (size_t)size();
        xyz.assign(3 * n, 0.f);
        normal.assign(3 * n, 0.f);
        if (curvature) curvature->assign(n, 0.f);
        if (status) status->assign(n, 0);
        if (count) count->assign(n, 0);
        if (key3) key3->assign(3 * n, 0);
        const long long got = rgbd360_map_normals(map_, params, viewpoint, (long long)n, xyz.data(), normal.data(), curvature ? curvature->data() : nullptr,
                                                  status ? status->data() : nullptr, count ? count->data() : nullptr, key3 ? key3->data() : nullptr,
                                                  &normal_);
        if (got != (long long)n) throw std::runtime_error(std::string("rgbd360_map_normals: ") + rgbd360_map_last_error(map_));
        return got;
    }
    const rgbd360_map_normal_stats& normalStats() const { return normal_; }      // of the last normals call
    // Colour (rgbd360_map_colours; defaults: the normals' three, min_gradient_support 4, min_spread 0.01): one intensity per voxel and its
    // gradient on the voxel's tangent plane (3 floats per metre, world), kept resident with the map.  One record per voxel ordered as
    // extract(); xyz is resized, the others may be nullptr; status is RGBD360_COLOUR_*, the gradient is zero unless it is RGBD360_COLOUR_OK.
    // Returns the voxel count; colourStats() has the counts.
    rgbd360_map_colour_params colourParams() const {
        rgbd360_map_colour_params p;
        rgbd360_map_default_colour_params(map_, &p);
        return p;
    }
    long long colours(std::vector<float>& xyz, std::vector<float>& intensity, std::vector<float>& gradient, std::vector<int32_t>* status = nullptr,
                      std::vector<int32_t>* count = nullptr, std::vector<int32_t>* key3 = nullptr, const rgbd360_map_colour_params* params = nullptr) {
        const size_t n = (size_t)size();
        xyz.assign(3 * n, 0.f);
        intensity.assign(n, 0.f);
        gradient.assign(3 * n, 0.f);
        if (status) status->assign(n, 0);
        if (count) count->assign(n, 0);
        if (key3) key3->assign(3 * n, 0);
        const long long got = rgbd360_map_colours(map_, params, (long long)n, xyz.data(), intensity.data(), gradient.data(), status ? status->data() : nullptr,
                                                  count ? count->data() : nullptr, key3 ? key3->data() : nullptr, &colour_);
        if (got != (long long)n) throw std::runtime_error(std::string("rgbd360_map_colours: ") + rgbd360_map_last_error(map_));
        return got;
    }
    const rgbd360_map_colour_stats& colourStats() const { return colour_; }      // of the last colours call
    size_t colourBytes() const { return rgbd360_map_colour_bytes(map_); }
    void releaseColours() { check(rgbd360_map_release_colours(map_), "rgbd360_map_release_colours"); }
    void raycastSurface(const std::vector<float>& origins, const std::vector<float>& dirs, std::vector<float>& t, std::vector<float>& normal,
                        std::vector<int32_t>* key3 = nullptr, std::vector<int32_t>* count = nullptr, std::vector<uint8_t>* rgb = nullptr,
                        std::vector<int32_t>* status = nullptr, const rgbd360_map_raycast_params* rayParams = nullptr,
                        const rgbd360_map_normal_params* normalParams = nullptr) {
        if (origins.size() != dirs.size() || origins.size() % 3 != 0)
            throw std::runtime_error("GlobalMap::raycastSurface: origins and dirs must hold 3 floats per ray");
        const size_t n = origins.size() / 3;
        t.assign(n, 0.f);
        normal.assign(3 * n, 0.f);
        if (key3) key3->assign(3 * n, 0);
        if (count) count->assign(n, 0);
        if (rgb) rgb->assign(3 * n, 0);
        if (status) status->assign(n, 0);
        check(rgbd360_map_raycast_surface(map_, (long long)n, origins.data(), dirs.data(), 0, rayParams, normalParams, t.data(), normal.data(),
                                          key3 ? key3->data() : nullptr, count ? count->data() : nullptr, rgb ? rgb->data() : nullptr,
                                          status ? status->data() : nullptr, &onPlane_, &raycast_),
              "rgbd360_map_raycast_surface");
    }
    void raycastSurfaceSphere(int rows, int cols, const Mat4f& pose, std::vector<float>& depth, std::vector<float>& normal, std::vector<uint8_t>& rgb,
                              std::vector<int32_t>* count = nullptr, std::vector<int32_t>* key3 = nullptr,
                              const rgbd360_map_raycast_params* rayParams = nullptr, const rgbd360_map_normal_params* normalParams = nullptr) {
        const size_t n = rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0;
        depth.assign(n, 0.f);
        normal.assign(3 * n, 0.f);
        rgb.assign(3 * n, 0);
        if (count) count->assign(n, 0);
        if (key3) key3->assign(3 * n, 0);
        check(rgbd360_map_raycast_surface_sphere(map_, rows, cols, pose.m, rayParams, normalParams, depth.data(), normal.data(), rgb.data(),
                                                 count ? count->data() : nullptr, key3 ? key3->data() : nullptr, &onPlane_, &raycast_),
              "rgbd360_map_raycast_surface_sphere");
    }
    long long onPlane() const { return onPlane_; }      // of the last raycastSurface / raycastSurfaceSphere call

    // Free-space observation and carving (rgbd360_map_observe_* / _votes / _carve; defaults: min_count 1, near = leaf, margin_leaves 2.0,
    // margin_rel 0, max_offset 0.5 leaves, max_steps 8192, accumulate 0).  observe: every pixel of the sphere frame at `pose`, or every
    // segment origin -> endpoint of a list (3 floats each, world coordinates), votes on the voxels it looks through; params->accumulate = 1
    // adds to the votes of the calls before.  The table is not changed.  votes: one record per voted voxel, sorted like points(); count reads
    // 0 for the voxels a carve erased; returns their number.  carve: erases the live voxels with through >= minThrough, end <= maxEnd and
    // (maxCount == 0 or count <= maxCount); the votes are spent afterwards.  Stale votes (the map was written since) throw.
    rgbd360_map_observe_params observeParams() const {
        rgbd360_map_observe_params p;
        rgbd360_map_default_observe_params(map_, &p);
        return p;
    }
    void observe(const ImageView& depth, const Mat4f& pose, int convention = 0, const rgbd360_map_observe_params* params = nullptr) {
        if (depth.type == ImageView::U8C3) throw std::runtime_error("GlobalMap::observe: a 16UC1 / 32FC1 depth image");
        check(rgbd360_map_observe_sphere(map_, depth.data, depth.step, depthType(depth), depth.rows, depth.cols, convention, pose.m, 0, params, &observe_),
              "rgbd360_map_observe_sphere");
    }
    void observe(const std::vector<float>& origins, const std::vector<float>& endpoints, const rgbd360_map_observe_params* params = nullptr) {
        if (origins.size() != endpoints.size() || origins.size() % 3 != 0)
            throw std::runtime_error("GlobalMap::observe: origins and endpoints must hold 3 floats per segment");
        check(rgbd360_map_observe_rays(map_, (long long)(origins.size() / 3), origins.data(), endpoints.data(), 0, params, &observe_), "rgbd360_map_observe_rays");
    }
    const rgbd360_map_observe_stats& observeStats() const { return observe_; }      // of the last observe call
    long long votes(std::vector<int32_t>& key3, std::vector<int32_t>& through, std::vector<int32_t>& end, std::vector<int32_t>* count = nullptr) {
        const long long n = rgbd360_map_votes(map_, 0, nullptr, nullptr, nullptr, nullptr);
        if (n < 0) throw std::runtime_error(std::string("rgbd360_map_votes: ") + rgbd360_map_last_error(map_));
        key3.assign(3 * (size_t)n, 0);
        through.assign((size_t)n, 0);
        end.assign((size_t)n, 0);
        if (count) count->assign((size_t)n, 0);
        const long long got = rgbd360_map_votes(map_, n, key3.data(), through.data(), end.data(), count ? count->data() : nullptr);
        if (got != n) throw std::runtime_error(std::string("rgbd360_map_votes: ") + rgbd360_map_last_error(map_));
        return n;
    }
    // Returns the voxels erased; carveStats() has the counters of the last call.
    long long carve(int minThrough = 1, int maxEnd = 0, int maxCount = 0) {
        check(rgbd360_map_carve(map_, minThrough, maxEnd, maxCount, &carve_), "rgbd360_map_carve");
        return carve_.n_voxels_carved;
    }
    const rgbd360_map_carve_stats& carveStats() const { return carve_; }
    size_t voteBytes() const { return rgbd360_map_vote_bytes(map_); }
    void releaseVotes() { check(rgbd360_map_release_votes(map_), "rgbd360_map_release_votes"); }

    // Planar regions and relocalisation (rgbd360_map_planes / _plane_labels; defaults: the normals' min_count 1, min_support 5, max_flatness
    // 0.05, then max_voxel_curvature inf, cos_angle cos 5 deg, max_offset 0.5 leaves, min_voxels 50, max_curvature 0.0013).  planes: the map's
    // planar regions by root key ascending, normals facing `viewpoint` (3 floats, world; nullptr: the origin), rootKey3 (may be nullptr) the
    // key of each region's root voxel; every plane that passes the filters comes back (the buffer grows to planeSegStats().n_planes_available).
    // planeLabels: one record per voxel in no specified order -- its key, its region's root key (its own where it has no normal), and the
    // region's place in planes() or -1.  relocalize: rgbd360_register_planes(ref = the map's planes, trg = framePlanes): the status (0: accepted),
    // pose = world <- frame, info (may be nullptr) the 6 x 6 information matrix; match (may be nullptr) gets, per map plane, the index of the frame
    // plane matched or -1.  mapPlanes (may be nullptr): the map planes used.
    rgbd360_map_plane_seg_params planeSegParams() const {
        rgbd360_map_plane_seg_params p;
        rgbd360_map_default_plane_seg_params(map_, &p);
        return p;
    }
    std::vector<rgbd360_plane> planes(std::vector<int32_t>* rootKey3 = nullptr, const float* viewpoint = nullptr,
                                      const rgbd360_map_plane_seg_params* params = nullptr) {
        std::vector<rgbd360_plane> out(64);
        int n = 0;
        for (;;) {
            if (rootKey3) rootKey3->assign(3 * out.size(), 0);
            check(rgbd360_map_planes(map_, params, viewpoint, (int)out.size(), out.data(), rootKey3 ? rootKey3->data() : nullptr, &n, &planeSeg_),
                  "rgbd360_map_planes");
            if (planeSeg_.n_planes_available <= (long long)out.size()) break;
            out.resize((size_t)planeSeg_.n_planes_available);
        }
        out.resize((size_t)n);
        if (rootKey3) rootKey3->resize(3 * (size_t)n);
        return out;
    }
    long long planeLabels(std::vector<int32_t>& key3, std::vector<int32_t>& labelKey3, std::vector<int32_t>& planeIndex,
                          const rgbd360_map_plane_seg_params* params = nullptr) {
        const size_t n = (size_t)size();
        key3.assign(3 * n, 0);
        labelKey3.assign(3 * n, 0);
        planeIndex.assign(n, -1);
        const long long got = rgbd360_map_plane_labels(map_, params, (long long)n, key3.data(), labelKey3.data(), planeIndex.data());
        if (got != (long long)n) throw std::runtime_error(std::string("rgbd360_map_plane_labels: ") + rgbd360_map_last_error(map_));
        return got;
    }
    const rgbd360_map_plane_seg_stats& planeSegStats() const { return planeSeg_; }      // of the last planes / relocalize call
    int relocalize(const std::vector<rgbd360_plane>& framePlanes, Mat4f& pose, float* info = nullptr, std::vector<int32_t>* match = nullptr,
                   int maxMatchPlanes = 0, int registMode = 0, const rgbd360_pbmap_params* pbmapParams = nullptr,
                   const rgbd360_map_plane_seg_params* params = nullptr, std::vector<rgbd360_plane>* mapPlanes = nullptr) {
        const std::vector<rgbd360_plane> ref = planes(nullptr, nullptr, params);
        if (match) match->assign(std::max<size_t>(ref.size(), 1), -1);
        const int rc = rgbd360_register_planes(ref.data(), (int)ref.size(), framePlanes.data(), (int)framePlanes.size(), maxMatchPlanes, registMode,
                                               pbmapParams, pose.m, info, match ? match->data() : nullptr, nullptr, nullptr);
        if (rc < 0) throw std::runtime_error("rgbd360_register_planes: bad arguments");
        if (match) match->resize(ref.size());
        if (mapPlanes) *mapPlanes = ref;
        return rc;
    }
    size_t planeBytes() const { return rgbd360_map_plane_bytes(map_); }
    void releasePlanes() { check(rgbd360_map_release_planes(map_), "rgbd360_map_release_planes"); }

    long long size() const { return rgbd360_map_size(map_); }
    size_t bytes() const { return rgbd360_map_bytes(map_); }
    void clear() { check(rgbd360_map_clear(map_), "rgbd360_map_clear"); }
    const rgbd360_map_stats& stats() const { return stats_; }      // of the last insert

    // One point per voxel, sorted by (i_z, i_y, i_x): the order of pcl::VoxelGrid's output.
    std::vector<MapPoint> points() const {
        const long long n = size();
        std::vector<float> xyz((size_t)n * 3);
        std::vector<uint8_t> rgb((size_t)n * 3);
        std::vector<int32_t> count((size_t)n);
        const long long got = n ? rgbd360_map_extract(map_, n, xyz.data(), rgb.data(), count.data(), nullptr) : 0;
        if (got != n) throw std::runtime_error(std::string("rgbd360_map_extract: ") + rgbd360_map_last_error(map_));
        std::vector<MapPoint> out((size_t)n);
        for (size_t k = 0; k < out.size(); ++k)
            out[k] = {xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2], rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2], count[k]};
        return out;
    }

    rgbd360_map* handle() { return map_; }

   private:
    static int depthType(const ImageView& depth) { return depth.type == ImageView::U16C1 ? 0 : 1; }      // the entries' depth_type
    void check(int rc, const char* what) const {
        if (rc < 0) throw std::runtime_error(std::string(what) + " (" + std::to_string(rc) + "): " + rgbd360_map_last_error(map_));
    }
    bool full(int rc, const char* what) const {
        check(rc, what);
        return rc != RGBD360_MAP_FULL;
    }
    bool matched(int rc, const char* what) const {
        check(rc, what);
        return rc != RGBD360_MAP_MISMATCH;
    }
    static void checkImages(const ImageView& rgb, const ImageView& depth, const char* who) {
        if (depth.type == ImageView::U8C3 || (rgb.data && (rgb.type != ImageView::U8C3 || rgb.rows != depth.rows || rgb.cols != depth.cols)))
            throw std::runtime_error(std::string(who) + ": an 8UC3 colour image and a 16UC1 / 32FC1 depth image of one size");
    }
    // the batch entries' outputs and inputs: the poses as 16 floats each; the frames of a batch, all of the first one's size and type
    static float* posesOut(std::vector<Mat4f>& poses) {
        static_assert(sizeof(Mat4f) == 16 * sizeof(float), "a Mat4f is its 16 floats");
        return poses.empty() ? nullptr : poses[0].m;
    }
    static std::vector<rgbd360_map_batch_frame> batchFrames(const std::vector<ImageView>& depths, const char* who) {
        if (depths.empty()) throw std::runtime_error(std::string(who) + ": no frames");
        std::vector<rgbd360_map_batch_frame> frames;
        for (const ImageView& d : depths) {
            if (d.type == ImageView::U8C3 || d.type != depths[0].type || d.rows != depths[0].rows || d.cols != depths[0].cols)
                throw std::runtime_error(std::string(who) + ": 16UC1 / 32FC1 depth images of one size and type");
            frames.push_back({d.data, d.step});
        }
        return frames;
    }
    rgbd360_map* map_ = nullptr;
    rgbd360_map_stats stats_{};
    rgbd360_map_edit_stats edit_{};
    rgbd360_map_align_result align_{};
    rgbd360_map_align_plane_result alignPlane_{};
    rgbd360_map_align_gicp_result alignGicp_{};
    rgbd360_map_align_colour_result alignColour_{};
    rgbd360_map_c2f_result c2f_{};
    rgbd360_map_render_stats render_{};
    rgbd360_map_raycast_stats raycast_{};
    rgbd360_map_normal_stats normal_{};
    rgbd360_map_colour_stats colour_{};
    rgbd360_map_plane_seg_stats planeSeg_{};
    rgbd360_map_observe_stats observe_{};
    rgbd360_map_carve_stats carve_{};
    rgbd360_map_merge_stats merge_{};
    rgbd360_rig_calib_result rigCalib_{};
    std::vector<rgbd360_rig_calib_sensor> rigSensors_;
    long long onPlane_ = 0;
};

}  // namespace rgbd360
