/*
 * rgbd360_hip.h -- C ABI of the MI355X (gfx950) dense spherical RGB-D alignment library.
 *
 * Drop-in boundary for ONE path of EduFdez/rgbd360: RegisterPhotoICP's spherical alignment
 * (setTargetFrame / setSourceFrame / alignFrames360 with its three occlusion modes and the per-pixel passes they
 * call), the pinhole single-sensor alignFrames, and the adjacent Frame360 per-pixel stages (frame file reader,
 * 8-sensor spherical stitching, sphere cloud, normal map, planar regions).  Everything is plain C: opaque context, POD structs, raw
 * pointers and sizes.  File:line citations are relative to the reference tree; "RPI.h" is
 * include/RegisterPhotoICP.h.
 *
 * Conventions
 *   - 4x4 poses and the 6x6 Hessian are COLUMN-MAJOR float arrays (Eigen's default layout, which
 *     is what Eigen::Matrix4f::data() of the reference's relPose/hessian hands over).
 *   - relPose maps source-frame points into the target frame: p_trg = R p_src + t (RPI.h:2663).
 *   - Images are row-major with an explicit byte stride (cv::Mat::step).  rgb is 8UC3, depth is
 *     16UC1 millimetres (depth_type 0; Frame360.h:394) or 32FC1 metres (depth_type 1; RPI.h:318).
 *   - Host image pointers are copied before the call returns; the caller keeps ownership
 *     (the reference aliases cv::Mat buffers, RPI.h:296,319, and never frees caller memory).
 *   - A context is stateful and not re-entrant, like a RegisterPhotoICP object (one per thread).
 *   - Every function returns 0 on success, a positive rgbd360 status (below) for algorithmic
 *     outcomes and a negative value for HIP/argument errors; rgbd360_last_error() has the text.
 *   - There is NO CPU fallback: without a usable HIP device rgbd360_create fails.
 */
#ifndef RGBD360_HIP_H
#define RGBD360_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rgbd360_ctx rgbd360_ctx;

/* costFuncType, RPI.h:194 */
enum { RGBD360_PHOTO_CONSISTENCY = 0, RGBD360_DEPTH_CONSISTENCY = 1, RGBD360_PHOTO_DEPTH = 2 };

/* status codes */
enum {
    RGBD360_OK = 0,
    RGBD360_ILL_POSED = 1,      /* rank(H + lambda diag H) != 6, RPI.h:4682-4690: pose_out = last accepted pose */
    RGBD360_NO_VALID_PIXELS = 2, /* the error pass found no residual (the reference would divide by zero) */
    RGBD360_MAP_FULL = 3,       /* rgbd360_map_insert_*: points of new voxels found no free slot (within the probe bound) and were dropped (counted) */
    RGBD360_MAP_MISMATCH = 4,   /* rgbd360_map_remove_* / _move_*: points were asked to leave that the map does not hold (counted); its content is then unspecified */
    RGBD360_NOT_CONVERGED = 5   /* rgbd360_graph_marginals / _relative_covariances: columns did not reach cg_tol within cg_max_iters (counted); everything is written */
};

/* Replaces the constructor defaults + setters of RegisterPhotoICP (RPI.h:201-221, 224-269) and the
 * loop constants of alignFrames360 (RPI.h:4593-4595). */
typedef struct {
    int   n_pyr;            /* setNumPyr, default 4 */
    float min_depth;        /* setMinDepth, 0.3 m */
    float max_depth;        /* setMaxDepth, 6.0 m */
    float sigma_photo;      /* setGrayVariance (sets the std-dev, RPI.h:242-245), 6/255 */
    float sigma_depth;      /* setDepthVariance (std-dev, RPI.h:248-251), 0.2 */
    float thres_sal_photo;  /* thresSaliencyIntensity, 0.01 */
    float thres_sal_depth;  /* thresSaliencyDepth, 0.01 */
    int   max_iters;        /* 10 */
    float tol_residual;     /* 1e-3 */
    float tol_update;       /* 1e-4 */
    int   mask_seams;       /* 1: zero the gradient bands at the 8-sensor seams (RPI.h:4538-4549) */
    int   device;           /* HIP device ordinal */
} rgbd360_params;

/* What callers read from a RegisterPhotoICP after alignFrames360: getHessian()/getGradient()
 * (RPI.h:279-288), SSO, avPhotoResidual/avDepthResidual (RPI.h:180-189), num_iterations (RPI.h:177). */
typedef struct {
    int    status;
    int    iters[8];        /* accepted Gauss-Newton iterations per pyramid level (index = level) */
    float  sso;             /* visible pixels / image size at level 0 (RPI.h:3226) */
    double err_final;       /* RMS residual of the error pass at pose_out, level 0 (occlusion 1 / 2 and the pinhole path:
                               avPhotoResidual + avDepthResidual, as their error functions define it) */
    double rms_photo;       /* photo / depth RMS of that pass (the reference leaves these unset on this path) */
    double rms_depth;
    float  hessian[36];     /* column-major 6x6: H of the last calcHessGrad_sphere the reference would have run */
    float  gradient[6];
} rgbd360_result;

void rgbd360_default_params(rgbd360_params* p);

/* RegisterPhotoICP::RegisterPhotoICP() (RPI.h:201) */
int  rgbd360_create(const rgbd360_params* p, rgbd360_ctx** out);
void rgbd360_destroy(rgbd360_ctx* ctx);
const char* rgbd360_last_error(rgbd360_ctx* ctx);

/* RegisterPhotoICP::setTargetFrame(cv::Mat& rgb, cv::Mat& depth) (RPI.h:498-516): gray conversion,
 * gray + depth pyramids, gradient pyramids.  Host pointers. */
int rgbd360_set_target(rgbd360_ctx* ctx, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                       int depth_type, int rows, int cols);
/* RegisterPhotoICP::setSourceFrame (RPI.h:480-494) + the per-level LUT of 3-D points (RPI.h:4554-4587). */
int rgbd360_set_source(rgbd360_ctx* ctx, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                       int depth_type, int rows, int cols);
/* Same, images already resident in device memory (HBM) on the context's device. */
int rgbd360_set_target_dev(rgbd360_ctx* ctx, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev,
                           size_t depth_step, int depth_type, int rows, int cols);
int rgbd360_set_source_dev(rgbd360_ctx* ctx, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev,
                           size_t depth_step, int depth_type, int rows, int cols);
/* Odometry reuse: the previous source frame becomes the target without re-uploading
 * (OdometryRGBD360.cpp:189-190 re-sets both frames every step). Builds the target gradients on device. */
int rgbd360_promote_source_to_target(rgbd360_ctx* ctx);

/* The arithmetic of the warp -- spherical (RPI.h:2663-2684 / 2959-2989: p' = R p + t, phi = asin(x / |p'|), theta = atan2(y, z) + PI,
 * row / column = round(...)) and pinhole (RPI.h:701-708: column = round(x fx / z + ox), ...) -- for every later pass of this context:
 * rgbd360_align360 and its _begin / _finish, the batch and sequence entries that run on this context, the occlusion-aware passes,
 * rgbd360_eval*, rgbd360_warp_indices*, rgbd360_align_pinhole; the sibling contexts and engines a sequence call creates inherit it, a
 * multi-GPU handle has rgbd360_multi_set_index_arithmetic, an 8-sensor rig rgbd360_rig_set_index_arithmetic:
 *   0 (default): the device definition -- fused multiply-adds, two correctly rounded arctangent evaluations by one polynomial,
 *      round-half-up; mirrored bit for bit by the CPU checker's math_mode 1.  About 1e-4 of the pixels land on a neighbouring target
 *      pixel compared with the reference built against glibc.
 *   1: the REFERENCE's arithmetic -- Eigen's product order without fused multiply-adds, norm(), 1 / dist, asinf, atan2f + (double) PI,
 *      roundf, the two functions restated operation for operation from glibc 2.35's fdlibm float code (csrc/libm_f32.h; neither is
 *      correctly rounded, so "the same index" means that operation sequence).  Target indices, visibility and |p'|^2 are bit-equal to
 *      the reference's own; the spherical per-pixel pass costs ~1.8 x.  The pinhole warp has no transcendental: there the option means
 *      the reference's operation order, 1.0 / z in double and roundf.
 * Returns -6 while an alignment is in flight. */
int rgbd360_set_index_arithmetic(rgbd360_ctx* ctx, int mode);
int rgbd360_get_index_arithmetic(rgbd360_ctx* ctx);

/* RegisterPhotoICP::alignFrames360(pose_guess, method, occlusion) (RPI.h:4519-4784) + getOptimalPose().
 * occlusion 0 = regular registration, 1 / 2 = the z-buffer variants errorPhotoICP_sphereOcc1/2 + calcHessGrad_sphereOcc1/2
 * (RPI.h:3232-4249) with the sequential semantics of the reference source (its OpenMP build races on the z-buffer; see
 * DESIGN.md).  occlusion 1 needs method PHOTO_DEPTH: with one modality the reference's error is 0/0 and it returns the
 * guess (status RGBD360_NO_VALID_PIXELS here). */
int rgbd360_align360(rgbd360_ctx* ctx, const float guess[16], int method, int occlusion, float pose_out[16],
                     rgbd360_result* res);

/* The same alignment split in two, so that several contexts (one per frame pair, each on its own HIP stream) can be in
 * flight on one GPU at once: _begin enqueues the coarse-to-fine schedule and returns without waiting; _finish waits,
 * tops the schedule up if a level needed more iterations than were enqueued, and returns what rgbd360_align360 returns.
 * Coarse-level launches of different pairs then overlap on the device (they fill only a fraction of the CUs). */
int rgbd360_align360_begin(rgbd360_ctx* ctx, const float guess[16], int method, int occlusion);
int rgbd360_align360_finish(rgbd360_ctx* ctx, float pose_out[16], rgbd360_result* res);

/* A sequence of n_frames frames = n_frames-1 consecutive pairs (pair j: frame j = target, frame j+1 = source), the way
 * OdometryRGBD360.cpp:141-297 walks a sequence; SURVEY.md 8b/8e's batch entry for ONE GPU (several GPUs: rgbd360_multi_* below,
 * or one process per GPU each calling this on its contiguous shard, rgbd360_amd/batch.py).  rgb[k] / depth[k]: host images as
 * in rgbd360_set_target.  n_inflight (1..64) pairs are in flight: the sequence is cut into that many contiguous spans ("slots")
 * which advance in lock step -- every kernel launch of a round (frame set-up, each pass and solve of each pyramid level)
 * carries a slot dimension, so a round of n_inflight alignments costs the launch count of one (csrc/sequence_engine.h;
 * 32 = two engines of 16 slots is the measured optimum at 2048x1024, ~3.6 GB of HBM; 16 costs 5 %; host frames use at most 16).  Inside a span every frame is uploaded once,
 * one round ahead of its alignment on a copy stream: the host images must stay unchanged until the call returns.  Poses are
 * bit-identical to rgbd360_align360 pair by pair, whatever n_inflight.  The occlusion-aware variants run one context per span
 * instead (at most six, three when GPU_MAX_HW_QUEUES > 4: the measured optima of that route).  guess (NULL = identity) is the initial pose of every pair.  poses_out: (n_frames-1) x 16
 * floats column-major; results_out (may be NULL): n_frames-1 records whose .status carries the per-pair outcome (0 / ILL_POSED
 * / NO_VALID_PIXELS).  Returns 0, or the first negative error. */
int rgbd360_align360_batch(rgbd360_ctx* ctx, int n_frames, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                           size_t depth_step, int depth_type, int rows, int cols, const float guess[16], int method,
                           int occlusion, int n_inflight, float* poses_out, rgbd360_result* results_out);
/* The same with every rgb[k] / depth[k] already in HBM on the context's device (as rgbd360_set_target_dev): no PCIe traffic
 * inside the call; poses_out / results_out stay host arrays. */
int rgbd360_align360_batch_dev(rgbd360_ctx* ctx, int n_frames, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                               size_t depth_step, int depth_type, int rows, int cols, const float guess[16], int method,
                               int occlusion, int n_inflight, float* poses_out, rgbd360_result* results_out);

/* ---- resident frame store: arbitrary pairs in lock step (csrc/frame_store.h) -----------------------------------------------
 * The sequence entry above aligns CONSECUTIVE pairs from ONE guess (OdometryRGBD360.cpp:141-297).  The reference's other callers
 * align one keyframe against many frames, or one frame against several keyframes in both roles, each pair from its own guess
 * (OdometryKeyFrame360.cpp:244-253, KFsphere_SLAM.cpp:146-150, 370-375, 423-428, LoopClosure360.h:309-312, 348-351).  A store
 * keeps `capacity` frames of one size in HBM in prepared form (per pyramid level the source records and both target record
 * streams of the per-pixel pass): a frame is prepared once, when it is put, whatever number of pairs it later takes part in and
 * in whichever role.  An align call takes (target entry, source entry, guess) triples and runs them through the lock-step
 * schedule of the sequence engine.  Per pair, pose / status / iters / hessian are bit-identical to rgbd360_align360 on the same
 * two frames and guess.  The store takes the context's parameters when it is created and its index arithmetic at every align
 * call; it is destroyed BEFORE its context and used from one thread at a time.
 * Out of scope: occlusion 1 / 2, the pinhole and rig paths, several GPUs, eviction (the caller picks the entry to overwrite),
 * PbMap (the guess is an input). */
typedef struct rgbd360_store rgbd360_store;
/* capacity frames of rows x cols on ctx's device.  0; -1 bad arguments (capacity < 1, the size limits of the sequence entry);
 * -103 out of device memory (nothing stays allocated).  The message of a failed create is the CONTEXT's last error. */
int  rgbd360_store_create(rgbd360_ctx* ctx, int capacity, int rows, int cols, rgbd360_store** out);
void rgbd360_store_destroy(rgbd360_store* st);
const char* rgbd360_store_last_error(rgbd360_store* st);
/* bytes of HBM one entry occupies (the store: capacity times that, plus the set-up scratch of at most 32 frames). */
size_t rgbd360_store_entry_bytes(const rgbd360_store* st);
/* Prepares n frames into the entries entry[0..n) (any order, distinct, 0 <= entry < capacity; an occupied entry is
 * overwritten).  Images as rgbd360_set_target (on_device = 0: host images, copied before the call returns) or as
 * rgbd360_set_target_dev (on_device = 1).  All n frames go through the fused set-up together, at most 32 per launch.
 * 0, -1 bad arguments (nothing launched), other negatives: HIP errors (the named entries are then empty). */
int  rgbd360_store_put(rgbd360_store* st, int n, const int* entry, const uint8_t* const* rgb, size_t rgb_step,
                       const void* const* depth, size_t depth_step, int depth_type, int on_device);
/* 1 occupied, 0 empty, -1 out of range. */
int  rgbd360_store_occupied(const rgbd360_store* st, int entry);
/* n_pairs alignments: pair k = alignFrames360 with entry trg[k] as target frame, entry src[k] as source frame and the 16 floats
 * at guesses + 16 k (column-major; guesses == NULL: identity for all) as pose_guess.  trg[k] == src[k], repeated entries and
 * repeated pairs are allowed.  method 0 / 1 / 2 (-4 otherwise); occlusion must be 0 (-1 otherwise); n_inflight 1..64 as in
 * rgbd360_align360_batch: pairs run in rounds of n_inflight in list order, the result does not depend on it.  poses_out
 * n_pairs x 16 floats, results_out (may be NULL) n_pairs records, both in list order.  n_pairs == 0 returns 0 and writes
 * nothing.  -1 and no launch at all if any index is out of range or names an empty entry (the message names the first such
 * pair). */
int  rgbd360_store_align(rgbd360_store* st, int n_pairs, const int* trg, const int* src, const float* guesses, int method,
                         int occlusion, int n_inflight, float* poses_out, rgbd360_result* results_out);

/* ---- resident voxel-grid global map (csrc/voxel_map.h) ----------------------------------------------------------------------
 * The other half of the reference's odometry loop: after the alignment every frame is added to a global point-cloud map,
 *   filter.filterEuclidean(frame->sphereCloud); currentPose = currentPose * rigidTransf;
 *   pcl::transformPointCloud(*frame->sphereCloud, *tc, currentPose); *viewer.globalMap += *tc; filter.filterVoxel(viewer.globalMap);
 * (OdometryRGBD360.cpp:242-268; OdometryKeyFrame360.cpp:316-343, SphereGraphSLAM.cpp:116-137, 193-209, KFsphere_SLAM.cpp:236, 558;
 * the filter class is FilterPointCloud.h:63-99).  A map is a hash grid in HBM: inserting a frame costs O(frame), not the O(map) of
 * the reference's re-filtering.  Per input point, in this order:
 *   1 point   from a sphere image: the point rgbd360_sphere_cloud gives for that pixel and convention, bit for bit; from a cloud: the
 *             three floats.  Skipped (and not counted as valid) unless all three are finite.
 *   2 box     in the frame's own coordinates, before the pose: kept iff lo[k] <= p[k] <= hi[k], limits included (pcl::PassThrough).
 *   3 pose    16 floats, column-major, world <- frame: w_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k in float32, every product and sum
 *             rounded on its own (no fused multiply-add).
 *   4 range   dropped and counted if a w_k is not finite or |w_k| >= 4096.
 *   5 voxel   i_k = (int)floorf(w_k * inv_leaf), inv_leaf = 1.0f / leaf in float32 (PCL's floor(x * inverse_leaf_size)): the cell
 *             boundaries do not depend on the cloud's bounds; negative coordinates floor.
 *   6 sums    per voxel, exact: count, S_k += llrint((double)w_k * 1048576.0) in int64 (half to even), integer sums of r, g, b.
 * Read-out per occupied voxel: centroid_k = (float)((double)S_k / ((double)count * 1048576.0)), colour_c = S_c / count (integer
 * division; PCL's float-to-uint8 cast truncates too), the key (i_x, i_y, i_z) and the count.  The result does not depend on the
 * order in which points or frames arrive and is the same from run to run.
 * Two deliberate differences from the reference.  Every point has weight one: the map is pcl::VoxelGrid applied ONCE to the
 * concatenation of all inserted clouds, whereas the reference's per-frame re-filter turns the previous centroid into a single point
 * of the next average, so that there the order of the frames decides the result.  And the sums are integers instead of PCL's float
 * accumulators.  (PCL is not part of the reference tree: parity with pcl::VoxelGrid itself is unpinned, as for the other PCL-backed
 * stages.)
 * A map is destroyed BEFORE its context and used from one thread at a time, like a store.
 * A map can be edited (rgbd360_map_remove_* / _move_* / _rehash / _census below): what was inserted can be taken out again, exactly.
 * Voxels that later measurements look straight through can be erased without the source data (rgbd360_map_observe_* / _carve below).
 * Out of scope: removal by age, per-frame or per-voxel provenance, moving the grid, several GPUs. */
typedef struct rgbd360_map rgbd360_map;
typedef struct { long long n_valid, n_box_rejected, n_out_of_range, n_added, n_dropped_full, n_voxels; } rgbd360_map_stats;
/* A map of `leaf` metres (>= 0.004) with room for capacity_voxels voxels (rounded up to a power of two, 64 bytes each) on ctx's
 * device; the box starts as FilterPointCloud's default (FilterPointCloud.h:63-74).  0; -1 bad arguments; -103 out of memory (nothing
 * stays allocated).  The message of a failed create is the CONTEXT's last error.
 * A new voxel looks for a free slot in at most 2048 consecutive slots of the table (all of it when the table is smaller): when it
 * finds none its points are dropped as if the table were full (RGBD360_MAP_FULL), which bounds the cost of a frame on a crowded
 * table.  Below about 85 % load such a run of taken slots does not occur (probability < 1e-11 per voxel); give the map twice the
 * voxels expected. */
int    rgbd360_map_create(rgbd360_ctx* ctx, float leaf, long long capacity_voxels, rgbd360_map** out);
void   rgbd360_map_destroy(rgbd360_map* map);
const char* rgbd360_map_last_error(rgbd360_map* map);
/* bytes of HBM the table occupies */
size_t rgbd360_map_bytes(const rgbd360_map* map);
/* filterEuclidean's limits (FilterPointCloud.h:66-71, 78-89): x in [-2, 1], y and z in [-4, 4] by default.  NULL, NULL: no box. */
int    rgbd360_map_set_box(rgbd360_map* map, const float lo[3], const float hi[3]);
/* OdometryRGBD360.cpp:242, 266-268 for one sphere frame: images as in rgbd360_set_target (on_device = 0: host images, free when the
 * call returns; 1: device memory on the map's device), convention as in rgbd360_sphere_cloud, the points formed inside the kernel.
 * rgb may be NULL: the colour sums stay 0.  stats (may be NULL) is filled per call; n_voxels is the map's size after the call.
 * 0; RGBD360_MAP_FULL when points of new voxels were dropped (points of voxels already in the table are still added); -1 bad
 * arguments (a bad convention or depth type, NULL depth or pose: nothing is launched); an empty image returns 0 and touches nothing. */
int    rgbd360_map_insert_sphere(rgbd360_map* map, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                                 int depth_type, int rows, int cols, int convention, const float pose[16], int on_device,
                                 rgbd360_map_stats* stats);
/* The same for n points xyz[3 n] with colours rgb3[3 n] (may be NULL) in the frame's coordinates (pcl::transformPointCloud +
 * globalMap += of any cloud, e.g. KFsphere_SLAM.cpp:236, 558).  n == 0 returns 0 and touches nothing. */
int    rgbd360_map_insert_cloud(rgbd360_map* map, const float* xyz, const uint8_t* rgb3, long long n, const float pose[16],
                                int on_device, rgbd360_map_stats* stats);
/* occupied voxels */
long long rgbd360_map_size(rgbd360_map* map);
int    rgbd360_map_clear(rgbd360_map* map);
/* The filtered map (what filterVoxel leaves in viewer.globalMap, OdometryRGBD360.cpp:268): per voxel the centroid xyz[3], colour
 * rgb3[3], count and key key3[3] = (i_x, i_y, i_z); any pointer may be NULL.  Returns the map's size and writes min(size, max_out)
 * records.  _extract: host arrays, sorted ascending by (i_z, i_y, i_x) -- the order of PCL's idx = i0 + i1 dx + i2 dx dy.
 * _extract_dev: device arrays, unsorted (which records are written when max_out < size is not defined).  Negative: an error. */
long long rgbd360_map_extract(rgbd360_map* map, long long max_out, float* xyz, uint8_t* rgb3, int32_t* count, int32_t* key3);
long long rgbd360_map_extract_dev(rgbd360_map* map, long long max_out, float* xyz, uint8_t* rgb3, int32_t* count, int32_t* key3);

/* ---- editing the map: exact removal, re-posing, rehash and census (csrc/map_edit.h) ----------------------------------------------
 * The reference's SLAM programs optimise their keyframe poses continuously and redraw the map from the corrected poses
 * (SphereGraphSLAM.cpp, KFsphere_SLAM.cpp: optimizer.optimizeGraph(), getPoses(Map.vOptimizedPoses)); odometry against a local map
 * needs old frames to leave it.  The sums are integers and steps 1-5 of an insertion are a pure function of (point, box, pose, leaf),
 * so subtracting the same integer terms undoes an insertion EXACTLY, whatever was inserted in between.
 * Removal, per point: steps 1-5 of the map's definition above, the same bits; then count -= 1, S_k -= llrint((double)w_k * 1048576.0),
 * S_c -= colour_c (the colour iff rgb is given, mirroring insert).  The lookup is read-only: removal never claims a slot.  A slot whose
 * count reaches 0 keeps its key (a tombstone: linear probing needs the run intact); extract, render and both alignments treat it as
 * absent, rgbd360_map_size does not count it, a later insert of that voxel revives it, rgbd360_map_rehash drops it.
 * The contract: the caller removes what it inserted -- the same data, pose, convention and box on a map of the same leaf -- and that
 * insert did not return RGBD360_MAP_FULL (which of its points were dropped is not recorded).  Then the result is exact and does not
 * depend on the order of points or workgroups: the map is, bit for bit, the map that never saw the removed frame.
 * Outside the contract the call is still memory-safe and no count ever wraps: points whose voxel is not in the table are counted in
 * n_missing and nothing is subtracted for them; a voxel asked for more points than it holds gives what it holds (the decrement of the
 * count word is a compare-and-swap loop clamped to the current count), the rest is refused, counted in n_underflow, and the sums are
 * left alone: per voxel n_removed = min(held, asked), whatever the order of points and workgroups.  If either counter is non-zero the call returns RGBD360_MAP_MISMATCH with a message: the counts stay
 * non-negative, but the map's content is then unspecified (sums and counts no longer belong together) and the caller should clear it.
 * n_removed + n_missing + n_underflow = the points that passed steps 1-4; n_voxels_emptied: voxels whose count reached 0 in this call;
 * n_voxels: the map's size after it.
 * Carving (rgbd360_map_carve below) is a lossy edit outside this contract: a carved voxel forgets its points.  Removing or moving a frame
 * that fed a carved voxel reports those points in n_underflow and returns RGBD360_MAP_MISMATCH; while the voxel was not revived in between
 * nothing is subtracted for them and the map stays consistent (n_inconsistent == 0 in the census); once it was revived the content is
 * unspecified as above. */
typedef struct { long long n_valid, n_box_rejected, n_out_of_range, n_removed, n_missing, n_underflow, n_voxels_emptied, n_voxels; } rgbd360_map_edit_stats;
/* Arguments, refusals and empty inputs as for rgbd360_map_insert_sphere / _cloud.  0, RGBD360_MAP_MISMATCH, or negative. */
int    rgbd360_map_remove_sphere(rgbd360_map* map, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                                 int depth_type, int rows, int cols, int convention, const float pose[16], int on_device,
                                 rgbd360_map_edit_stats* stats);
int    rgbd360_map_remove_cloud(rgbd360_map* map, const float* xyz, const uint8_t* rgb3, long long n, const float pose[16],
                                int on_device, rgbd360_map_edit_stats* stats);
/* Re-posing: the source is removed at pose_old and inserted at pose_new -- one upload of a host source, the removal launch and the
 * insert launch on the map's stream, one synchronisation.  Returns the worse (larger) of the two statuses.  If the removal reports a
 * mismatch the insertion is still performed and both statistics are filled: the caller clears the map either way. */
int    rgbd360_map_move_sphere(rgbd360_map* map, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                               int depth_type, int rows, int cols, int convention, const float pose_old[16], const float pose_new[16],
                               int on_device, rgbd360_map_edit_stats* removed, rgbd360_map_stats* inserted);
int    rgbd360_map_move_cloud(rgbd360_map* map, const float* xyz, const uint8_t* rgb3, long long n, const float pose_old[16],
                              const float pose_new[16], int on_device, rgbd360_map_edit_stats* removed, rgbd360_map_stats* inserted);
/* Rebuilds the table without tombstones into capacity_voxels slots (rounded up to a power of two; 0 keeps the current number): the
 * compaction, and the way to grow or shrink a map.  A second table of 64 bytes x slots exists until the call returns.  0; -1 for a
 * capacity below the number of occupied voxels or above 2^30 (nothing is allocated); RGBD360_MAP_FULL when a voxel found no slot within
 * the probe bound of the new table, -103 out of memory: in all three cases the map is unchanged.  Afterwards rgbd360_map_bytes reflects
 * the new size; extract, render and both alignments give the bits they gave before (none depends on the table's layout). */
int    rgbd360_map_rehash(rgbd360_map* map, long long capacity_voxels);
/* A read-only scan of the table: its slots, the occupied voxels (count > 0; = rgbd360_map_size), the tombstones, the points the
 * occupied voxels hold, and the slots whose words cannot come from insertions and contract-keeping removals: count == 0 with a non-zero
 * sum, or count > 0 with a colour sum > 255 count or |S_k| >= count * 2^32 (|w| < 4096 in 2^-20 units).  It tells when to rehash
 * (tombstones against occupied voxels) and whether a removal kept the contract: a voxel that empties must have all-zero sums. */
typedef struct { long long n_slots, n_live, n_tombstones, n_points, n_inconsistent; } rgbd360_map_census_counts;
int    rgbd360_map_census(rgbd360_map* map, rgbd360_map_census_counts* out);

/* ---- point-to-point ICP of a frame against the map (csrc/map_align.h) -----------------------------------------------------------
 * The reference's registration programs put a cloud-to-cloud ICP on voxel-filtered clouds next to the dense alignment
 * (RegisterPairRGBD360.cpp:111-118, MethodsRegisterRGBD360.cpp:294-320, OdometryRGBD360.cpp:98-114 and 210-222: filterVoxel, then
 * setInputSource / setInputTarget / align(guess); OdometryKeyFrame360.cpp:124-140).  Here the target is the resident map: the nearest
 * neighbour of a point is the nearest voxel CENTROID among the 3 x 3 x 3 cells around the point, a bounded number of hash probes, and
 * the Gauss-Newton loop runs on the device with one stream synchronisation per alignment.  Per source point at the current pose T
 * (16 floats, column-major, world <- frame):
 *   1 steps 1-5 of the map's definition above (point, the map's box, pose, range, voxel index i), bit for bit; skipped, box-rejected
 *     and out-of-range points are counted as in rgbd360_map_stats and contribute nothing.
 *   2 candidates: the centre cell i first, then the other 26 cells i + (dx, dy, dz) in the order of three nested loops, dz outermost
 *     and dx innermost, each ascending over -1, 0, 1 (ascending keys).  A cell is a candidate if it is in the table with
 *     count >= min_count.  A read-only lookup ends at the first empty slot or after the table's probe bound (2048 slots, the whole
 *     table when it is smaller).  A neighbour index outside the 21-bit key range is no candidate; it is never wrapped.
 *   3 centroid c_k = (float)((double)S_k / ((double)count * 1048576.0)), the read-out's expression.
 *   4 distance e_k = w_k - c_k, d2 = (e_x e_x + e_y e_y) + e_z e_z in float32, every operation rounded on its own.  The match is the
 *     candidate of smallest d2; a later candidate replaces the current one only if it is strictly smaller (a tie goes to the earlier
 *     one).  It is kept iff d2 <= max_dist * max_dist (the product in float32).
 *   5 sums over the kept matches in float64, every term formed in double from the float32 w and e: n, sum w (3), sum w_j w_k for
 *     j <= k (xx, xy, xz, yy, yz, zz), sum e (3), sum w x e (3), sum (e_x e_x + e_y e_y) + e_z e_z -- 17 in all.  No floating-point
 *     atomics: a workgroup reduces its points into one partial row and the rows are added in ascending order, so the sums are the
 *     same from run to run.
 *   6 step: J = [I | -[w]x], the increment pose <- pseudo_exp(v, omega) pose; H = sum J^T J and g = sum J^T e assembled from the 17
 *     sums in double, cast to float32, then the step of the dense alignment (csrc/gn_math.h, gn::step with lambda 0).
 *     rank(H) != 6: RGBD360_ILL_POSED, pose_out = the last pose.  n < min_matches: RGBD360_NO_VALID_PIXELS.  Converged when
 *     v.v <= eps and omega.omega <= eps in float32 after the step is applied (a stated simplification of PCL's
 *     setTransformationEpsilon).  At most max_iters steps (the reference: 10).
 *   7 one more evaluation at pose_out gives n_matched, fitness = sum e.e / n (PCL's getFitnessScore over the kept matches), hessian
 *     and gradient (and NO_VALID_PIXELS when n < min_matches there and nothing else was reported).
 * max_dist must lie in (0, leaf]: within that range the 27 cells hold every centroid closer than max_dist (up to rounding at cell
 * faces), so the match is the true nearest centroid; a larger radius would need (2r + 1)^3 probes.  Callers who need a wider basin
 * align against a coarser map first.
 * Differences from the reference, stated: its active choice is pcl::GeneralizedIterativeClosestPoint at 0.3 - 0.4 m over a kd-tree of
 * the other cloud; this is the point-to-point form on the grid, against centroids.  PCL is not part of the reference tree: parity
 * with PCL is unpinned.  The point-to-plane form of the same alignment follows below (rgbd360_map_align_plane_*), GICP's cost with its
 * per-match covariance weighting further down (rgbd360_map_align_gicp_*).  Out of scope: radii above one leaf, several GPUs.  (A
 * coarse-to-fine chain over coarser maps derived from this one: rgbd360_map_align_c2f_* below.) */
typedef struct {
    float max_dist;            /* setMaxCorrespondenceDistance, in (0, leaf]; default: leaf */
    int   max_iters;           /* setMaximumIterations: 10 (OdometryRGBD360.cpp:102) */
    float eps;                 /* on |v|^2 and |omega|^2 of the last step: 1e-6 */
    int   min_count;           /* points a voxel must hold to be a candidate: 1 */
    long long min_matches;     /* kept matches an evaluation must have: 6 */
} rgbd360_map_align_params;
typedef struct {
    int status, iterations, converged;      /* RGBD360_OK / ILL_POSED / NO_VALID_PIXELS; steps applied; 1 when the last step was below eps */
    long long n_valid, n_box_rejected, n_out_of_range, n_matched;      /* of the final evaluation at pose_out */
    double fitness;            /* sum e.e / n_matched of the final evaluation (0 when nothing matched) */
    float hessian[36], gradient[6];         /* column-major 6x6, of the final evaluation */
} rgbd360_map_align_result;
void   rgbd360_map_default_align_params(const rgbd360_map* map, rgbd360_map_align_params* p);
/* A sphere frame (as in rgbd360_map_insert_sphere, without colour) from `guess`.  The map is not changed.  Returns the status (>= 0,
 * also in result->status; result may be NULL); -1 bad arguments, nothing launched: max_dist outside (0, leaf], max_iters < 0 or
 * > 1000, min_count < 1, a NULL depth / guess / pose_out, a bad convention or depth type.  params NULL: the defaults.  An empty image
 * returns RGBD360_NO_VALID_PIXELS with pose_out = guess. */
int    rgbd360_map_align_sphere(rgbd360_map* map, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                const float guess[16], int on_device, const rgbd360_map_align_params* params, float pose_out[16],
                                rgbd360_map_align_result* result);
/* The same for n points xyz[3 n] in the frame's coordinates (the filtered cloud of the reference's call sites). */
int    rgbd360_map_align_cloud(rgbd360_map* map, const float* xyz, long long n, const float guess[16], int on_device,
                               const rgbd360_map_align_params* params, float pose_out[16], rgbd360_map_align_result* result);

/* ---- point-to-plane ICP of a frame against the map (csrc/map_align_plane.h) -----------------------------------------------------
 * Every cloud ICP call site of the reference uses pcl::GeneralizedIterativeClosestPoint, a plane-to-plane cost (OdometryRGBD360.cpp:98-114
 * and 210-222, RegisterPairRGBD360.cpp:111-118, MethodsRegisterRGBD360.cpp:294-320).  Against one centroid per cell of a lattice the
 * point-to-point residual above has a tangential part of up to half a leaf along a wall, which says nothing about the pose and pulls the
 * translation towards the lattice; the distance to a plane fitted to the centroids around the point has none.  The plane is
 * fitted around the posed point from the centroids of the 27 cells the lookup reads anyway (the map's resident per-voxel normals,
 * rgbd360_map_normals below, are fitted around a voxel and are not used here).  Per source point at the current pose T:
 *   1 candidates and match: steps 1-4 of the point-to-point definition above, bit for bit -- the map's steps 1-5, the 27 cells in the
 *     same order, count >= min_count, the read-out's centroid, d2 in float32, a tie to the earlier cell, kept iff d2 <= max_dist^2,
 *     max_dist in (0, leaf].  The winning key and d2 of a point are those of rgbd360_map_align_*.
 *   2 support: over ALL m candidates of step 2 (not only the match) e_j = (double)w - (double)c_j per component; sum e (3) and
 *     sum e e^T (xx, xy, xz, yy, yz, zz) in float64, the candidates in the cells' order.  e_mean = sum e / m (= w - mu, mu the mean of
 *     the centroids), C = sum e e^T / m - e_mean e_mean^T, every operation rounded on its own.  A kept point with m < min_support is
 *     counted in n_unsupported and contributes nothing.
 *   3 plane: with c2 = (C00 + C11) + C22, c1 = ((C00 C11 - C01^2) + (C00 C22 - C02^2)) + (C11 C22 - C12^2), c0 = det C by the first row,
 *     the smallest eigenvalue l0 by Newton's method on l^3 - c2 l^2 + c1 l - c0 from l = 0 (Horner form; at most 12 steps; it ends when
 *     the derivative is not positive or |step| <= 1e-15 c2).  The normal n is the largest (by squared length, the earlier on a tie) of
 *     the cross products rows 0 x 1, 0 x 2, 1 x 2 of C - l0 I, divided by its length.  The middle eigenvalue: s = c2 - l0,
 *     p = c1 - l0 s, l1 = 0.5 (s - sqrt(max(s s - 4 p, 0))).  The point is planar iff the largest squared cross product is > 0, l1 > 0
 *     and l0 <= max_flatness l1; otherwise it is counted in n_nonplanar and contributes nothing (room corners and edges).  Float64,
 *     only + - x / sqrt, no fused multiply-add: host, device and a restatement in IEEE arithmetic agree bit for bit.  The sign of n is
 *     what the cross product gives; nothing depends on it.
 *   4 residual r = (n_x e_mean_x + n_y e_mean_y) + n_z e_mean_z, the distance of w from the plane through mu; row J = [n ; w x n]
 *     (= n^T [I | -[w]x]) for the increment pose <- pseudo_exp(v, omega) pose; float64 from the float32 w and the float64 n.
 *   5 sums over the contributing points in float64, no floating-point atomics, one partial row per workgroup, rows added in ascending
 *     order: n, the 21 upper-triangle terms of sum J J^T, sum J r (6), sum r r, sum e_match . e_match (the point-to-point fitness of the
 *     same matches), and the counters.
 *   6 step, stop tests, statuses and the final pass as in steps 6-7 above: H and g cast to float32, gn::step with lambda 0,
 *     RGBD360_ILL_POSED on rank(H) < 6 (a single wall is ill-posed: the correct answer), RGBD360_NO_VALID_PIXELS when fewer than
 *     min_matches points contribute, converged on v.v <= eps and omega.omega <= eps, one stream synchronisation per alignment.
 *     fitness = sum r r / n, fitness_point = sum e_match . e_match / n, n_matched = n (the contributing points).
 * Differences from GICP, stated: planes on the target side only (the source point is a point) and every contributing point has weight
 * one -- the weighted plane-to-plane cost is rgbd360_map_align_gicp_* below; PCL is not part of the reference tree: parity with PCL is
 * unpinned. */
typedef struct {
    float max_dist;            /* as in rgbd360_map_align_params */
    int   max_iters;
    float eps;
    int   min_count;
    long long min_matches;     /* contributing points an evaluation must have: 6 */
    int   min_support;         /* candidates (occupied cells of the 27) a point's plane needs, 1 .. 27: 5 */
    float max_flatness;        /* largest l0 / l1 of a planar support, >= 0: 0.05 (about 2e-3 for a wall whose centroids lie within 2 mm of
                                  it, about 0.3 for a wall-to-wall corner: settings, not measurements) */
} rgbd360_map_align_plane_params;
typedef struct {
    int status, iterations, converged;
    long long n_valid, n_box_rejected, n_out_of_range, n_matched;      /* of the final evaluation; n_matched: the contributing points */
    double fitness;            /* sum r r / n_matched (0 when nothing contributed) */
    float hessian[36], gradient[6];
    long long n_unsupported, n_nonplanar;   /* kept matches with fewer than min_support candidates / whose support is not planar */
    double fitness_point;      /* sum e.e / n_matched over the same matches: rgbd360_map_align_result.fitness's scale */
} rgbd360_map_align_plane_result;
void   rgbd360_map_default_align_plane_params(const rgbd360_map* map, rgbd360_map_align_plane_params* p);
/* As rgbd360_map_align_sphere / _cloud (arguments, return values, refusals; also -1 for min_support outside 1 .. 27 or a negative or
 * NaN max_flatness).  The map is not changed. */
int    rgbd360_map_align_plane_sphere(rgbd360_map* map, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                      const float guess[16], int on_device, const rgbd360_map_align_plane_params* params, float pose_out[16],
                                      rgbd360_map_align_plane_result* result);
int    rgbd360_map_align_plane_cloud(rgbd360_map* map, const float* xyz, long long n, const float guess[16], int on_device,
                                     const rgbd360_map_align_plane_params* params, float pose_out[16], rgbd360_map_align_plane_result* result);

/* ---- many alignments against the map in lock step (csrc/map_align_batch.h) ---------------------------------------------------------
 * The callers of the alignments above rarely come with one input and one guess: relocalisation tries a lattice of guesses because the
 * basin of one call is about a leaf wide (max_dist <= leaf), a pose-graph correction re-refines the keyframes of a window, a rig brings
 * eight clouds.  One call each is n synchronisations and n x (2 max_iters + 3) launches of a few workgroups.  A batch is n_inputs
 * inputs of one form -- all clouds, or all sphere frames of one geometry (rows, cols, depth_type and convention are given once: the
 * context holds the angle tables of one geometry) -- and n_jobs jobs, each (input index, guess[16]); one params struct holds for all.
 * The definition is the single call: for every job j, poses_out + 16 j, results[j] (the whole struct, hessian and gradient included)
 * and the trace (rgbd360_map_align_batch_trace, rgbd360_hip_diag.h) are byte for byte what rgbd360_map_align_cloud / _sphere
 * (rgbd360_map_align_plane_cloud / _sphere) return on the same map for inputs[jobs[j].input] from jobs[j].guess with the same params.
 * No job's bytes depend on which other jobs are in the batch, on their order or on n_jobs.  The map is not changed.  Statuses are per
 * job: a job that ends early (converged, RGBD360_ILL_POSED, RGBD360_NO_VALID_PIXELS) stops, the others go on; a job on an empty input
 * (n = 0; rows or cols = 0) has RGBD360_NO_VALID_PIXELS, its guess as its pose and a zeroed result, as the single call.  The jobs iterate
 * in lock step: one init launch, max_iters x (evaluation over the workgroups of all jobs, solve with one workgroup per job), the final
 * pass, one copy of all states, ONE synchronisation -- 2 max_iters + 3 launches whatever n_jobs is.  Host inputs are uploaded packed,
 * each once however many jobs use it.
 * Returns 0 when the batch ran (the statuses are in the results; results may be NULL).  Returns -1 with rgbd360_map_last_error set,
 * nothing launched, uploaded or allocated and the outputs untouched, for: what the single calls refuse (of the params, of any input);
 * n_jobs or n_inputs outside 1 .. RGBD360_MAP_BATCH_MAX; a job's input index outside 0 .. n_inputs - 1; a NULL inputs, jobs or
 * poses_out; a batch whose jobs need more than RGBD360_MAP_BATCH_MAX_ROWS workgroups in all (a job of a cloud of n points needs
 * ceil(n / 1024), of a frame rows x ceil(cols / 1024): the partial rows take 304 bytes each); host inputs of more than
 * RGBD360_MAP_BATCH_MAX_UPLOAD bytes packed (each used input once, rounded up to 256 bytes).  A level of a pyramid (rgbd360_map_level) is
 * accepted as the single calls accept it.  Out of scope: generalized and coloured ICP in batch form (the driver is written over the
 * method, as the single loop is), a batched coarse-to-fine chain, clouds and frames mixed or frames of different geometry, parameters per
 * job, per-point outputs, several GPUs. */
#define RGBD360_MAP_BATCH_MAX        1024
#define RGBD360_MAP_BATCH_MAX_ROWS   (1 << 20)
#define RGBD360_MAP_BATCH_MAX_UPLOAD (1ull << 30)
typedef struct { const float* xyz; long long n; } rgbd360_map_batch_cloud;              /* n points xyz[3 n] in the frame's coordinates */
typedef struct { const void* depth; size_t depth_step; } rgbd360_map_batch_frame;       /* a depth image of the batch's geometry */
typedef struct { int input; float guess[16]; } rgbd360_map_batch_job;                   /* column-major, world <- frame */
/* inputs, jobs: host arrays; on_device: the xyz / depth pointers of ALL inputs are device memory.  params NULL: the defaults. */
int    rgbd360_map_align_batch_cloud(rgbd360_map* map, const rgbd360_map_batch_cloud* inputs, int n_inputs, int on_device,
                                     const rgbd360_map_batch_job* jobs, int n_jobs, const rgbd360_map_align_params* params, float* poses_out,
                                     rgbd360_map_align_result* results);
int    rgbd360_map_align_batch_sphere(rgbd360_map* map, const rgbd360_map_batch_frame* inputs, int n_inputs, int depth_type, int rows, int cols,
                                      int convention, int on_device, const rgbd360_map_batch_job* jobs, int n_jobs,
                                      const rgbd360_map_align_params* params, float* poses_out, rgbd360_map_align_result* results);
int    rgbd360_map_align_plane_batch_cloud(rgbd360_map* map, const rgbd360_map_batch_cloud* inputs, int n_inputs, int on_device,
                                           const rgbd360_map_batch_job* jobs, int n_jobs, const rgbd360_map_align_plane_params* params,
                                           float* poses_out, rgbd360_map_align_plane_result* results);
int    rgbd360_map_align_plane_batch_sphere(rgbd360_map* map, const rgbd360_map_batch_frame* inputs, int n_inputs, int depth_type, int rows, int cols,
                                            int convention, int on_device, const rgbd360_map_batch_job* jobs, int n_jobs,
                                            const rgbd360_map_align_plane_params* params, float* poses_out,
                                            rgbd360_map_align_plane_result* results);
/* The winner among n results, host only: eligible are the jobs with status == RGBD360_OK and n_matched >= min_matched; the winner has
 * the largest n_matched, then the smaller fitness, then the smaller index.  -1 when none is eligible, n <= 0 or results is NULL.  This
 * is a policy for the jobs of ONE input from several guesses -- an inlier count; across inputs of different size it says nothing -- and
 * no part of the alignment: a caller with a better criterion reads the results itself. */
int    rgbd360_map_align_best(const rgbd360_map_align_result* results, int n, long long min_matched);
int    rgbd360_map_align_plane_best(const rgbd360_map_align_plane_result* results, int n, long long min_matched);

/* ---- the rig's extrinsics against the map (csrc/rig_calib.h) ------------------------------------------------------------------------
 * Calib360::loadExtrinsicCalibration (Calib360.h:122-131) reads Rt_01.txt .. Rt_08.txt, the rig <- sensor poses that
 * rgbd360_rig_create takes and every rig pose is multiplied by.  This call produces them from what is resident: a map built from posed
 * frames, the point-to-plane evaluation against it and the lock-step batch above.  With refine_poses the same call is a small bundle
 * adjustment of a keyframe window against the map.  The reference's own method (Calibrator::CalibrateRotation / CalibrateTranslation
 * from matched planes of adjacent sensors) is not restated.
 * Inputs: K = n_frames frames and S = n_sensors sensors, 1 <= S <= RGBD360_RIG_CALIB_MAX_SENSORS, K S <= RGBD360_MAP_BATCH_MAX; the
 *   bounds RGBD360_MAP_BATCH_MAX_ROWS / _MAX_UPLOAD apply to the K S inputs as to a batch.  inputs[k S + s] is the cloud of sensor s in
 *   frame k in the sensor's coordinates (n = 0: the sensor has no data in that frame).  poses[16 K]: world <- rig; extrinsics[16 S]:
 *   rig <- sensor; column-major float32, both in/out.
 * Evaluation: P_ks = T_k E_s by gn_math.h's 4 x 4 product in float32, C(r, c) = ((A(r,0) B(0,c) + A(r,1) B(1,c)) + A(r,2) B(2,c)) +
 *   A(r,3) B(3,c).  Input (k, s) is evaluated at P_ks by steps 1-5 of the point-to-plane definition above, bit for bit (the batch's
 *   evaluation launch, unchanged).  Its partial rows added in ascending order give, in float64, n_ks, A_ks (6 x 6, from the 21 upper-
 *   triangle sums), b_ks (sum J r) and sum r r, in the world-left parameterisation P <- pseudo_exp(xi) P.  An input with
 *   n_ks < min_input_matches contributes nothing; n_inputs_used counts the others.
 * Unknowns: epsilon_s per free sensor, E_s <- pseudo_exp(epsilon_s) E_s; with refine_poses delta_k per frame, T_k <- pseudo_exp(delta_k)
 *   T_k.  To first order xi_ks = delta_k + Ad(T_k) epsilon_s, Ad(T) = [[R, [t]x R], [0, R]] for twists ordered (v, omega), formed in
 *   float64 from the float32 pose.
 * Normal equations, float64 with + - x / sqrt and no contraction, sums of products ascending from 0.0, sums over s and over k ascending
 *   over the contributing inputs: C_ks = A_ks Ad_k, G_ks = Ad_k^T C_ks, gs_ks = Ad_k^T b_ks; F_k = sum_s A_ks, f_k = -(sum_s b_ks);
 *   G_s = sum_k G_ks, g_s = -(sum_k gs_ks).  lambda >= 0 (default 0) replaces every diagonal entry d of F_k and of the reduced matrix
 *   by d + lambda d; there is no adaptive damping.
 * Solve: with refine_poses every frame with a contributing input is eliminated: L_k the Cholesky factor of F_k (column j ascending;
 *   element (i, j), i >= j: F_ij - sum_{p < j} L_ip L_jp with p ascending; the diagonal's square root, the others divided by it),
 *   z_k = L_k^-1 f_k and W_ks = L_k^-1 C_ks by forward substitution.  A frame without a contributing input is skipped and left untouched
 *   (n_frames_skipped).  The reduced matrix over the F free sensors, 6 F x 6 F, lower triangle: M_ij = [same sensor] sum_k G_ks(i, j) -
 *   sum_k (W_k,si^T W_k,sj)(i, j), rhs_i = g_s(i) - sum_k (W_k,si^T z_k)(i); the G sum first, then frame after frame the six products of
 *   a frame summed from 0.0 and subtracted.  (Of the nearly symmetric G_ks the lower triangle is read.)  Cholesky as above, L y = rhs
 *   and L^T epsilon = y column by column, then L_k^T delta_k = z_k - sum_s W_ks epsilon_s.  F <= 15 with a fixed sensor (90 x 90), 16
 *   without; the packed triangle of 96 x 97 / 2 doubles lies in one workgroup's LDS.
 *   Pivot rule, a setting: a pivot <= 1e-12 x its undamped diagonal entry (or a NaN) ends the call with RGBD360_ILL_POSED; it holds for
 *   the frame blocks and the reduced matrix.  A free sensor without any contributing input is such a pivot.
 *   The updates are cast to float32 and applied with gn_math.h's pseudo-exponential and 4 x 4 product; the new P_ks are the inputs' poses
 *   of the next evaluation.
 * Gauge: T_k -> T_k G^-1, E_s -> G E_s changes no residual.  With refine_poses a fixed_sensor in 0 .. S - 1 is required (-1 otherwise);
 *   without it fixed_sensor may be -1: the sensors decouple, M is block diagonal and a sensor's extrinsic does not depend on which other
 *   sensors are in the call (the stop test and the statuses are the call's).
 * Stop and statuses: converged when v.v <= eps and omega.omega <= eps for every block's float32 update; at most plane.max_iters steps,
 *   then one final evaluation at the returned poses, of which n_matched, cost = sum r r, fitness = cost / n_matched and the per-sensor
 *   records are.  RGBD360_NO_VALID_PIXELS when the contributing points of all inputs are fewer than plane.min_matches.  The last iterate
 *   is returned, as the single loops do.  The iterates need not settle: the evaluation's floor is about a hundredth of a leaf.
 * Schedule: one init launch, max_iters x (the batched evaluation + 3 solve launches), the final pass, one copy, ONE synchronisation:
 *   4 max_iters + 5 launches whatever K and S are.  No floating-point atomics, no inline assembly.  The map is not changed; a level of
 *   a pyramid is accepted as the single calls accept it; callers chain coarse -> fine by calling again.
 * The call estimates extrinsics against a map built with the OLD extrinsics: CLAMS alternates calibrate, re-map (rgbd360_map_move /
 * _merge), repeat; the alternation is the caller's loop (examples/calibrate_extrinsics.cpp).
 * Returns the status.  Returns -1 with rgbd360_map_last_error set, nothing launched and the outputs untouched, for: what the batch
 * refuses; K < 1, S outside 1 .. 16, K S > RGBD360_MAP_BATCH_MAX; NULL inputs, poses or extrinsics; poses or extrinsics that are not
 * finite; refine_poses without a fixed_sensor; fixed_sensor outside -1 .. S - 1; lambda negative or not finite; min_input_matches < 1.
 * The map's robust setting for the plane method (rgbd360_map_set_align_robust) is NOT honoured: the calibration keeps the quadratic kernels.
 * Out of scope: the reference's control-plane method, per-sensor intrinsics, robust weights, sphere-frame inputs, several GPUs. */
#define RGBD360_RIG_CALIB_MAX_SENSORS 16
typedef struct { rgbd360_map_align_plane_params plane; int refine_poses, fixed_sensor; float lambda; long long min_input_matches; } rgbd360_rig_calib_params;
typedef struct { int status, iterations, converged, n_inputs_used, n_frames_skipped; long long n_matched; double cost, fitness; } rgbd360_rig_calib_result;
typedef struct { long long n_matched; double cost; float hessian[36], gradient[6]; } rgbd360_rig_calib_sensor;   /* G_s and sum_k gs_ks, final evaluation, rig frame */
/* the point-to-plane defaults; refine_poses 0, fixed_sensor -1, lambda 0, min_input_matches 6 */
void   rgbd360_map_default_rig_calib_params(const rgbd360_map* map, rgbd360_rig_calib_params* p);
/* inputs: a host array of K S clouds, frame-major; on_device: the xyz pointers of ALL inputs are device memory.  params NULL: the
 * defaults.  result and sensors (S records) may be NULL. */
int    rgbd360_map_calibrate_rig_clouds(rgbd360_map* map, const rgbd360_map_batch_cloud* inputs, int n_frames, int n_sensors, int on_device,
                                        float* poses, float* extrinsics, const rgbd360_rig_calib_params* params, rgbd360_rig_calib_result* result,
                                        rgbd360_rig_calib_sensor* sensors);
/* The same from K S pinhole depth images of one geometry (depth_type 0 uint16 millimetres, z = 0.001f (float)v; 1 float32 metres), each
 * turned into a packed cloud of rows cols points on the device by one launch over all images: the ray of pixel (v, u) is
 * f = (((float)u - cx) / fx, ((float)v - cy) / fy, 1), the ray of rgbd360_depth_trainer_accumulate_map, every float32 operation rounded
 * on its own, the point (z f_x, z f_y, z).  A pixel without a measurement (0; not finite, zero or negative) becomes a NaN triple, which
 * the evaluation skips.  The call then proceeds exactly as _clouds on device memory.  Also refused: a pinhole that is not finite, fx or
 * fy zero, a bad depth_type or image size, a NULL image, a row step shorter than a row. */
int    rgbd360_map_calibrate_rig_depth(rgbd360_map* map, const rgbd360_map_batch_frame* depth, int depth_type, int rows, int cols, float fx, float fy,
                                       float cx, float cy, int n_frames, int n_sensors, int on_device, float* poses, float* extrinsics,
                                       const rgbd360_rig_calib_params* params, rgbd360_rig_calib_result* result, rgbd360_rig_calib_sensor* sensors);
/* Rt_0N.txt, N = 1 .. n_sensors, in `dir`: four lines of four numbers, row by row, printed with %.9g (a float32 survives the round trip):
 * the layout Calib360::loadExtrinsicCalibration reads.  Host only.  0; 1 a file could not be written; -1 bad arguments. */
int    rgbd360_rig_save_extrinsics(const float* extrinsics, int n_sensors, const char* dir);

/* ---- the map rendered as a spherical frame (csrc/map_render.h) -------------------------------------------------------------------
 * The reference looks at its global map in a PCL window (viewer.globalMap, OdometryRGBD360.cpp:242-268) and aligns new frames against
 * keyframes (OdometryKeyFrame360.cpp).  Here the map is turned back into what the dense alignment takes: a full-sphere RGB-D panorama
 * at a pose, a z-buffered splat of the table.  depth and rgb go straight into rgbd360_set_target (depth_type 1) -- frame-to-model
 * alignment against everything inserted so far -- and the panorama is the map's picture.  The pixel grid is that of rgbd360_set_target
 * for an image of rows x cols (RPI.h:4567-4582).  pose: 16 floats, column-major, world <- frame, as for every map entry.
 *   1 inverse pose  formed once on the host: Rinv = R^T, tinv_k = -(R_0k t_x + R_1k t_y + R_2k t_z) evaluated in double from the float32
 *                   inputs, summed left to right, rounded to float32.  R is taken to be a rotation; this is not checked.
 *   2 voxel         every occupied voxel with count >= min_count takes part; centroid c_k = (float)((double)S_k / ((double)count *
 *                   1048576.0)) and colour S_c / count are the read-out's expressions, bit for bit.
 *   3 projection    the dense alignment's warp in the device arithmetic (the one rgbd360_set_index_arithmetic(ctx, 0) selects, the
 *                   oracle's math_mode 1) at the pose of step 1 with c as the source point: target row r', column c', d^2 and visibility.
 *                   dist = the correctly rounded float32 square root of d^2.  A voxel is skipped and counted in n_near when it is not
 *                   visible, when dist is not finite or when dist < near (default: leaf, which drops the voxel the camera sits in).
 *   4 footprint     half-width in pixels h = min(max_half, (int)(foot * (1 / dist))), the reciprocal correctly rounded, the product in
 *                   float32, the cast truncating; foot = (splat * leaf) * angle_res_inv, both products in float32 in that order.  The voxel
 *                   covers the rows r' - h .. r' + h clipped to [0, rows) and the columns c' - h .. c' + h modulo cols (the panorama is
 *                   closed in theta); when 2 h + 1 >= cols every column once.  splat = 0 gives single pixels.
 *   5 visibility    per pixel the voxel of smallest dist wins (positive float32 values compared by their bit patterns); on equal bits
 *                   the smaller packed key (i_z, i_y, i_x from the top, the table's own key).  A slot index, an arrival order or a thread
 *                   never decides: the image does not depend on the order of insertion, on the table's capacity or on the run.
 *   6 outputs       row-major rows x cols, any pointer may be NULL: depth float32 = the winner's dist, 0 where nothing landed; rgb 8UC3
 *                   tightly packed = the winner's colour; count int32 = the winner's point count (the hole mask: 0 in holes); key3
 *                   3 x int32 = (i_x, i_y, i_z), 0 in holes.  The statistics are exact integers.
 * Stated limitations: the depth across a footprint is the centroid's dist (flat-shaded discs); the footprint is a square in pixels and
 * is not widened towards the poles; silhouettes grow by the footprint; the render does not use the map's surface normals.  Out of scope:
 * anti-aliased or normal-shaded splats.  (The first surface along a ray, and with it any other view: rgbd360_map_raycast below; the
 * surface with its normals: rgbd360_map_raycast_surface below.) */
typedef struct {
    int   min_count;           /* points a voxel must hold to be drawn: 1 */
    float near;                /* voxels closer than this are skipped: leaf */
    float splat;               /* footprint in leaves at unit distance, >= 0: 1.0 */
    int   max_half;            /* largest footprint half-width in pixels, 0 .. 64: 8 */
} rgbd360_map_render_params;
typedef struct { long long n_voxels, n_below_min_count, n_near, n_splatted, n_pixels_covered; } rgbd360_map_render_stats;
void   rgbd360_map_default_render_params(const rgbd360_map* map, rgbd360_map_render_params* p);
/* Host outputs; the call waits for them.  0; -1 bad arguments, nothing launched: a NULL pose, rows or cols negative or outside what a
 * level of the dense alignment accepts (2 x 8 .. < 16 Mpx, both sides < 32768), min_count < 1, max_half outside 0 .. 64, splat or near
 * negative or not finite.  params NULL: the defaults.  An empty map or rows * cols == 0 returns 0 with zero-filled outputs and
 * statistics and launches no kernel.  A render never writes the table; the two work planes (12 bytes per pixel) belong to the map. */
int    rgbd360_map_render_sphere(rgbd360_map* map, int rows, int cols, const float pose[16], const rgbd360_map_render_params* params,
                                 float* depth, uint8_t* rgb, int32_t* count, int32_t* key3, rgbd360_map_render_stats* stats);
/* The same into device arrays on the map's device (stats_dev too): enqueued on the context's stream, the call does not wait. */
int    rgbd360_map_render_sphere_dev(rgbd360_map* map, int rows, int cols, const float pose[16], const rgbd360_map_render_params* params,
                                     float* depth_dev, uint8_t* rgb_dev, int32_t* count_dev, int32_t* key3_dev,
                                     rgbd360_map_render_stats* stats_dev);

/* ---- ray casting through the map (csrc/map_raycast.h) ---------------------------------------------------------------------------
 * What a map is usually asked: the first surface along a ray.  A list of rays (pinhole views, single beams, the line of sight between
 * two keyframe poses), or every pixel of the dense alignment's full-sphere panorama at a pose: the model image of frame-to-model
 * alignment as a per-pixel first hit where rgbd360_map_render_sphere splats.  The result is a function of the voxel set and the ray
 * alone: it does not depend on the order of insertion, on the table's capacity, on slot indices or on the run.  A ray cast never writes
 * the table.  All traversal arithmetic is float64 + - x / without contraction; o, d, the centroid and inv_leaf = 1.0f / leaf enter as
 * the doubles of their float32 values.
 *   1 ray         origin o and direction d, float32 triples in world coordinates; the point at t >= 0 is o + t d.  d need not be a unit
 *                 vector: t is in units of |d|.  A component not finite, or d = 0: status RGBD360_RAY_BAD, nothing traversed.
 *   2 grid        g_k = o_k inv_leaf, u_k = d_k inv_leaf (exact products), r_k = 1 / u_k.  The ray meets the cell boundary b of axis k
 *                 (the plane between the cells b - 1 and b; cells are [i, i + 1)) at T_k(b) = (b - g_k) r_k -- two roundings, a function
 *                 of b alone and never a running sum, so a boundary's time does not depend on the path to it.  u_k = 0: T_k = +inf.
 *   3 clip        against the box of the live voxels, the cells lo_k .. hi_k (the integer key bounds over the voxels with count > 0, a
 *                 function of the voxel set): t0 = max(0, near_k), t1 = min(far_k) over the axes with u_k != 0, near / far the smaller
 *                 / larger of T_k(lo_k) and T_k(hi_k + 1); an axis with u_k = 0 misses unless lo_k <= g_k < hi_k + 1.  t0 > t1:
 *                 status RGBD360_RAY_MISS_BOX, zero steps.
 *   4 start       the cell i_k = floor(g_k + t0 u_k), clamped to lo_k .. hi_k; t_in = t0.
 *   5 per cell    (Amanatides-Woo)  t_in > t_max: status RGBD360_RAY_T_MAX.  max_steps cells visited: RGBD360_RAY_MAX_STEPS.  Else the
 *                 cell is counted as a step; t_out = the smallest T_k(next boundary of axis k); on equal times the LOWEST axis index
 *                 steps (x before y before z).  The cell is a candidate if its voxel holds count >= min_count points; removed voxels
 *                 (tombstones) and empty cells are air.  c = the read-out's float32 centroid, bit for bit;
 *                 s = (((c_x - o_x) d_x + (c_y - o_y) d_y) + (c_z - o_z) d_z) / ((d_x d_x + d_y d_y) + d_z d_z), the centroid's
 *                 projection on the ray; t_hit = min(max(s, t_in), t_out).  The candidate is rejected, and the traversal goes on, when
 *                 t_hit < t_min (default: leaf, which drops the voxel the camera sits in) or when the centroid lies farther than
 *                 max_offset leaves from the ray: ((e_x e_x + e_y e_y) + e_z e_z) (inv_leaf inv_leaf) > max_offset max_offset with
 *                 e_k = (c_k - o_k) - s d_k (default +inf: the test is off).  Else: status RGBD360_RAY_HIT.
 *   6 advance     the axis of t_out moves one cell by the sign of u_k; a cell outside lo .. hi ends the ray with RGBD360_RAY_LEFT_BOX
 *                 (the box lies inside the key range |i| < 2^20, so no index outside that range is ever looked up).  t_in = t_out.
 *   7 outputs     per ray, any pointer may be NULL: t float32 = (float)t_hit, 0 on a miss (the render's hole convention); key3 3 x int32
 *                 = (i_x, i_y, i_z); count int32; rgb3 = the read-out's colour S_c / count; status int32.  All zero on a miss but status.
 *                 The statistics are exact integers.  n_steps: cells visited.  n_lookups: lookups in the voxel table, the one number
 *                 that depends on the form of the traversal (the coarse layer looks up live cells only; the plain form every cell).
 * The coarse layer (bricks of 8^3 cells: brick key -> 512-bit mask, plus the live-key bounds) belongs to the map, is built on the first
 * ray cast after the map was written (two scans of the table; that call waits for the first) and changes no output bit.
 * Stated limitations: cells are cubes -- a ray that clips an occupied cell's corner hits it unless max_offset is set; the depth inside a
 * cell is the centroid's projection, a staircase of cells (the depth on the plane fitted around the hit voxel, and its normal:
 * rgbd360_map_raycast_surface below); the layer costs extra device memory per map (12 bytes per brick-table slot, a power of two
 * >= 2 x voxels, and 64 bytes per occupied brick).  The same traversal, not ending at a candidate, is the line of sight of
 * rgbd360_map_observe_* below (free-space votes and carving).  Out of scope: shaded output. */
enum { RGBD360_RAY_MISS_BOX = 0, RGBD360_RAY_HIT = 1, RGBD360_RAY_LEFT_BOX = 2, RGBD360_RAY_T_MAX = 3, RGBD360_RAY_MAX_STEPS = 4, RGBD360_RAY_BAD = 5 };
typedef struct {
    int   min_count;           /* points a voxel must hold to stop a ray: 1 */
    float t_min;               /* hits nearer than this are passed through: leaf */
    float t_max;               /* the ray ends where a cell's entry lies beyond this: +inf */
    float max_offset;          /* largest distance of the centroid from the ray, in leaves: +inf (off) */
    int   max_steps;           /* cells a ray may visit, 1 .. 2^23: 8192 */
} rgbd360_map_raycast_params;
typedef struct {
    long long n_rays, n_hits, n_miss_box, n_left_box, n_t_max, n_max_steps, n_bad_rays, n_steps, n_lookups;
} rgbd360_map_raycast_stats;
void   rgbd360_map_default_raycast_params(const rgbd360_map* map, rgbd360_map_raycast_params* p);
/* n rays: origins and dirs are n x 3 float32.  on_device 0: every array is host memory; 1: origins, dirs and the five outputs are
 * device arrays on the map's device.  stats is host memory and the call waits in both cases.  0; -1 bad arguments, nothing launched:
 * n < 0 or >= 2^31, origins or dirs NULL with n > 0, min_count < 1, t_min negative or not finite, t_max or max_offset negative or not
 * a number, max_steps outside 1 .. 2^23.  params NULL: the defaults.  An empty map or n == 0 returns 0 with zero-filled outputs and
 * statistics and launches no kernel. */
int    rgbd360_map_raycast(rgbd360_map* map, long long n, const float* origins, const float* dirs, int on_device,
                           const rgbd360_map_raycast_params* params, float* t, int32_t* key3, int32_t* count, uint8_t* rgb3, int32_t* status,
                           rgbd360_map_raycast_stats* stats);
/* The panorama: the pixel grid, the pose convention, the output planes and the argument checks of rgbd360_map_render_sphere.  The ray of
 * pixel (r, c) starts at the pose's translation; its direction is the pixel's unit vector f = (sin phi_r, (-cos phi_r) sin theta_c,
 * (-cos phi_r) cos theta_c) in float32 -- the dense alignment's source point at depth 1 (RPI.h:4556-4571), with theta_c = c angle_res and
 * phi_r = (half_nRows - r) angle_res in float32 and their sine and cosine taken in double and rounded to float32 (at most an ulp from
 * the alignment's own tables, and no function of a C library's sinf) -- rotated by the pose, d_k = (R_k0 f_x + R_k1 f_y) + R_k2 f_z, every
 * product and sum rounded to float32 on its own.  depth = t; depth and rgb go straight into rgbd360_set_target with depth_type 1. */
int    rgbd360_map_raycast_sphere(rgbd360_map* map, int rows, int cols, const float pose[16], const rgbd360_map_raycast_params* params,
                                  float* depth, uint8_t* rgb, int32_t* count, int32_t* key3, rgbd360_map_raycast_stats* stats);
/* The same into device arrays on the map's device (stats_dev too): enqueued on the context's stream; the call waits only where the
 * coarse layer has to be rebuilt. */
int    rgbd360_map_raycast_sphere_dev(rgbd360_map* map, int rows, int cols, const float pose[16], const rgbd360_map_raycast_params* params,
                                      float* depth_dev, uint8_t* rgb_dev, int32_t* count_dev, int32_t* key3_dev,
                                      rgbd360_map_raycast_stats* stats_dev);

/* ---- surface normals of the map (csrc/map_normals.h) -------------------------------------------------------------------------------
 * One normal per voxel, fitted to the centroids around it, kept resident next to the table; a read-out with normals and a ray cast that
 * returns the surface -- a normal per hit and a depth on the fitted plane instead of the staircase of cell centroids -- are its two
 * consumers.  The normal of a voxel is a function of the voxel set and of (min_count, min_support, max_flatness) alone: it does not
 * depend on the order of insertion, on the table's capacity, on a slot index or on the run.  Nothing here writes the table.
 *   1 voxel       v with count >= min_count; w = the read-out's float32 centroid of v.  Below min_count: status RGBD360_NORMAL_NONE.
 *   2 support     steps 2-3 of the point-to-plane definition above with v's own key as the centre and w as the point: the candidates are
 *                 the voxels with count >= min_count among the 27 cells, the centre first, then dz / dy / dx ascending; v itself is one
 *                 (e = 0); tombstones and empty cells are absent; a neighbour index outside the 21-bit key range does not exist and is
 *                 not looked up.  The nine sums in float64, e_mean and C as there.  m < min_support: RGBD360_NORMAL_UNSUPPORTED.
 *   3 plane       the plane function of step 3 there (rgbd360_map_plane_fit, the diagnostics header).  Not planar:
 *                 RGBD360_NORMAL_NONPLANAR.  Else RGBD360_NORMAL_OK.
 *   4 normal      n32_k = (float)n_k; canonical sign: the component of n32 of largest magnitude (the earliest on a tie) is positive,
 *                 otherwise all three are negated.  Every consumer uses n32 widened to double.  curvature = (float)(l0 / c2), c2 =
 *                 (C00 + C11) + C22 (lambda_min over the sum of the eigenvalues), 0 when c2 is not positive.  The normal is zero unless
 *                 the status is OK; the curvature is zero unless it is OK or NONPLANAR.
 * The layer: 16 bytes per table slot of device memory beside the table (a quarter of the table; rgbd360_map_bytes stays the table's
 * size), owned by the map, built by the first call that needs it -- one launch over the slots -- and reused until the map is written
 * or one of the three parameters differs.  max_shift is no parameter of the layer.
 * Out of scope: shaded or anti-aliased output; normals from the points inside a voxel (insertion is unchanged); neighbourhoods wider
 * than the 27 cells; camera-frame normals (normals are in world coordinates); rgbd360_map_align_plane_* on the resident normals (its
 * plane is fitted around the posed point, not around a voxel, and its bits are pinned). */
enum { RGBD360_NORMAL_NONE = 0, RGBD360_NORMAL_OK = 1, RGBD360_NORMAL_UNSUPPORTED = 2, RGBD360_NORMAL_NONPLANAR = 3 };
typedef struct {
    int   min_count;           /* points a voxel must hold to have a normal and to support one: 1 */
    int   min_support;         /* candidates (occupied cells of the 27) a normal needs, 1 .. 27: 5 */
    float max_flatness;        /* largest l0 / l1 of a planar support, >= 0: 0.05 (rgbd360_map_align_plane_params) */
    float max_shift;           /* surface cast only: how far, in leaves, the plane point may lie from the hit voxel's centroid, >= 0: 2.0
                                  (a setting, not a measurement: on oblique noisy walls 1.5 still rejected 0.5 - 1.7 % of the hits of a probe
                                  and 2.0 none; 0 keeps every depth of the plain cast) */
} rgbd360_map_normal_params;
typedef struct { long long n_voxels, n_below_min_count, n_unsupported, n_nonplanar, n_normals; } rgbd360_map_normal_stats;
void      rgbd360_map_default_normal_params(const rgbd360_map* map, rgbd360_map_normal_params* p);
/* One record per voxel with count > 0, in the manner of rgbd360_map_extract but in NO specified order (key3 and xyz come along): returns
 * the voxel count; at most max_out records are written; any output pointer may be NULL.  xyz [3], count and key3 [3] are the read-out's
 * bits; normal [3], curvature and status as defined above.  viewpoint (3 floats, world; may be NULL): an OK normal is negated when
 * ((n_x e_x + n_y e_y) + n_z e_z) < 0 for e = viewpoint - w in double, so that it faces the viewpoint; NULL keeps the canonical sign.
 * stats (may be NULL): exact counts over the whole map, whatever max_out.  Host arrays; the call waits.  -1, nothing launched and no
 * output touched: min_count < 1, min_support outside 1 .. 27, max_flatness or max_shift negative or NaN, a viewpoint that is not finite,
 * max_out < 0.  params NULL: the defaults.  An empty map returns 0 with zero statistics and launches no kernel. */
long long rgbd360_map_normals(rgbd360_map* map, const rgbd360_map_normal_params* params, const float viewpoint[3], long long max_out, float* xyz,
                              float* normal, float* curvature, int32_t* status, int32_t* count, int32_t* key3, rgbd360_map_normal_stats* stats);
/* The same into device arrays on the map's device (stats_dev too; params and viewpoint are host memory): enqueued on the context's
 * stream, the call does not wait. */
long long rgbd360_map_normals_dev(rgbd360_map* map, const rgbd360_map_normal_params* params, const float viewpoint[3], long long max_out,
                                  float* xyz_dev, float* normal_dev, float* curvature_dev, int32_t* status_dev, int32_t* count_dev,
                                  int32_t* key3_dev, rgbd360_map_normal_stats* stats_dev);
/* The surface cast.  Rays, checks, refusals (and those of the normal parameters above), empty inputs, output planes, pose convention and
 * stream behaviour are those of rgbd360_map_raycast / _sphere / _sphere_dev; the traversal and the hit decision (with the centroid's
 * projection) are the same, so status, key3, count, rgb and stats are byte-equal to the plain entry's on the same rays.  On a hit whose
 * voxel is RGBD360_NORMAL_OK, with n = n32 widened, c the voxel's centroid, all in double without contraction:
 *   q = (n_x d_x + n_y d_y) + n_z d_z; normal = n32, negated when q > 0 (it faces the ray's origin).  If q != 0:
 *   t_p = ((n_x (c_x - o_x) + n_y (c_y - o_y)) + n_z (c_z - o_z)) / q, f_k = (o_k + t_p d_k) - c_k; the plane depth is taken iff
 *   t_p >= t_min and ((f_x f_x + f_y f_y) + f_z f_z) (inv_leaf inv_leaf) <= max_shift max_shift -- it is NOT clamped to the cell (clamping
 *   gives the gain away) -- and then t = (float)t_p.
 * Every other hit keeps the plain entry's t bit for bit and has a zero normal; a miss has zeros.  normal: 3 floats per ray / pixel, world
 * coordinates.  n_on_plane (may be NULL; host memory where stats is, device memory for the _dev entry): the rays whose plane depth was
 * taken.  The sphere variant's depth and rgb go straight into rgbd360_set_target. */
int       rgbd360_map_raycast_surface(rgbd360_map* map, long long n, const float* origins, const float* dirs, int on_device,
                                      const rgbd360_map_raycast_params* ray_params, const rgbd360_map_normal_params* normal_params, float* t,
                                      float* normal, int32_t* key3, int32_t* count, uint8_t* rgb3, int32_t* status, long long* n_on_plane,
                                      rgbd360_map_raycast_stats* stats);
int       rgbd360_map_raycast_surface_sphere(rgbd360_map* map, int rows, int cols, const float pose[16], const rgbd360_map_raycast_params* ray_params,
                                             const rgbd360_map_normal_params* normal_params, float* depth, float* normal, uint8_t* rgb,
                                             int32_t* count, int32_t* key3, long long* n_on_plane, rgbd360_map_raycast_stats* stats);
int       rgbd360_map_raycast_surface_sphere_dev(rgbd360_map* map, int rows, int cols, const float pose[16],
                                                 const rgbd360_map_raycast_params* ray_params, const rgbd360_map_normal_params* normal_params,
                                                 float* depth_dev, float* normal_dev, uint8_t* rgb_dev, int32_t* count_dev, int32_t* key3_dev,
                                                 long long* n_on_plane_dev, rgbd360_map_raycast_stats* stats_dev);

/* ---- generalized ICP against the map (csrc/map_align_gicp.h) ---------------------------------------------------------------------
 * The cost the reference's cloud ICP call sites actually minimise: pcl::GeneralizedIterativeClosestPoint on two voxel-filtered clouds
 * (OdometryRGBD360.cpp:98-114 and 210-222, RegisterPairRGBD360.cpp:111-118, MethodsRegisterRGBD360.cpp:294-320,
 * OdometryKeyFrame360.cpp:124-140) -- Segal, Haehnel and Thrun's plane-to-plane ICP.  Every match has a 3 x 3 weight built from a
 * covariance on either side; here the target's covariance comes from the map's resident per-voxel normal (the section above) and the
 * source's from a normal per source point, which may be those of another voxel map: "filterVoxel both, then GICP", and also the
 * alignment of one submap against another.  Planar pairs constrain along their normals; a pair without a planar side degrades to
 * point-to-point instead of dropping out, which is what rgbd360_map_align_plane_* does with corners and edges.
 * Everything below is float64 with + - x / sqrt only, every operation rounded on its own (no fused multiply-add): host, device and a
 * restatement in IEEE arithmetic agree bit for bit per point.  Per source point at the current pose T = [R | t]:
 *   1 match: steps 1-4 of the point-to-point definition, bit for bit -- the map's steps 1-5, the 27 cells in the same order,
 *     count >= min_count, the read-out's centroid, d2 in float32, a tie to the earlier cell, kept iff d2 <= max_dist^2, max_dist in
 *     (0, leaf].  The key and d2 of a point are those of rgbd360_map_align_*.  e = the float32 w - c of the match, widened to double.
 *   2 target covariance: if use_target_normals != 0 and the matched voxel is RGBD360_NORMAL_OK in the normal layer of
 *     (min_count, min_support, max_flatness) -- this call's min_count; the layer is built or reused exactly as by the surface cast --
 *     nb = the doubles of its float32 normal as stored and C_B[j][k] = delta_jk - s (nb_j nb_k), s = 1.0 - (double)epsilon (the
 *     off-diagonal terms as 0.0 - s (nb_j nb_k)).  Otherwise C_B = I.
 *   3 source covariance: a source normal is present for point i iff a normal array was passed, its three floats are finite and
 *     q = (n_x n_x + n_y n_y) + n_z n_z > 0 (in double).  Then n^ = n / sqrt(q), na_k = (R_k0 n^_x + R_k1 n^_y) + R_k2 n^_z with R the
 *     doubles of the float32 pose, and C_A[j][k] = delta_jk - s (na_j na_k).  Otherwise C_A = 0: the source point is a point.
 *     These are the special cases of Segal et al.: no normal on either side is point-to-point (M = I exactly), target normals only is
 *     point-to-plane with weight 1 / epsilon along the normal and 1 across it, normals on both sides is plane-to-plane.
 *   4 weight: A = C_B + C_A per element, symmetric;  c00 = A11 A22 - A12 A12, c01 = A02 A12 - A01 A22, c02 = A01 A12 - A02 A11,
 *     c11 = A00 A22 - A02 A02, c12 = A01 A02 - A00 A12, c22 = A00 A11 - A01 A01, det = (A00 c00 + A01 c01) + A02 c02, M_jk = c_jk / det.
 *     A is positive definite for epsilon in (0, 1] (its eigenvalues are at least epsilon): there is no failure branch.
 *   5 terms: J = [I | -[w]x], the point method's Jacobian, for the increment pose <- pseudo_exp(v, omega) pose.  Its columns are
 *     u_0..2, the unit vectors, and u_3 = (0, -w_z, w_y), u_4 = (w_z, 0, -w_x), u_5 = (-w_y, w_x, 0) (u_3+k = e_k x w).  m_b = M u_b,
 *     q = M e, each a sum of products left to right, (a + b) + c; a component of u that is 0 contributes no term and one that is 1 no
 *     product.  H_ab = u_a . m_b for a <= b, g_a = u_a . q, cost = (e_x q_x + e_y q_y) + e_z q_z, ee = (e_x e_x + e_y e_y) + e_z e_z.
 *   6 row: n, the 21 H terms row by row, the 6 g terms, sum cost, sum ee, then the counters n_valid, n_box_rejected, n_out_of_range,
 *     n_target_planes (kept matches with a target normal), n_source_planes (kept matches with a source normal), n_plane_pairs (both),
 *     probes and points searched: 38 doubles.  One partial row per workgroup, the rows added in ascending order; no floating-point
 *     atomics: the same sums from run to run.
 *   7 loop: steps 6-7 of the point method unchanged -- H and g cast to float32, gn::step with lambda 0, RGBD360_ILL_POSED on
 *     rank(H) < 6, RGBD360_NO_VALID_PIXELS below min_matches, converged on v.v <= eps and omega.omega <= eps, at most max_iters steps,
 *     the final evaluation, one stream synchronisation.  fitness = sum cost / n, fitness_point = sum ee / n.
 * The table and the map are never written; the normal layer is the map's own (16 bytes per slot, see above).
 * Differences from PCL's GICP, stated: PCL minimises with BFGS and keeps the weights of a set of correspondences fixed while it does;
 * here it is Gauss-Newton with M re-formed from the current rotation at every evaluation (M's dependence on the pose is not
 * differentiated).  PCL's covariances come from the 20 nearest neighbours of every point of either cloud; here from the normal of the
 * matched voxel (fitted to the centroids of its 27 cells) and from the normals the caller passes.  The match is the nearest centroid
 * within one leaf, not a kd-tree search within 0.3 - 0.4 m.  PCL is not part of the reference tree: parity with PCL is unpinned.
 * rgbd360_map_align_c2f_* does not take this method. */
typedef struct {
    float max_dist;            /* as in rgbd360_map_align_params */
    int   max_iters;
    float eps;
    int   min_count;           /* also the normal layer's */
    long long min_matches;     /* kept matches an evaluation must have: 6 */
    float epsilon;             /* the covariance of a plane along its normal, in (0, 1]: 1e-3 (PCL's gicp_epsilon); 1 makes every side isotropic */
    int   use_target_normals;  /* 0: C_B = I for every match; default 1 */
    int   min_support;         /* of the normal layer, 1 .. 27: 5 */
    float max_flatness;        /* of the normal layer, >= 0: 0.05 */
} rgbd360_map_align_gicp_params;
typedef struct {
    int status, iterations, converged;
    long long n_valid, n_box_rejected, n_out_of_range, n_matched;      /* of the final evaluation; n_matched: the kept matches */
    double fitness;            /* sum e^T M e / n_matched (0 when nothing matched) */
    float hessian[36], gradient[6];
    long long n_target_planes, n_source_planes, n_plane_pairs;   /* kept matches with a target normal / a source normal / both */
    double fitness_point;      /* sum e.e / n_matched over the same matches: rgbd360_map_align_result.fitness's scale */
} rgbd360_map_align_gicp_result;
void   rgbd360_map_default_align_gicp_params(const rgbd360_map* map, rgbd360_map_align_gicp_params* p);
/* As rgbd360_map_align_cloud (arguments, return values, refusals, an empty map, an empty input; also -1 for epsilon outside (0, 1] or
 * NaN, min_support outside 1 .. 27, a negative or NaN max_flatness).  normal: 3 n floats in the frame's coordinates where xyz is (host
 * or device memory), one per point, any length; NULL: no source normals.  A normal that is zero or not finite marks a point without
 * one.  rgbd360_map_align_trace's records work as for the other methods (sum_sq: sum cost). */
int    rgbd360_map_align_gicp_cloud(rgbd360_map* map, const float* xyz, const float* normal, long long n, const float guess[16], int on_device,
                                    const rgbd360_map_align_gicp_params* params, float pose_out[16], rgbd360_map_align_gicp_result* result);
/* A sphere frame, as rgbd360_map_align_sphere.  It takes no source normals: the point-to-plane limit on the resident normals. */
int    rgbd360_map_align_gicp_sphere(rgbd360_map* map, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                     const float guess[16], int on_device, const rgbd360_map_align_gicp_params* params, float pose_out[16],
                                     rgbd360_map_align_gicp_result* result);

/* ---- colour of the map (csrc/map_colour.h) ---------------------------------------------------------------------------------------
 * What an alignment needs of the colour sums every slot keeps: one intensity per voxel and its gradient on the voxel's tangent plane,
 * fitted to the intensities of the voxels around it, kept resident next to the table like the normals it builds on.  A function of the
 * voxel set, its colour sums and the five parameters alone: not of the order of insertion, the table's capacity, a slot index or the
 * run.  Float64 with + - x / sqrt only, every operation rounded on its own and in the order written: host, device and a restatement in
 * IEEE arithmetic agree bit for bit.  Nothing here writes the table.
 *   1 intensity   Y = 4899 Sr + 9617 Sg + 1868 Sb in int64 (the dense alignment's gray weights, their sum 2^14), I64 = (double)Y /
 *                 (((double)count 16384) 255), in [0, 1].  A voxel's I = (float)I64.  A source point's intensity (coloured ICP below) is I64
 *                 of its three bytes with count 1, kept as a double.
 *   2 status      RGBD360_COLOUR_NONE: count < min_count.  RGBD360_COLOUR_NO_NORMAL: the voxel is not RGBD360_NORMAL_OK in the normal
 *                 layer of (min_count, min_support, max_flatness).  Otherwise the fit decides: RGBD360_COLOUR_OK or _NO_GRADIENT.
 *   3 basis       n = the doubles of the voxel's float32 normal; k = the axis of smallest |n_k|, the lowest index on a tie; t = e_k x n
 *                 (k = 0: (0, -n_z, n_y); 1: (n_z, 0, -n_x); 2: (-n_y, n_x, 0)); u = t / sqrt((t_x t_x + t_y t_y) + t_z t_z); v = n x u.
 *   4 fit         the neighbours are the voxels with count >= min_count in the 27 cells, the voxel itself left out, in the cells' order
 *                 of the alignments (the centre first, then dz / dy / dx ascending).  Per neighbour r = the float32 difference of the
 *                 read-out's centroids, neighbour minus voxel, widened; a = (r_x u_x + r_y u_y) + r_z u_z, b the same with v,
 *                 delta = (double)I_nb - (double)I; m counts them, Saa += a a, Sab += a b, Sbb += b b, Sad += a delta, Sbd += b delta.
 *                 NO_GRADIENT when m < min_gradient_support, or unless det > min_spread (tr tr) with det = Saa Sbb - Sab Sab and
 *                 tr = Saa + Sbb (neighbours on one line, or too few directions: det / tr^2 is lambda_0 lambda_1 / (lambda_0 + lambda_1)^2 of
 *                 their tangential scatter, at most 1/4).  Else du = (Sad Sbb - Sbd Sab) / det, dv = (Saa Sbd - Sab Sad) / det and
 *                 d_k = (float)(du u_k + dv v_k): the gradient in world coordinates, per metre, tangent to the voxel's plane.  d is zero
 *                 unless the status is OK.
 * The layer: 16 bytes per table slot of device memory beside the table (I with the status in its two spare top bits, then d),
 * owned by the map, built by the first call that needs it -- one launch over the slots behind the normal layer's -- reused until the
 * map is written or one of the five parameters differs, freed with the map or by rgbd360_map_release_colours (rgbd360_map_bytes stays
 * the table's size).  A map that was fed without colours has I = 0 and d = 0 everywhere; nothing detects it: that is the caller's
 * business.  Out of scope: colour gradients from the points inside a voxel, neighbourhoods wider than the 27 cells, exposure
 * compensation. */
enum { RGBD360_COLOUR_NONE = 0, RGBD360_COLOUR_OK = 1, RGBD360_COLOUR_NO_NORMAL = 2, RGBD360_COLOUR_NO_GRADIENT = 3 };
typedef struct {
    int   min_count;             /* the normal layer's three (rgbd360_map_normal_params): 1 */
    int   min_support;           /* 5 */
    float max_flatness;          /* 0.05 */
    int   min_gradient_support;  /* neighbours a gradient needs, 1 .. 26: 4 */
    float min_spread;            /* smallest det / tr^2 of the neighbours' tangential scatter, >= 0: 0.01 (the smaller spread about a tenth of
                                    the larger) */
} rgbd360_map_colour_params;
typedef struct { long long n_voxels, n_below_min_count, n_no_normal, n_no_gradient, n_gradients; } rgbd360_map_colour_stats;
void      rgbd360_map_default_colour_params(const rgbd360_map* map, rgbd360_map_colour_params* p);
/* One record per voxel with count > 0, sorted as rgbd360_map_extract sorts ((i_z, i_y, i_x) ascending): returns the voxel count; the first
 * max_out records are written; any output pointer may be NULL.  xyz [3], count and key3 [3] are the read-out's bits; intensity, gradient
 * [3] and status as defined above.  stats (may be NULL): exact counts over the whole map, whatever max_out.  Host arrays; the call waits.
 * -1, nothing launched and no output touched: min_count < 1, min_support outside 1 .. 27, min_gradient_support outside 1 .. 26,
 * max_flatness or min_spread negative or NaN, max_out < 0.  params NULL: the defaults.  An empty map returns 0 with zero statistics and
 * launches no kernel. */
long long rgbd360_map_colours(rgbd360_map* map, const rgbd360_map_colour_params* params, long long max_out, float* xyz, float* intensity,
                              float* gradient, int32_t* status, int32_t* count, int32_t* key3, rgbd360_map_colour_stats* stats);
/* The same into device arrays on the map's device (stats_dev too; params is host memory), in NO specified order (key3 and xyz come
 * along), at most max_out records: enqueued on the context's stream, the call does not wait. */
long long rgbd360_map_colours_dev(rgbd360_map* map, const rgbd360_map_colour_params* params, long long max_out, float* xyz_dev, float* intensity_dev,
                                  float* gradient_dev, int32_t* status_dev, int32_t* count_dev, int32_t* key3_dev, rgbd360_map_colour_stats* stats_dev);
/* Device memory of the colour layer (0: none); rgbd360_map_release_colours frees it, the next call that needs it rebuilds. */
size_t    rgbd360_map_colour_bytes(const rgbd360_map* map);
int       rgbd360_map_release_colours(rgbd360_map* map);

/* ---- coloured ICP against the map (csrc/map_align_colour.h) ------------------------------------------------------------------------
 * Park, Zhou and Koltun's coloured point-cloud registration (Open3D's registration_colored_icp) with the map as the target: the
 * point-to-plane term on the map's resident normals joined with a photometric term on the resident intensity gradients above.  Indoors
 * -- a corridor, a floor and one wall -- geometry leaves the pose unobservable along the surfaces; the texture on them does not.
 * Float64 with + - x / only, every operation rounded on its own.  Per source point at the current pose:
 *   1 match: steps 1-4 of the point-to-point definition, bit for bit; e = the float32 w - c of the match, widened to double.
 *   2 class: a kept match whose voxel is not RGBD360_NORMAL_OK in the normal layer of (min_count, min_support, max_flatness) is dropped
 *     and counted in n_no_normal.  Otherwise n = the doubles of its float32 normal and I, d = those of its colour record under
 *     (min_gradient_support, min_spread) -- both layers built or reused as their read-outs do; with RGBD360_COLOUR_NO_GRADIENT d = 0, the
 *     point is counted in n_no_gradient and stays.  I_q = the source point's intensity (step 1 of the section above).
 *   3 residuals: r_G = (n_x e_x + n_y e_y) + n_z e_z; p_k = e_k - r_G n_k; r_C = (I + ((d_x p_x + d_y p_y) + d_z p_z)) - I_q.
 *   4 rows, for the increment pose <- pseudo_exp(v, omega) pose: J_G = [n | w x n], J_C = [d | w x d] (d is tangent, so the derivative of
 *     the projection drops out), w x n = (w_y n_z - w_z n_y, w_z n_x - w_x n_z, w_x n_y - w_y n_x).
 *   5 sums: l = (double)lambda_geometric, c = 1.0 - l, sG_a = l J_G,a, sC_a = c J_C,a; H_ab += sG_a J_G,b + sC_a J_C,b for a <= b,
 *     g_a += sG_a r_G + sC_a r_C, cost += l (r_G r_G) + c (r_C r_C), gg += r_G r_G, cc += r_C r_C.
 *   6 row: n, the 21 H terms row by row, the 6 g terms, cost, gg, cc, then the counters n_valid, n_box_rejected, n_out_of_range,
 *     n_no_normal, n_no_gradient, probes and points searched: 38 doubles.  One partial row per workgroup, the rows added in ascending
 *     order; no floating-point atomics.
 *   7 loop: as for the other methods -- H and g cast to float32, gn::step with lambda 0, RGBD360_ILL_POSED on rank(H) < 6,
 *     RGBD360_NO_VALID_PIXELS below min_matches, converged on v.v <= eps and omega.omega <= eps, at most max_iters steps, the final
 *     evaluation, one stream synchronisation.  fitness = cost / n.
 * With lambda_geometric = 1 everything but cc is independent of the colours (point-to-plane on the resident normals); 0 is the
 * photometric term alone.  The table is never written.  Differences from Open3D, stated: the target's gradient comes from the voxels of
 * the 27 cells, not from a radius search; a robust kernel is a setting of the map (below: one joint weight for both terms); sqrt(lambda) is not folded into the residuals (the same
 * normal equations).  Out of scope: a colour switch in rgbd360_map_align_c2f_*, colour on the source side of a map-against-map
 * alignment, exposure compensation. */
typedef struct {
    float max_dist;              /* as in rgbd360_map_align_params */
    int   max_iters;
    float eps;
    int   min_count;             /* also the two layers' */
    long long min_matches;       /* contributing points an evaluation must have: 6 */
    float lambda_geometric;      /* the geometric term's weight in [0, 1], the photometric term's is 1 - lambda: 0.968 (Open3D's) */
    int   min_support;           /* of the normal layer: 5 */
    float max_flatness;          /* 0.05 */
    int   min_gradient_support;  /* of the colour layer: 4 */
    float min_spread;            /* 0.01 */
} rgbd360_map_align_colour_params;
typedef struct {
    int status, iterations, converged;
    long long n_valid, n_box_rejected, n_out_of_range, n_matched;      /* of the final evaluation; n_matched: the contributing points */
    double fitness;              /* (lambda sum r_G^2 + (1 - lambda) sum r_C^2) / n_matched (0 when nothing matched) */
    float hessian[36], gradient[6];
    long long n_no_normal, n_no_gradient;      /* kept matches dropped for want of a normal / contributing with a zero gradient */
    double rms_geometric, rms_colour;          /* sqrt(sum r_G^2 / n_matched) in metres, sqrt(sum r_C^2 / n_matched) in intensity units */
} rgbd360_map_align_colour_result;
void   rgbd360_map_default_align_colour_params(const rgbd360_map* map, rgbd360_map_align_colour_params* p);
/* As rgbd360_map_align_cloud (arguments, return values, refusals, an empty map, an empty input) with the cloud's colours rgb3, n x 3
 * bytes where xyz is, as rgbd360_map_insert_cloud takes them.  Also -1, before anything is launched: rgb3 NULL with n > 0, lambda_geometric
 * outside [0, 1] or NaN, and what rgbd360_map_colours refuses of the layers' parameters.  rgbd360_map_align_trace's records work as for
 * the other methods (sum_sq: the cost). */
int    rgbd360_map_align_colour_cloud(rgbd360_map* map, const float* xyz, const uint8_t* rgb3, long long n, const float guess[16], int on_device,
                                      const rgbd360_map_align_colour_params* params, float pose_out[16], rgbd360_map_align_colour_result* result);
/* A sphere frame with its colour image, as rgbd360_map_insert_sphere takes the two; rgb NULL is refused. */
int    rgbd360_map_align_colour_sphere(rgbd360_map* map, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type,
                                       int rows, int cols, int convention, const float guess[16], int on_device,
                                       const rgbd360_map_align_colour_params* params, float pose_out[16], rgbd360_map_align_colour_result* result);

/* ---- robust kernels of the alignments against the map (csrc/map_align_robust.h) ----------------------------------------------------
 * The match gate max_dist <= leaf is all that keeps a wrong match out of the four alignments above: at leaf 0.1 m a surface 4 - 6 cm
 * from where the map has it -- a box that moved, a door, a ghost wall, a person -- still matches and enters the normal equations at full
 * weight.  A robust kernel gives every contributing point one weight, computed from the residual the method already has; the kinds and
 * their formulas are the pose graph's (gn::robust_rho_w, one text for host and device; RGBD360_MAP_ROBUST_* equal RGBD360_GRAPH_ROBUST_*).
 * Float64 with + - x / sqrt only (Cauchy's rho also log1p), every operation rounded on its own; tests/map_align_robust_reference.py
 * restates it in numpy.
 *   cost term   a kept, contributing point of method M has the per-point cost term s, exactly the double the quadratic evaluation adds to
 *               its cost word: point (e_x e_x + e_y e_y) + e_z e_z; plane r r; generalized ICP its cost e^T M e; colour
 *               l (r_G r_G) + c (r_C r_C) -- one joint weight for both terms.
 *   weight      (rho, w) = robust_rho_w(kind, delta_eff, s): Huber rho = s, w = 1 for s <= delta^2, else rho = 2 delta sqrt(s) - delta^2,
 *               w = delta / sqrt(s); Cauchy rho = delta^2 log1p(s / delta^2), w = 1 / (1 + s / delta^2); Geman-McClure t = delta^2 /
 *               (delta^2 + s), rho = s t, w = t t.  s = 0 gives (0, 1) for every kind.  delta is in the units of sqrt(s): metres for point
 *               and plane.  delta_eff = delta 2^shift on the level `shift` of a map pyramid when scale_with_level is set (exact), else delta.
 *   row         M's row with two words behind it.  Every word in front of M's cost word receives w t, t the quadratic evaluation's own
 *               term rounded as it rounds it (e.g. t = J_a J_b), then the one product w t, then the add: word 0 holds sum w.  The cost
 *               word receives rho.  The diagnostic sums behind it (sum e.e, sum r_G^2, sum r_C^2) and all counters stay unweighted.
 *               Word kWords: the number of contributing points n -- what min_matches, n_matched, the trace's n and fitness = sum rho / n
 *               use.  Word kWords + 1: the number of points with w < 1.  H and g are assembled from the weighted words as M assembles
 *               them; the trace's sum_sq is sum rho.  The returned Hessian and gradient are the weighted ones: an edge built from a
 *               robust alignment carries less information where the alignment distrusted its matches.
 * The setting is per method and resident in the map; it is no layer and bumps no revision.  Every method starts at
 * RGBD360_MAP_ROBUST_NONE, and with NONE no robust kernel is launched: the call is the quadratic call, byte for byte.  Honoured by
 * rgbd360_map_align_* / _plane_* / _gicp_* / _colour_* (sphere and cloud), rgbd360_map_align_batch_* and _plane_batch_* (_best compares
 * the robust fitness), rgbd360_map_align_c2f_* (a level uses its root's setting) and whatever is built on them.  NOT honoured by
 * rgbd360_map_calibrate_rig_*, the depth trainer and evaluator, and the plane relocalisation: they keep the quadratic kernels.
 * Out of scope: separate weights for the two terms of coloured ICP, an adaptive delta, the second-order term of the loss, any change to
 * the match gate.  Limit, stated: a robust kernel needs the displaced surface to be the minority of what constrains a direction; where
 * it is the majority every kind locks onto it. */
enum { RGBD360_MAP_METHOD_POINT = 0, RGBD360_MAP_METHOD_PLANE = 1, RGBD360_MAP_METHOD_GICP = 2, RGBD360_MAP_METHOD_COLOUR = 3 };
enum { RGBD360_MAP_ROBUST_NONE = 0, RGBD360_MAP_ROBUST_HUBER = 1, RGBD360_MAP_ROBUST_CAUCHY = 2, RGBD360_MAP_ROBUST_GEMAN_MCCLURE = 3 };
typedef struct {
    int    kind;               /* RGBD360_MAP_ROBUST_*: NONE */
    int    scale_with_level;   /* != 0: delta x 2^shift on level `shift` of the map's pyramid: 0 */
    double delta;              /* > 0 and finite unless kind is NONE (then ignored), in the units of sqrt(s) */
} rgbd360_map_robust;
typedef struct {
    int    method, kind;       /* of the alignment reported; kind NONE: the quadratic call (sum_w = n, n_downweighted = 0) */
    double delta_eff;          /* the delta the kernels took */
    double sum_w;              /* word 0 of the final evaluation's row */
    long long n, n_downweighted;       /* its contributing points, and those of them with w < 1 */
} rgbd360_map_robust_info;
/* 0; -1 with rgbd360_map_last_error set and the setting untouched: a NULL map or setting, an unknown method, a kind outside 0 .. 3, a
 * delta that is not finite and positive when the kind is not NONE, a `map` that is a level of a pyramid (levels follow their root). */
int    rgbd360_map_set_align_robust(rgbd360_map* map, int method, const rgbd360_map_robust* robust);
/* The method's setting (a level: its root's); -1 for a NULL map or output or an unknown method, the output untouched. */
int    rgbd360_map_get_align_robust(rgbd360_map* map, int method, rgbd360_map_robust* robust);
/* What the last single alignment on this map did (rgbd360_map_align_c2f_*: its finest level); all zero before the first.  The
 * second: job `job` of the map's last batch; -1 when there is no such job. */
int    rgbd360_map_align_robust_info(rgbd360_map* map, rgbd360_map_robust_info* info);
int    rgbd360_map_align_batch_robust_info(rgbd360_map* map, int job, rgbd360_map_robust_info* info);

/* ---- free-space observation and carving of the map (csrc/map_carve.h) -----------------------------------------------------------
 * What lets the map react to what a new frame sees: an object that moved away, a ghost wall left by a pose that was corrected later,
 * points dropped into space that a later frame looks straight through.  Every measurement of a posed depth frame, or of a list of rays,
 * is a line of sight.  The map voxels it passes through well in front of the measured point are SEEN THROUGH: rgbd360_map_observe_*
 * counts that per voxel (the votes: a free-space check), rgbd360_map_votes reads the counts out and rgbd360_map_carve erases the voxels
 * that thresholds on them condemn.  An observation never writes the table.  All traversal arithmetic is float64 + - x / without
 * contraction, as for the ray cast above, whose steps these are; there is no square root and no libm call in it.  The votes are a
 * function of the voxel set and the measurements alone: not of the order of insertion, the table's capacity, slot indices or the run.
 *   1 segment     from a sphere image: the world point w of steps 1, 3 and 4 of the map's definition (the point of the pixel and
 *                 convention, the pose, the range check).  The box of step 2 is NOT applied: a point outside the box is not stored, but it
 *                 still proves free space.  o = the pose's translation.  From a list: origins and endpoints, n x 3 float32 in world
 *                 coordinates; o the origin, w the endpoint, range-checked as in step 4.  d_k = w_k - o_k, rounded to float32: the
 *                 measurement lies at t = 1.  A measurement is invalid -- counted in n_skipped, nothing traversed, no vote -- when the
 *                 point or w is not finite or out of range, o or d is not finite, or d = 0.
 *   2 walk        steps 2 - 6 of the ray cast with t_max = 1 and max_steps as there, but the walk does not end at a candidate: it ends
 *                 where a cell's entry lies beyond t = 1, where it leaves the box of the live voxels, or after max_steps cells
 *                 (n_max_steps).  A segment that misses the box (n_miss_box) visits nothing.  The coarse layer's jump through absent
 *                 bricks is kept: it changes no vote and no counter but n_lookups.
 *   3 through     a cell is considered when its voxel is live with count >= min_count.  c, s, t_in, t_out and
 *                 th = min(max(s, t_in), t_out) are those of step 5 of the ray cast, off2 = ((e_x e_x + e_y e_y) + e_z e_z) (inv_leaf
 *                 inv_leaf) its squared offset in leaves, dd = (d_x d_x + d_y d_y) + d_z d_z.  The voxel gets one through-vote iff
 *                   (th th) dd >= near near                       (near in metres; default: leaf, which drops the voxel the camera sits in),
 *                   q = (1 - th) - margin_rel >= 0 and (q q) dd >= (margin_leaves leaf)^2
 *                                                                 (it lies at least margin_leaves leaf + margin_rel |d| metres in front of
 *                                                                 the measured point; defaults 2.0 and 0), and
 *                   off2 <= max_offset max_offset                 (default 0.5 leaves: a segment that only clips a cell's corner does not vote).
 *                 near, margin_rel, margin_leaves, leaf and max_offset enter as the doubles of their float32 values.
 *   4 end         the voxel of step 5 of the map's definition for w -- (int)floorf(w_k * inv_leaf) in float32, the voxel this measurement
 *                 would feed -- gets one end-vote if it is live (count > 0).  End-votes protect the surfaces the frame also measures: a
 *                 wall seen at a grazing angle by one ray and frontally by others.
 *   5 votes       one 64-bit word per table slot in a side array: through-votes in the low 32 bits, end-votes in the high 32 bits; every
 *                 vote is one 64-bit atomic add, and the add that sees 0 counts the voxel in n_voxels_voted (exact, whatever the order).
 *                 The array is allocated by the first observation (8 bytes per slot: rgbd360_map_vote_bytes) and freed by
 *                 rgbd360_map_release_votes, rgbd360_map_rehash and rgbd360_map_destroy.  It belongs to the table as it stood when the
 *                 votes were taken: once the map is written (insert, remove, move, clear) the votes are stale.
 *   6 carve       per live voxel with a non-zero vote word (n_voted): erased iff through >= min_through, end <= max_end, and
 *                 max_count == 0 or count <= max_count.  n_protected_end: through >= min_through but end > max_end; n_protected_count:
 *                 both hold but count > max_count.  Erasing sets the count and the six sums to 0 and keeps the key: exactly the
 *                 tombstone a removal leaves.  The map's size falls by n_voxels_carved; the coarse layer, the normals and the pyramid
 *                 levels follow on their next use.  A carve marks the votes spent.
 * Statistics of an observation, exact integers: n_rays measurements, n_valid + n_skipped = n_rays, n_miss_box and n_max_steps among
 * the valid ones, n_steps cells visited, n_lookups voxel-table lookups of the walk (the one number that depends on the form of the
 * traversal; the end-vote's lookup is not counted), n_through and n_end votes given, n_voxels_voted voxels whose word left 0 in this call.
 * The contract with exact removal (rgbd360_map_remove_* / _move_* above).  Carving is a LOSSY edit: a carved voxel forgets its points.
 * A later removal or move of a frame that fed a carved voxel reports those points in n_underflow and returns RGBD360_MAP_MISMATCH; as
 * long as the voxel was not revived in between nothing is subtracted for them and the map stays consistent (rgbd360_map_census:
 * n_inconsistent == 0), every other voxel is what the removal contract makes it.  Once a carved voxel was revived by an insert, removing
 * a frame that fed it before the carve leaves the map unspecified, as any removal outside the contract does.  Per-voxel provenance,
 * which would lift this, stays out of scope, as do normal-based rejection of grazing rays, occupancy probabilities, carving inside
 * pyramid levels and several GPUs. */
typedef struct {
    int   min_count;           /* points a voxel must hold to be voted on: 1 */
    float near;                /* voxels nearer than this to the origin, in metres, are not voted on: leaf */
    float margin_leaves;       /* the free margin in front of the measured point, in leaves ...: 2.0 */
    float margin_rel;          /* ... plus this share of the measured range: 0 */
    float max_offset;          /* largest distance of the centroid from the segment, in leaves: 0.5 */
    int   max_steps;           /* cells a segment may visit, 1 .. 2^23: 8192 */
    int   accumulate;          /* 0: the votes are zeroed first; 1: the votes are added to */
} rgbd360_map_observe_params;
typedef struct {
    long long n_rays, n_valid, n_skipped, n_miss_box, n_max_steps, n_steps, n_lookups, n_through, n_end, n_voxels_voted;
} rgbd360_map_observe_stats;
typedef struct { long long n_voted, n_voxels_carved, n_points_carved, n_protected_end, n_protected_count, n_voxels; } rgbd360_map_carve_stats;
void   rgbd360_map_default_observe_params(const rgbd360_map* map, rgbd360_map_observe_params* p);
/* The frame's arguments, refusals and empty inputs as for rgbd360_map_insert_sphere (no colour); stats is host memory and the call waits.
 * 0; -1, nothing launched and the votes untouched: a bad frame or NULL pose; min_count < 1; near, margin_leaves or margin_rel negative
 * or not finite; max_offset negative or not a number; max_steps outside 1 .. 2^23; accumulate not 0 or 1; a map that is a pyramid level;
 * accumulate = 1 when the votes are spent, when the map was written since they were taken, or when the measurements accumulated would
 * reach 2^31 (accumulate = 1 on a map without votes starts them).  An empty image or an empty map returns 0 with zero statistics,
 * launches no kernel and leaves the votes as they were.  params NULL: the defaults. */
int    rgbd360_map_observe_sphere(rgbd360_map* map, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                  const float pose[16], int on_device, const rgbd360_map_observe_params* params, rgbd360_map_observe_stats* stats);
/* The same for n segments: origins and endpoints are n x 3 float32 (on_device 1: device arrays on the map's device).  Also -1: n < 0 or
 * >= 2^31, origins or endpoints NULL with n > 0.  n == 0 as an empty image. */
int    rgbd360_map_observe_rays(rgbd360_map* map, long long n, const float* origins, const float* endpoints, int on_device,
                                const rgbd360_map_observe_params* params, rgbd360_map_observe_stats* stats);
/* The votes: one record per voxel with a non-zero vote word into host arrays (any may be NULL), sorted ascending by (i_z, i_y, i_x) like
 * rgbd360_map_extract: key3 = (i_x, i_y, i_z), the through- and end-votes, and the voxel's count at the time of the call -- 0 for the
 * voxels a carve erased.  Returns the number of voted voxels and writes min(that, max_out) records; -1 when the map holds no votes or
 * was written since they were taken by anything other than rgbd360_map_carve. */
long long rgbd360_map_votes(rgbd360_map* map, long long max_out, int32_t* key3, int32_t* through, int32_t* end, int32_t* count);
/* Step 6 over the votes as they stand; stats (may be NULL) as above, n_voxels the map's size after the call.  0; -1, the map untouched:
 * min_through < 1, max_end < 0 or max_count < 0; a pyramid level; no votes; the votes are spent; the map was written since they were
 * taken. */
int    rgbd360_map_carve(rgbd360_map* map, int min_through, int max_end, int max_count, rgbd360_map_carve_stats* stats);
/* bytes of device memory the vote array occupies (0: none), and its release */
size_t rgbd360_map_vote_bytes(const rgbd360_map* map);
int    rgbd360_map_release_votes(rgbd360_map* map);

/* ---- the map pyramid and coarse-to-fine ICP against it (csrc/map_pyramid.h) -------------------------------------------------------
 * Both ICPs above match within one leaf, so their capture range is one leaf; the reference's call sites run at 0.3 - 0.4 m.  The coarser
 * maps a wider basin needs are a function of the resident table.  Level s (1 <= s <= RGBD360_MAP_MAX_SHIFT) of a map is the map with
 * leaf' = leaf 2^s, inv_leaf' = inv_leaf 2^-s (both exact), the same box, one voxel per distinct (i_x >> s, i_y >> s, i_z >> s)
 * (arithmetic shifts: -1 and -2 merge at s = 1, -1 and 0 never do) over the parent's voxels with count > 0, and as its seven words
 * (count, S_x, S_y, S_z, S_r, S_g, S_b) the integer sums of theirs.  That is the contract.  Since fl(w inv_leaf') = fl(w inv_leaf) 2^-s
 * while the product is a normal float, the level equals, word for word, the map the same inserts build at leaf' -- for every point
 * whose |w_k inv_leaf| is 0 or >= 2^-126 2^s on all axes (a subnormal product may round differently: such a point lies within 1e-36 m of
 * a coordinate plane).  Levels are exact, independent of the order of insertion and of the table's layout.
 * Levels belong to the parent and are built on demand, level s out of level s - 1 by one kernel (integer atomics only), into a table of
 * the next power of two at or above twice the voxels of the level below (at least 1024 slots), so that no voxel is ever dropped; they are
 * device memory BESIDE the table: rgbd360_map_bytes stays the table's, rgbd360_map_pyramid_bytes is the levels'.  A level remembers the
 * parent's state it was built from and is rebuilt by the next rgbd360_map_level / _align_c2f_* call after the parent was written;
 * between such calls it keeps the content of the last one.  Nothing is maintained incrementally. */
#define RGBD360_MAP_MAX_SHIFT 6
/* Builds or refreshes levels 1 .. shift and hands out level `shift` as a BORROWED handle: every entry that only reads a map takes it
 * (size, bytes, extract, census, both alignments with their default-params and diagnostic eval entries, render, both ray casts,
 * normals, last_error); every entry that writes one (insert, remove, move, clear, rehash, set_box) refuses it with -1 and a message
 * before anything is touched; rgbd360_map_destroy of it does nothing.  The handle stays the same pointer for later calls with the same
 * shift and is valid until the parent is destroyed or rgbd360_map_release_levels is called.  The box is the parent's at the time of the
 * call.  0; -1 for a shift outside 1 .. RGBD360_MAP_MAX_SHIFT, a NULL argument or a `map` that is itself a level; -103 out of memory;
 * RGBD360_MAP_FULL if a build dropped a voxel (not expected at half load): then levels from that one up are gone. */
int    rgbd360_map_level(rgbd360_map* map, int shift, rgbd360_map** level);
/* device memory of the levels' tables (0 without levels; their ray-cast and normal layers and work buffers are not counted, as for a map) */
size_t rgbd360_map_pyramid_bytes(const rgbd360_map* map);
/* frees every level; handles handed out become invalid.  0; -1 for NULL or a level. */
int    rgbd360_map_release_levels(rgbd360_map* map);
/* Coarse-to-fine: for s = top_shift .. 0 the alignment of `kind` above runs on level s (level 0 is the map itself) from the pose the
 * level before ended on, with max_dist = max_dist_leaves x that level's leaf (the product in float32) and the other parameters as
 * given.  A level that ends with a status other than RGBD360_OK hands on the pose it was given.  The input is checked and uploaded
 * once.  Each level's step is, bit for bit, the single-level entry called on rgbd360_map_level(map, s) with that pose and those
 * parameters.  top_shift 0 is the single-level call. */
typedef struct {
    int   top_shift;           /* the coarsest level, 0 .. RGBD360_MAP_MAX_SHIFT: 3 */
    int   kind;                /* 0 point-to-point (rgbd360_map_align_*), 1 point-to-plane (rgbd360_map_align_plane_*), on every level */
    int   max_iters;           /* per level; these four as in rgbd360_map_align_params: 10, 1, 1e-6, 6 */
    int   min_count;
    float eps;
    float max_dist_leaves;     /* in (0, 1]: 1 */
    long long min_matches;
    int   min_support;         /* kind 1, as in rgbd360_map_align_plane_params: 5, 0.05 */
    float max_flatness;
} rgbd360_map_c2f_params;
typedef struct {
    int shift, status, iterations, converged;                          /* of this level's alignment */
    long long n_valid, n_box_rejected, n_out_of_range, n_matched;      /* of its final evaluation */
    double fitness;
    float pose[16];            /* the pose it ended on (its own result; what it hands on is this only when status is RGBD360_OK) */
} rgbd360_map_c2f_level;
typedef struct {
    int n_levels;              /* top_shift + 1; levels[0] is the coarsest, levels[n_levels - 1] the map itself */
    rgbd360_map_c2f_level levels[RGBD360_MAP_MAX_SHIFT + 1];
    float hessian[36], gradient[6];         /* of level 0's final evaluation */
} rgbd360_map_c2f_result;
void   rgbd360_map_default_c2f_params(const rgbd360_map* map, rgbd360_map_c2f_params* p);
/* Arguments, refusals and empty inputs as for rgbd360_map_align_sphere / _cloud; also -1 for top_shift outside 0 .. RGBD360_MAP_MAX_SHIFT,
 * a kind other than 0 or 1, max_dist_leaves outside (0, 1] or a `map` that is itself a level, and what rgbd360_map_level returns when a
 * level cannot be built.  The status returned and pose_out are those of level 0.  Neither the map nor a level's table is written;
 * levels 1 .. top_shift are refreshed first. */
int    rgbd360_map_align_c2f_sphere(rgbd360_map* map, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                    const float guess[16], int on_device, const rgbd360_map_c2f_params* params, float pose_out[16],
                                    rgbd360_map_c2f_result* result);
int    rgbd360_map_align_c2f_cloud(rgbd360_map* map, const float* xyz, long long n, const float guess[16], int on_device,
                                   const rgbd360_map_c2f_params* params, float pose_out[16], rgbd360_map_c2f_result* result);

/* ---- composing maps: merge at a pose, exact un-merge, table records (csrc/map_merge.h) -------------------------------------------------
 * Submaps: a small map per keyframe window, the pose graph moves the windows, the global map is composed from them.  The table's sums
 * are integers, so composition is exact and reversible, as removal and the pyramid are.  The source of a merge is the set of live
 * voxels of `src` (count >= min_count, default 1), each with its words {key, n, Sx, Sy, Sz, Sr, Sg, Sb}.
 * Pose mode (pose != NULL: 16 floats, column-major, the destination's world <- the source's world; the leaves may differ).  Per source
 * voxel, in this order:
 *   1 centroid  c_k = (float)((double)S_k / ((double)n * 1048576.0)): the read-out's bits.
 *   2 box       none: the content passed the source's box when it was inserted.
 *   3 pose      w_k = ((R_k0 c_x + R_k1 c_y) + R_k2 c_z) + t_k in float32, every product and sum rounded on its own: step 3 of an insert.
 *   4 range     dropped and counted unless every w_k is finite and |w_k| < 4096; a source voxel of 2^31 points or more is out of range too.
 *   5 voxel     i_k = (int)floorf(w_k * inv_leaf) with the DESTINATION's inv_leaf.
 *   6 sums      into that destination voxel: count += n, S_k += n * llrint((double)w_k * 1048576.0) (in int64: n < 2^31), S_c += S_c(src).
 * The result is the insertion of n coincident points at the posed centroid, with the colour total kept: rgbd360_map_census reports
 * n_inconsistent == 0 afterwards.
 * Sum mode (pose == NULL; src's leaf must be bit-equal to dst's): the key is kept and all seven words are added.  dst is then, bit for
 * bit, the map that received both maps' insertions.
 * Un-merge takes the same terms off again, in removal's manner: a read-only lookup, the count lowered in a compare-and-swap loop that
 * never goes below zero, the two's-complement negatives of the six sums added; emptied voxels stay as tombstones.  The contract: the same
 * source, unchanged since the merge, the same pose and min_count, and that merge did not return RGBD360_MAP_FULL.  Then dst is, bit for
 * bit, the map that never saw the merge, whatever was inserted in between.  Outside the contract no word wraps: a source voxel whose
 * destination is not in the table counts its points in n_missing; one asked for more than the destination holds takes what is there,
 * counts the rest in n_underflow and leaves the sums alone (per voxel, as rgbd360_map_remove_*); the call returns RGBD360_MAP_MISMATCH.
 * Both write dst as any writer does (levels, ray-cast, normal and plane layers follow, votes go stale, rgbd360_map_size is exact with
 * and without tombstones in dst); src is only read and may be a level of a pyramid.  Both maps belong to one context.
 * Statistics: n_voxels_read / n_points_read = n_*_below_min_count + n_*_out_of_range + n_*_dropped + n_*_added, voxels and points each.
 * merge: n_*_dropped found no free slot; n_voxels_new were created (or revived).  un-merge: n_*_added are the voxels taken off in full
 * and the points taken off, n_voxels_new the voxels emptied, n_voxels_dropped the voxels missing or short, n_points_dropped =
 * n_missing + n_underflow.  n_voxels: dst's size after the call.
 * Out of scope: sum mode across leaves, several GPUs, incremental upkeep of the layers, any interpolation or splatting of a posed voxel
 * over several cells. */
typedef struct {
    int min_count;             /* source voxels with fewer points are skipped (and counted): 1 */
} rgbd360_map_merge_params;
typedef struct {
    long long n_voxels_read, n_points_read, n_voxels_below_min_count, n_points_below_min_count, n_voxels_out_of_range, n_points_out_of_range;
    long long n_voxels_added, n_points_added, n_voxels_new, n_voxels_dropped, n_points_dropped, n_missing, n_underflow, n_voxels;
} rgbd360_map_merge_stats;
void   rgbd360_map_default_merge_params(const rgbd360_map* map, rgbd360_map_merge_params* p);
/* params and stats may be NULL.  0; RGBD360_MAP_FULL (merge: voxels already present still receive their terms); RGBD360_MAP_MISMATCH
 * (un-merge); -1 with a message in dst's last error and nothing launched for a NULL map, dst == src, a level as dst, maps of different
 * contexts, unequal leaves in sum mode, a pose with a non-finite entry or min_count < 1.  An empty source returns 0 and touches nothing. */
int    rgbd360_map_merge(rgbd360_map* dst, rgbd360_map* src, const float pose[16], const rgbd360_map_merge_params* params,
                         rgbd360_map_merge_stats* stats);
int    rgbd360_map_unmerge(rgbd360_map* dst, rgbd360_map* src, const float pose[16], const rgbd360_map_merge_params* params,
                           rgbd360_map_merge_stats* stats);
/* A map's live slots as they are: 8 x uint64 per voxel {key, n, Sx, Sy, Sz, Sr, Sg, Sb} (key = i_z + 2^20 << 42 | i_y + 2^20 << 21 |
 * i_x + 2^20; the sums in two's complement), ascending key.  Returns the voxel count and writes min(that, max_out) records to host
 * memory; negative: an error.  A map rebuilt from its records is the same map. */
long long rgbd360_map_records(rgbd360_map* map, long long max_out, uint64_t* records);
/* Adds n such records in sum mode (host memory, or on_device: device memory on the map's device); equal keys in one list add up.
 * Before anything is written a device pass checks every record: the key is not the empty marker (all ones) and is below 2^63 (three
 * 21-bit indices), the count lies in 1 .. 2^31 - 1, every colour sum is <= 255 count and every |S_k| < count 2^32.  One bad record
 * fails the call with -1 and a message naming how many were bad; the map is untouched.  0, RGBD360_MAP_FULL, or negative; n == 0
 * returns 0 and touches nothing.  stats (may be NULL) as for a merge. */
int    rgbd360_map_add_records(rgbd360_map* map, const uint64_t* records, long long n, int on_device, rgbd360_map_merge_stats* stats);

/* ---- pose-graph optimisation of store edges (csrc/pose_graph.h) -----------------------------------------------------------------
 * The reference closes its SLAM loop in g2o: optimizer.addVertex(pose), optimizer.addEdge(nearestKF, newKF, relPose, registerer.getInfoMat()),
 * optimizer.optimizeGraph(), optimizer.getPoses(...) (KFsphere_SLAM.cpp:262-265, 542-550, 630, 679-689; GraphOptimizer_G2O.cpp:
 * Levenberg-Marquardt, dense linear solver, optimize(10), vertex 0 fixed).  Here that step runs on the device: the edges are what
 * rgbd360_store_align returns, the optimised poses are what rgbd360_map_move_* takes.
 *   vertices   poses T_v (world <- frame): 16 floats column-major in and out, held in float64; each with a `fixed` flag.
 *   edges      (i, j, Z, Omega): Z (16 floats) is frame j in frame i -- the pose rgbd360_store_align returns for target i and source j;
 *              Omega (36 floats column-major) is used as (Omega + Omega^T) / 2 in float64, NULL = identity.
 *   tangent    (v; w), translation first, as everywhere in csrc/gn_math.h; updates multiply on the left: T_v <- se3_exp(x_v) T_v with the
 *              full exponential gn::se3_exp in float64.
 *   residual   E = Z T_j^-1 T_i, r = se3_log(E), the inverse of gn::se3_exp: a = vee of the antisymmetric part of R, the angle
 *              atan2(|a|, (tr R - 1) / 2); finite for every input, accurate for angles <= 3 rad.  T^-1 is the rigid inverse (R^T, -R^T t).
 *              r is the left perturbation xi in Z = exp(xi) T_i^-1 T_j: the tangent in which the dense alignment forms its Hessian
 *              (gn::step: exp(u) pose; its pseudo-exponential differs at second order only).  So rgbd360_result.hessian IS the
 *              information matrix of the edge, with no conversion.
 *   Jacobians  dr/dx_i = A = J_l^-1(r) Ad(Z T_j^-1), dr/dx_j = -A; J_l^-1 = I - ad/2 + ad^2/12 - ad^4/720 + ad^6/30240,
 *              ad(r) = [ [w]x [v]x ; 0 [w]x ] (truncation below 3e-9 for |r| <= 0.5).  Per edge W = A^T Omega A and b = A^T Omega r:
 *              H gains +W at (i,i) and (j,j), -W at (i,j) and (j,i); g gains +b at i, -b at j.
 *   cost, loop chi2 = sum r^T Omega r (quadratic edges; `robust` below).  Levenberg-Marquardt with the damping of the dense alignment, H + lambda diag(H): lambda starts at
 *              lambda_init (1e-3), is divided by 10 after an accepted step (not below 1e-9) and multiplied by 10 after a rejected one
 *              (RegisterRGBD360.h:389).  A step is accepted iff chi2 at the trial poses is smaller than chi2 at the current ones; a
 *              rejected step leaves the poses unchanged.  The loop ends after max_iters iterations (10: the reference's optimize(10)),
 *              after an accepted step with max |x| <= tol_update (converged), or with RGBD360_ILL_POSED when lambda > lambda_max or a
 *              damped 6x6 diagonal block has no Cholesky factor.
 *   vertices   a fixed vertex has x_v = 0; a vertex without edges is treated as fixed and counted (n_isolated); at least one vertex must
 *              be flagged fixed (-1 otherwise).
 *   solve      (H + lambda diag H) x = -g by conjugate gradients in float64, matrix-free over the edge list (q_i += W (p_i - p_j),
 *              q_j -= the same, plus lambda diag(H) p), preconditioned with the inverse of the damped 6x6 diagonal blocks; it ends at
 *              |r|_M <= cg_tol |r_0|_M, after cg_max_iters iterations, or when p.q is not positive.  The iteration count of block-Jacobi
 *              grows with the graph's diameter.
 *   sums       no floating-point atomics: a vertex adds its edges in edge-list order, every global scalar is a table of per-workgroup rows
 *              added in ascending order -- two calls on equal graphs give equal bits.
 * The host builds and uploads the incidence lists and edge arrays only when the graph changed; one stream synchronisation per
 * Levenberg-Marquardt iteration.  A graph is destroyed BEFORE its context and used from one thread at a time.
 *   robust     every edge carries a kind, a delta > 0 (double) and an enabled flag; a new edge is RGBD360_GRAPH_ROBUST_NONE and enabled.
 *              For an enabled edge s = r^T Omega r as above and, in float64 with d2 = delta * delta,
 *                NONE           rho = s                                              w = 1
 *                HUBER          s <= d2: rho = s; else q = sqrt(s), 2 delta q - d2   w = 1; else delta / q
 *                CAUCHY         u = s / d2, rho = d2 log1p(u)                        w = 1 / (1 + u)
 *                GEMAN_MCCLURE  t = d2 / (d2 + s), rho = s t                         w = t t
 *              with w = d rho / d s.  Omega only has a positive diagonal, so s may be <= 0: whenever !(s > 0) every kind gives rho = s,
 *              w = 1.  The cost is the sum of rho over the enabled edges, and chi2, chi2_trial, chi2_initial and chi2_final of the
 *              result and the trace are that cost.  The linearisation is first order (Triggs; g2o's rho[1]): W_e = w_e A^T Omega A,
 *              b_e = w_e A^T Omega r, without the second-derivative term.  Assembly, the solve, the trial poses, the accept test, the
 *              lambda schedule and the stop rules are as above, on the robust cost.  A graph whose edges are all NONE and enabled gives the
 *              bits it gave before the kinds existed (w is an exact 1).
 *   disabled   a disabled edge adds nothing to the cost, H or g and does not count as an edge of its vertices: a free vertex whose edges
 *              are all disabled is treated as fixed, counted in n_isolated, and its pose comes back bit for bit.  The enabled edges enter
 *              every vertex sum in edge-list order, as in a graph built without the disabled ones.
 *   caveats    the redescending kinds (CAUCHY, GEMAN_MCCLURE) can starve a vertex whose edges all have large residuals: when its damped
 *              block then has no Cholesky factor the call ends RGBD360_ILL_POSED as above.  Iteratively re-weighted least squares
 *              converges linearly: robust runs want tol_update around 1e-8; at 1e-10 the loop often ends on lambda_max instead.
 * The host builds and uploads the incidence lists again when an enabled flag changed; a change of kind or delta uploads two arrays of one
 * word per edge.
 *   covariance rgbd360_graph_marginals and rgbd360_graph_relative_covariances (csrc/pose_graph_cov.h; g2o's computeMarginals) recover 6x6 blocks of
 *              H^-1.  H is the Gauss-Newton matrix at the CURRENT poses with lambda = 0 over the free vertices: per enabled edge
 *              W_e = w_e A^T Omega A with the robust weight w_e, disabled edges absent, fixed and isolated vertices as above -- the matrix
 *              the linearisation and the assembly of rgbd360_graph_optimize build.  The calls change neither poses, nor edge state, nor
 *              the trace of the last optimisation: a following rgbd360_graph_optimize gives the bits it would have given without them.
 *                marginal of v        Sigma_vv, the diagonal block of H^-1, in the update tangent (v; w) of T_v <- se3_exp(x_v) T_v.  A fixed
 *                                     or isolated vertex gives an exact zero block with cg_iterations 0.
 *                relative (i, j)      C_ij = Ad(T_i^-1) (Sigma_ii + Sigma_jj - Sigma_ij - Sigma_ji) Ad(T_i^-1)^T, i = from, j = to: the first-order
 *                                     covariance of the left perturbation xi in T_i^-1 T_j <- exp(xi) T_i^-1 T_j, the tangent of the residual of
 *                                     an edge (i, j, Z), so commensurate with Omega^-1 of such an edge.  Computed from ONE block solve
 *                                     H X = E_j - E_i as (E_j - E_i)^T X, not from two marginals; a fixed end contributes no E; i == j gives zeros.
 *              Both are symmetrised as (M + M^T) / 2 in float64 and are NOT multiplied by the variance factor.
 *              cost is the bits rgbd360_graph_chi2 returns, dof = 6 (enabled edges) - 6 (free vertices), variance_factor = cost / dof when
 *              dof > 0, else 1: the a-posteriori variance factor sigma0^2.  Alignment Hessians used as Omega are overconfident (DESIGN.md
 *              3.18), so a caller who gates on a covariance scales it by variance_factor.
 *   gauge      a queried free vertex in a connected component (over enabled edges) without a fixed vertex makes H singular: the host finds
 *              it with a union-find, launches nothing, writes nothing to the outputs and returns RGBD360_ILL_POSED; the message names the
 *              first such query.
 *   cov. solve conjugate gradients as above (same preconditioner, same stop rule |r|_M <= cg_tol |r_0|_M) per right-hand side, six per query,
 *              up to 16 queries in lock step, further queries batch after batch; every column has its own scalars and stop word and is
 *              frozen once it stopped, so a query's bits do not depend on what shares its batch or on the order of the queries.  A query is
 *              finished when its six columns are; cg_iterations / cg_residual report the largest of the six.  p.q <= 0 on an unfinished
 *              column, or a diagonal block without a Cholesky factor: RGBD360_ILL_POSED.  Columns that have not stopped after cg_max_iters:
 *              RGBD360_NOT_CONVERGED, everything is still written, n_not_converged counts the queries that have such a column and the
 *              per-query arrays tell which (cg_residual > cg_tol).  Sums as above; one stream synchronisation per batch.
 * Out of scope: the second-order robust term, dynamic covariance scaling and switch variables, an adaptive delta, robust weights inside
 * the dense alignment, marginalisation (removing vertices from the graph), the full dense covariance, incremental solving, SE(2),
 * landmarks, several GPUs, a stronger preconditioner. */
typedef struct rgbd360_graph rgbd360_graph;
enum { RGBD360_GRAPH_ROBUST_NONE = 0, RGBD360_GRAPH_ROBUST_HUBER = 1, RGBD360_GRAPH_ROBUST_CAUCHY = 2, RGBD360_GRAPH_ROBUST_GEMAN_MCCLURE = 3 };
typedef struct {
    int    max_iters;          /* Levenberg-Marquardt iterations, 0 .. 10000: 10 */
    int    cg_max_iters;       /* per solve, 1 .. 100000: 400 */
    double tol_update;         /* on max |x| of an accepted step: 1e-6 */
    double lambda_init;        /* 1e-3 */
    double lambda_max;         /* 1e30 */
    double cg_tol;             /* 1e-8 */
} rgbd360_graph_params;
typedef struct {
    int status, iterations, accepted, converged;      /* RGBD360_OK / ILL_POSED; trace records; accepted steps; 1: ended on tol_update */
    double chi2_initial, chi2_final, lambda_final;
    long long cg_iterations;                           /* over all solves */
    int n_fixed, n_isolated;
} rgbd360_graph_result;
/* one Levenberg-Marquardt iteration: chi2 at the current poses, at the trial poses, the lambda of the solve, 1 when the step was taken,
 * the solve's iterations and |r|_M / |r_0|_M, max |x| of the step */
typedef struct { double chi2, chi2_trial, lambda; int accepted, cg_iterations; double cg_residual, max_update; } rgbd360_graph_iteration;
int  rgbd360_graph_create(rgbd360_ctx* ctx, rgbd360_graph** out);
void rgbd360_graph_destroy(rgbd360_graph* g);
const char* rgbd360_graph_last_error(rgbd360_graph* g);
/* n vertices; fixed: n bytes, NULL = none fixed.  Returns the index of the first new vertex; -1 (nothing added) for a negative n, a NULL
 * pose array or a non-finite entry (the message names the first such vertex of the call). */
int  rgbd360_graph_add_vertices(rgbd360_graph* g, int n, const float* poses, const uint8_t* fixed);
/* n edges from[k] -> to[k].  0; -1 and nothing added when an index is no vertex, from == to, an entry is not finite or the information
 * matrix has a non-positive diagonal entry (the message names the first such edge of the call).  Repeated edges and from > to are allowed. */
int  rgbd360_graph_add_edges(rgbd360_graph* g, int n, const int* from, const int* to, const float* rel_poses, const float* information);
int  rgbd360_graph_set_poses(rgbd360_graph* g, int first, int n, const float* poses);
int  rgbd360_graph_set_fixed(rgbd360_graph* g, int first, int n, const uint8_t* fixed);
int  rgbd360_graph_n_vertices(const rgbd360_graph* g);
int  rgbd360_graph_n_edges(const rgbd360_graph* g);
int  rgbd360_graph_clear(rgbd360_graph* g);
void rgbd360_graph_default_params(rgbd360_graph_params* p);
/* Returns the status (>= 0, also in result->status; result may be NULL); -1: bad parameters or no fixed vertex, nothing launched.  A graph
 * without vertices, edges or free vertices returns RGBD360_OK with 0 iterations. */
int  rgbd360_graph_optimize(rgbd360_graph* g, const rgbd360_graph_params* params, rgbd360_graph_result* result);
int  rgbd360_graph_get_poses(rgbd360_graph* g, int first, int n, float* out);
/* The cost at the current poses (the bits rgbd360_graph_optimize reports as chi2_initial from there): the sum of rho over the enabled
 * edges; per_edge (may be NULL): the raw s = r^T Omega r of every edge, enabled or not, so that a rejected closure can be tested again. */
int  rgbd360_graph_chi2(rgbd360_graph* g, double* chi2, double* per_edge);
/* Kind and delta of the edges first .. first + n - 1.  deltas may be NULL only when every kind is NONE; the delta of a NONE edge is
 * neither checked nor stored (a new edge's delta reads 1).  0; -1 and nothing changed when the range is outside the edges, a kind is outside 0..3, or the delta of a kind
 * other than NONE is not finite or <= 0 (the message names the first such edge).  rgbd360_graph_clear forgets the settings. */
int  rgbd360_graph_set_edge_robust(rgbd360_graph* g, int first, int n, const int* kinds, const double* deltas);
/* Switches edges off (0) and on (non-zero); -1 and nothing changed when the range is outside the edges. */
int  rgbd360_graph_set_edge_enabled(rgbd360_graph* g, int first, int n, const uint8_t* enabled);
/* What the two setters left; kinds, deltas and enabled may each be NULL. */
int  rgbd360_graph_get_edge_state(rgbd360_graph* g, int first, int n, int* kinds, double* deltas, uint8_t* enabled);
/* At the current poses, per edge: s, rho and w (rho = w = 0 for a disabled edge), and *cost, bit for bit what rgbd360_graph_chi2
 * returns.  Each of the four may be NULL. */
int  rgbd360_graph_edge_weights(rgbd360_graph* g, double* cost, double* s, double* rho, double* w);
/* the first min(max_trace, iterations) records of the last rgbd360_graph_optimize; *n_trace (may be NULL): iterations */
int  rgbd360_graph_get_trace(rgbd360_graph* g, int max_trace, int* n_trace, rgbd360_graph_iteration* trace);
typedef struct {
    int    cg_max_iters;       /* per right-hand side, 1 .. 100000: 1000 */
    double cg_tol;             /* in (0, 1): 1e-10 */
} rgbd360_graph_cov_params;
typedef struct {
    int status;                /* RGBD360_OK / ILL_POSED / NOT_CONVERGED */
    int n_queries, n_not_converged;
    int cg_iterations_max;     /* over the queries */
    double cg_residual_max;
    long long dof;             /* 6 (enabled edges) - 6 (free vertices) */
    double cost;               /* the bits rgbd360_graph_chi2 returns */
    double variance_factor;    /* cost / dof when dof > 0, else 1 */
    int n_fixed, n_isolated;
} rgbd360_graph_cov_result;
void rgbd360_graph_default_cov_params(rgbd360_graph_cov_params* p);
/* Sigma_vv of the n vertices `vertices` (`covariance` above): cov holds n x 36 doubles, each block column-major; cg_iterations and
 * cg_residual (n each) and result may be NULL, params NULL = the defaults.  Returns the status (also in result->status); -1 and nothing
 * launched when an index is no vertex (the message names the first such query), an array is NULL with n > 0, cg_max_iters is outside
 * 1 .. 100000 or cg_tol is not in (0, 1).  n == 0 returns RGBD360_OK. */
int  rgbd360_graph_marginals(rgbd360_graph* g, int n, const int* vertices, const rgbd360_graph_cov_params* params, double* cov,
                             int* cg_iterations, double* cg_residual, rgbd360_graph_cov_result* result);
/* C_ij of the n pairs (from[k], to[k]); arguments and return value as above. */
int  rgbd360_graph_relative_covariances(rgbd360_graph* g, int n, const int* from, const int* to, const rgbd360_graph_cov_params* params,
                                        double* cov, int* cg_iterations, double* cg_residual, rgbd360_graph_cov_result* result);

/* ---- one process, several GPUs (BASELINE.json configs[3]) ---------------------------------------------------
 * The sequence path shards by independent frame pairs: device d gets the contiguous pairs rgbd360_shard_range(n_frames-1, d,
 * n_gpus) and therefore the frames lo..hi (one boundary frame is shared by two neighbours); one host thread per device drives
 * that device's contexts as rgbd360_align360_batch does, no collective touches the data path, and ONE ncclAllGather (RCCL over
 * xGMI) of the per-pair result rows {pose[16], rgbd360_result} ends the call, after which every device holds the whole
 * trajectory (the host reads device 0's copy and checks it against the rows the shards produced).  The caller composes the
 * relative poses like OdometryRGBD360.cpp:257.  n_gpus == 1 runs without any RCCL call (RGBD360_FORCE_RCCL=1 in the
 * environment forces the one-rank exchange, for tests).  The handle owns the per-device contexts and the communicators:
 * create it once, align many sequences.  Replaces the role of the reference's single-threaded odometry loop
 * (Registration/OdometryRGBD360.cpp:141-297) for a recorded sequence. */
typedef struct rgbd360_multi rgbd360_multi;
/* device_ids: n_gpus distinct HIP device indices, NULL = 0..n_gpus-1.  Returns 0, -100 no HIP device, -101 bad device list,
 * -105 RCCL initialisation failed. */
int  rgbd360_multi_create(const rgbd360_params* p, int n_gpus, const int* device_ids, rgbd360_multi** out);
void rgbd360_multi_destroy(rgbd360_multi* m);
const char* rgbd360_multi_last_error(rgbd360_multi* m);
int  rgbd360_multi_n_gpus(rgbd360_multi* m);
int  rgbd360_multi_uses_rccl(rgbd360_multi* m);
/* rgbd360_set_index_arithmetic on every device's context of the handle (0: device definition, 1: the reference's libm arithmetic). */
int  rgbd360_multi_set_index_arithmetic(rgbd360_multi* m, int mode);
/* Contiguous balanced partition used by the sharding: the first n_items % world ranks get one item more. */
void rgbd360_shard_range(int n_items, int rank, int world, int* lo, int* hi);
/* Layout of the exchange step (ncclAllGather wants equal counts): every rank contributes rows_per_rank = ceil(n_pairs / world) result
 * rows, the first hi - lo of them its pairs; global pair `pair` is row *row of the gathered table and belongs to rank *rank.
 * Pure index arithmetic (no device): what rgbd360_multi_* use to scatter the gathered rows back into sequence order. */
void rgbd360_gather_slot(int n_pairs, int world, int pair, int* rank, int* row, int* rows_per_rank);
/* Host frames (as rgbd360_align360_batch: uploaded one frame ahead on each device's copy stream, unchanged until the call
 * returns).  poses_out: (n_frames-1) x 16 floats; results_out may be NULL.  Returns 0 or the first negative error. */
int  rgbd360_multi_align_sequence(rgbd360_multi* m, int n_frames, const uint8_t* const* rgb, size_t rgb_step,
                                  const void* const* depth, size_t depth_step, int depth_type, int rows, int cols,
                                  const float guess[16], int method, int occlusion, int n_inflight, float* poses_out,
                                  rgbd360_result* results_out);
/* Resident variant: _load_sequence copies every device's frames lo..hi into its HBM once (sized for 288 GB per device: a
 * 2048x1024 frame is 10.5 MB); _align_resident then aligns the whole sequence with no PCIe traffic but the result rows. */
int  rgbd360_multi_load_sequence(rgbd360_multi* m, int n_frames, const uint8_t* const* rgb, size_t rgb_step,
                                 const void* const* depth, size_t depth_step, int depth_type, int rows, int cols);
int  rgbd360_multi_align_resident(rgbd360_multi* m, const float guess[16], int method, int occlusion, int n_inflight,
                                  float* poses_out, rgbd360_result* results_out);
/* One-shot form (create + align_sequence + destroy): pays the communicator set-up on every call. */
int  rgbd360_align360_batch_multi(const rgbd360_params* p, int n_frames, const uint8_t* const* rgb, size_t rgb_step,
                                  const void* const* depth, size_t depth_step, int depth_type, int rows, int cols,
                                  const float guess[16], int method, int occlusion, int n_inflight, int n_gpus,
                                  const int* device_ids, float* poses_out, rgbd360_result* results_out);

/* ---- stage-level entry points (parity tests and measurement) ------------------------------------------------ */

/* Pyramid planes as float32 rows x cols (level dims via rgbd360_level_dims).
 * which: 0 graySrc 1 grayTrg 2 depthSrc 3 depthTrg 4 grayTrgGradX 5 grayTrgGradY 6 depthTrgGradX 7 depthTrgGradY
 * (the public pyramid vectors of RPI.h:198-199).  Gradients already carry the seam mask. */
int rgbd360_level_dims(rgbd360_ctx* ctx, int level, int* rows, int* cols);
int rgbd360_get_plane(rgbd360_ctx* ctx, int which, int level, float* host_out);
/* LUT_xyz_sphere of a level (RPI.h:4554-4587) as n x 3 floats; invalid points have x = -10000. */
int rgbd360_get_lut(rgbd360_ctx* ctx, int level, float* host_out_xyz);

/* One fused per-pixel pass at `pose` on `level`: errorPhotoICP_sphere (RPI.h:2545) and calcHessGrad_sphere
 * (RPI.h:2745) evaluated at the same pose.  Any output pointer may be NULL.
 * err2 / n_valid: sum of squared weighted residuals and their count (RPI.h:2707-2729), split photo / depth in
 * err2_split[2], n_split[2].  H (column-major) and g from float64 block partials of float32 rows. */
int rgbd360_eval(rgbd360_ctx* ctx, int level, const float pose[16], int method, double* err2, long long* n_valid,
                 double err2_split[2], long long n_split[2], float H[36], float g[6], double H64[36], double g64[6],
                 long long* n_visible);
/* The same pass in the occlusion-aware variants (occlusion 1: RPI.h:3232-3716, 2: RPI.h:3720-4249; 0 = rgbd360_eval).
 * n_split[] are the reference's nValidPhotoPts / nValidDepthPts (occlusion 2: both = nValidDepthPts), the error of
 * the alignment loop is sqrt(err2_split[0]/n_split[0]) + sqrt(err2_split[1]/n_split[1]). */
int rgbd360_eval_occ(rgbd360_ctx* ctx, int level, const float pose[16], int method, int occlusion, double* err2,
                     long long* n_valid, double err2_split[2], long long n_split[2], float H[36], float g[6], double H64[36],
                     double g64[6], long long* n_visible);
/* Warped target pixel of every source pixel of `level` under `pose`: out[2i] = r', out[2i+1] = c', -1 if the
 * pixel is invalid or leaves the image (RPI.h:2663-2684).  Host output, n x 2 int32. */
int rgbd360_warp_indices(rgbd360_ctx* ctx, int level, const float pose[16], int32_t* host_out_rc);
/* The source frame warped into the target frame at `pose`, and the two difference images: the per-pixel product of the
 * reference's visualisation path (warped_source_grayImage / warped_source_depthImage RPI.h:163-166, filled inside
 * calcHessGrad_sphere RPI.h:2779-2785, 3032-3033, 3066-3067; imgDiff / depthDiff RPI.h:4664-4676) without its windows.  Every
 * plane has the geometry of the target level (rows x cols, row-major); any output pointer may be NULL.
 *  - A source pixel i (flat index) is VISIBLE exactly when rgbd360_warp_indices reports a target (r', c') for it, in whichever
 *    index arithmetic the context is set to (rgbd360_set_index_arithmetic).
 *  - warped_gray (methods 0 and 2; zero-filled, RPI.h:2782): every visible i writes Isrc[i] at its target pixel, BEFORE the
 *    saliency test (RPI.h:3033 precedes 3038): non-salient target pixels take a value too.
 *  - warped_depth (methods 1 and 2; zero-filled): a visible i writes dist = |R p + t| (RPI.h:2976, 3067) where the target depth
 *    at (r', c') is finite (RPI.h:3064).  With method 2 the photometric `continue` (RPI.h:3038-3039) skips the depth block:
 *    only where NOT (|gx| < thres_sal_photo && |gy| < thres_sal_photo) of the target's gray gradient.
 *  - Collisions: the reference's loop runs i ascending and each write overwrites (RPI.h:2953; its OpenMP build races there).
 *    The sequential semantics hold here: the LARGEST source index that lands on a target pixel wins, identically from run to
 *    run.  Whether a target pixel takes depth writes depends on the target pixel alone, so the depth winner is the gray winner.
 *    winner: that source index per target pixel, -1 where nothing landed (any method).
 *  - diff_gray = |Itrg - warped_gray| (methods 0 and 2), diff_depth = |Dtrg - warped_depth| (methods 1 and 2), over the whole
 *    level, holes included (cv::absdiff, RPI.h:4664-4676); a non-finite target depth propagates.
 * A plane that does not apply to the method comes back zero.  Returns 0, -1 bad arguments, -2 frame missing, -3 bad level,
 * -4 bad method, -6 an rgbd360_align360_begin alignment is in flight. */
int rgbd360_warp_images(rgbd360_ctx* ctx, int level, const float pose[16], int method, float* warped_gray, float* warped_depth,
                        float* diff_gray, float* diff_depth, int32_t* winner);
/* The same with DEVICE output pointers (on the context's device): enqueued on the context's stream, returns without waiting
 * (rgbd360_sync, or further work on rgbd360_stream). */
int rgbd360_warp_images_dev(rgbd360_ctx* ctx, int level, const float pose[16], int method, float* warped_gray_dev,
                            float* warped_depth_dev, float* diff_gray_dev, float* diff_depth_dev, int32_t* winner_dev);
/* One Gauss-Newton step on the device from the H,g of the preceding rgbd360_eval... exposed for tests:
 * pose_tmp = exp(-H^-1 g) * pose (RPI.h:4682-4697).  Returns RGBD360_ILL_POSED when the rank test fails. */
int rgbd360_gn_step(rgbd360_ctx* ctx, const float H[36], const float g[6], float lambda, const float pose[16],
                    float pose_tmp[16], float update[6]);

/* Measurement and self-test entry points (forced iteration schedule, kernel timers, device arithmetic self-test) are not part
 * of the product ABI: include/rgbd360_hip_diag.h. */

/* The HIP stream all work of this context is enqueued on (hipStream_t as void*). */
void* rgbd360_stream(rgbd360_ctx* ctx);
int   rgbd360_sync(rgbd360_ctx* ctx);
/* Number of HIP devices visible; does not create a context. */
int   rgbd360_device_count(void);

/* ---- dense registration of two frames of the 8-sensor rig ---------------------------------------------
 * RegisterRGBD360::RegisterDensePhotoICP (RegisterRGBD360.h:344-520) over RegisterPhotoICP::calcPhotoICPError_robot
 * (RPI.h:4905-5076) and calcHessianGradient_robot (RPI.h:5083-5407): the unknown is the RIG's relative pose (p_rig1 = T p_rig2),
 * every sensor contributes its pinhole photometric / depth rows through its extrinsic Rt_s (sensor -> rig), the 8 sets of normal
 * equations add up, Levenberg-Marquardt on the sum (lambda 0.001, x / 10, one retry, full SE(3) exponential, tolerances 0.1 on
 * the summed squared error / 1e-6).  The reference function is broken as written; three defects are FIXED here and in the
 * oracle (oracle/photo_icp_ref.cpp documents them): new_error is evaluated at the candidate pose (RegisterRGBD360.h:462,488
 * use the old one), jacobianRt_z is row 2 of the transform Jacobian (RPI.h:5226-5228 leave it uninitialised), and the depth
 * residual uses the transformed point's depth (RPI.h:5037 uses the untransformed one).
 * Rt: n_sensors x 16 floats, column-major sensor -> rig poses (Calib360::Rt_); fx, fy, ox, oy: the sensors' level-0 intrinsics
 * (RegisterRGBD360.h:357-365: 525 * width / 640, centre).  All sensor images of a frame share one size. */
typedef struct rgbd360_rig rgbd360_rig;
int  rgbd360_rig_create(const rgbd360_params* p, int n_sensors, const float* Rt, float fx, float fy, float ox, float oy,
                        rgbd360_rig** out);
void rgbd360_rig_destroy(rgbd360_rig* rig);
const char* rgbd360_rig_last_error(rgbd360_rig* rig);
/* frame1 (target) / frame2 (source): n_sensors host images each, as rgbd360_set_target takes them; copied before return. */
int  rgbd360_rig_set_target(rgbd360_rig* rig, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                            size_t depth_step, int depth_type, int rows, int cols);
int  rgbd360_rig_set_source(rgbd360_rig* rig, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                            size_t depth_step, int depth_type, int rows, int cols);
/* One fused pass over all sensors at rig pose `pose`: err2_split = {photo, depth} sums of squared weighted residuals (no
 * saliency test; their sum is calcPhotoICPError_robot summed over the sensors), n_split the pixel counts, H / g the summed
 * normal equations (float, per-sensor totals added in sensor order), H64 / g64 the same in double, n_rows the Jacobian rows. */
int  rgbd360_rig_eval(rgbd360_rig* rig, int level, const float pose[16], int method, double err2_split[2], long long n_split[2],
                      float H[36], float g[6], double H64[36], double g64[6], long long* n_rows);
/* The registration.  Returns 0 or RGBD360_ILL_POSED (pose_out = the pose reached).  res->iters = accepted steps per level,
 * res->hessian = the summed Hessian of the last step (informationM, RegisterRGBD360.h:511), res->err_final = the summed
 * squared error at pose_out. */
int  rgbd360_rig_align(rgbd360_rig* rig, const float guess[16], int method, float pose_out[16], rgbd360_result* res);
/* useSaliency(true) on the per-sensor RegisterPhotoICP objects (RPI.h:266-269): calcPhotoICPError_robot and
 * calcHessianGradient_robot run over vSalientPixels only (RPI.h:4930-5003, 5121-5262: the same loop bodies over the list built by
 * calcGradientXY_saliency from the TARGET's gray gradients, RPI.h:401-425, used as source pixel indices).  Off by default, as in
 * every application of the reference. */
int  rgbd360_rig_use_saliency(rgbd360_rig* rig, int on, float thres_saliency);
/* The arithmetic of the rig's warp (rgbd360_set_index_arithmetic's modes) for every later rgbd360_rig_eval / rgbd360_rig_align; may be
 * set before or after the frames.  0 (default): the device definition -- one chain q = (T Rt_s) p, P' = Rt_s^-1 q for both passes,
 * fused multiply-adds, round-half-up.  1: the REFERENCE's arithmetic, whose two passes warp a pixel differently:
 * calcPhotoICPError_robot through relPoseCam = (Rt_s^-1 T) Rt_s formed in float (RPI.h:4923-4924, 5021-5029), calcHessianGradient_robot
 * through Rt_s^-1 (T (Rt_s p)) (RPI.h:5278-5290); Eigen's product order without fused multiply-adds, 1.0 / Z' and the projection in
 * double, round half away from zero.  Target indices, visibility and counts of both passes are bit-equal to the CPU checker's math_mode 0
 * restatement of the reference.  The Levenberg-Marquardt loop is the same in both modes.  Returns -1 for another mode. */
int  rgbd360_rig_set_index_arithmetic(rgbd360_rig* rig, int mode);
int  rgbd360_rig_get_index_arithmetic(rgbd360_rig* rig);

/* ---- Frame360 per-pixel stages ------------------------------------------------------------------------------ */

/* Spherical point cloud from a range panorama.
 * convention 0: Frame360::buildSphereCloud_fromImage (Frame360.h:555-612): depth u16 mm, phi offset 31.5 deg,
 *               xyz = d (sin phi, -cos phi sin theta, -cos phi cos theta), NaN where depth == 0.
 * convention 1: Frame360_stereo::buildSphereCloud (Frame360_stereo.h:454-512): depth f32 m valid in (0,15),
 *               phi = (row+166) step - pi/2, theta = col step - pi, xyz = d (sin theta cos phi, sin phi, cos theta cos phi).
 * convention 2: full-sphere RegisterPhotoICP convention (RPI.h:4567-4582) with depth_type as in set_source.
 * Output: xyz as rows*cols x 3 float32 (host).  */
int rgbd360_sphere_cloud(rgbd360_ctx* ctx, const void* depth, size_t depth_step, int depth_type, int rows, int cols,
                         int convention, float* host_out_xyz);

/* Normal map of an organised cloud (rows*cols x 3 float32, NaN = invalid): pcl::IntegralImageNormalEstimation with
 * AVERAGE_3D_GRADIENT, setMaxDepthChangeFactor(max_depth_change_factor), setNormalSmoothingSize(normal_smoothing_size),
 * setDepthDependentSmoothing(true), as configured at Frame360.h:949-957 (0.02, 8) and Frame360_stereo.h:854-862
 * (0.05, 8).  depth_mode 0 uses the z coordinate as "depth" like PCL, 1 the range |p| (full spheres).
 * normals_out: rows*cols x 3, NaN where PCL leaves the normal undefined; normals point towards the origin. */
int rgbd360_normals(rgbd360_ctx* ctx, const float* xyz, int rows, int cols, float max_depth_change_factor,
                    float normal_smoothing_size, int depth_mode, float* normals_out);
/* The chamfer (1 / 1.4) distance-to-depth-discontinuity map that drives the smoothing window (diagnostics). */
int rgbd360_distance_map(rgbd360_ctx* ctx, const float* xyz, int rows, int cols, float max_depth_change_factor,
                         int depth_mode, float* dist_out);

/* pcl::FastBilateralFilter<PointXYZRGBA> with setSigmaS(sigma_s) / setSigmaR(sigma_r) on an organised cloud (rows*cols x 3
 * float32, NaN = invalid): the smoothing Frame360 applies to every sensor cloud before its planes are segmented
 * (Frame360.h:40, 493-499: sigma_s 10 px, sigma_r 0.05 m).  PCL's bilateral-grid algorithm (third-party; restated, see
 * oracle/frame360_ref.cpp): only z changes, x and y are copied.  xyz_out may alias xyz. */
int rgbd360_bilateral_filter(rgbd360_ctx* ctx, const float* xyz, int rows, int cols, float sigma_s, float sigma_r, float* xyz_out);

#define RGBD360_HULL_MAX 64
/* One planar region: n . x + d = 0 with n towards the origin, curvature = lambda_min / trace(cov). */
typedef struct {
    float centroid[3];
    float normal[3];
    float d;
    float curvature;
    int   count;        /* inliers */
    int   root;         /* smallest pixel index of the region = its label */
    /* Extent descriptors -- the roles of mrpt::pbmap::Plane::areaHull / elongation / v3PpalDir (Frame360.h:1025-1037; MRPT is
     * third-party and not in the reference tree):
     *   area        area of the convex hull of the region's contour projected onto its plane (calcConvexHull +
     *               computeMassCenterAndArea): metric, whatever the pixel density.  The device reduces the boundary pixels to the
     *               region's extreme point in each of 1024 in-plane directions (eight interleaved sets of 128), the host runs hull + shoelace on those (an inscribed
     *               polygon: exact for sharp-cornered polygons, 0.01 % low for a disc, a few 0.1 % low where long edges are slightly bowed).  Frame360.h:1031 compares it with min_area_plane (0.12 m2),
     *               RegisterRGBD360.h:126-136 ranks planes by it.
     *   elongation  sqrt(l2 / l1), ppal_dir = eigenvector of l2: PCA of the inliers (l1 <= l2 the in-plane eigenvalues of their
     *               covariance beside the normal's l0), as calcElongationAndPpalDir does on the inlier cloud. */
    float area;
    float elongation;
    float ppal_dir[3];
    /* area_moment  12 sqrt(l1 l2): the rectangle with the inliers' second moments (rounds 1-2 reported this as `area`; pixel-density
     *              weighted, it reads a wall seen from a spherical image several times too small).  rgbd360_merge_planes rebuilds a
     *              piece's covariance from it; 0 in a caller-made record means "take area".
     * center_hull  mass centre of the hull polygon (what computeMassCenterAndArea leaves in v3center); hull_points = vertices of the
     *              hull (0: no hull was formed -- caller-made record, or fewer than three extreme points: area = area_moment then). */
    float area_moment;
    float center_hull[3];
    int   hull_points;
    /* Colour descriptors -- the roles of mrpt::pbmap::Plane::v3colorNrgb / dominantIntensity (calcMainColor2) and hist_H
     * (calcPlaneHistH), which Frame360.h:1045-1046 / Frame360_stereo.h:949-950 fill for every plane and the PbMap matcher's unary
     * colour constraint reads (configLocaliser_spherical.ini:19-21).  Filled when a colour image is registered for the plane call
     * (rgbd360_set_plane_color_image); color_count = 0 otherwise, and the matcher then skips its colour tests.
     *   color_nrgb   mean of the normalised colour (R, G, B) / (R + G + B) over the inliers with R + G + B > 0 (invariant to a global
     *                brightness change), color_dev its standard deviation per channel.  MRPT's calcMainColor2 takes the mean-shift
     *                mode of these values; the mean is what its calcMainColor takes, and the two coincide for a region of one colour.
     *   intensity    mean R + G + B (0..765) of the same pixels.
     *   hist_h       normalised histogram over ALL inliers: 72 bins of 5 degrees of hue for saturated pixels, [72] dark pixels
     *                (V <= 0.2), [73] unsaturated ones (S <= 0.2). */
    int   color_count;
    float color_nrgb[3];
    float color_dev[3];
    float intensity;
    float hist_h[74];
    /* The hull POLYGON itself -- mrpt::pbmap::Plane::polygonContourPtr, which Frame360::mergePlanes tests for proximity vertex by vertex and
     * edge by edge (Frame360.h:680-711) and mergePlane2 re-hulls: hull_n <= RGBD360_HULL_MAX vertices in the frame of the plane record,
     * counter-clockwise seen from the side the normal points to (the camera's side), on the fitted plane.  A hull of more vertices is
     * thinned to its extreme points in RGBD360_HULL_MAX evenly spaced in-plane directions (an inscribed polygon: < 0.2 % of the area of a
     * disc is lost).  hull_n = 0: the record carries no polygon (caller-made record, or no hull was formed). */
    int   hull_n;
    float hull[RGBD360_HULL_MAX][3];
    /* The DOMINANT colour -- what mrpt::pbmap::Plane::calcMainColor2 leaves in v3colorNrgb / dominantIntensity (Frame360.h:1046): the plane's
     * pixels thinned to about 2000 samples, then getMultiDimMeanShift_color: samples farther from the running mean than the norm of the
     * standard deviation are dropped for good, until half the samples are gone or the mean stops moving (third-party; restated in integer
     * arithmetic, so the CPU checker repeats it exactly).  On a surface of two colours (a poster on a wall) the mean lies between them and
     * moves with the share of each in view; the dominant colour does not.  color_mode_count = samples it was sought over (0: none --
     * no colour image, or a caller-made record: the matcher then compares color_nrgb / intensity), color_concentration = the share of the
     * samples it ended on (MRPT's `concentration`). */
    int   color_mode_count;
    float color_mode[3];
    float intensity_mode;
    float color_concentration;
} rgbd360_plane;

/* Registers the colour image that goes with the organised cloud of the context's next plane calls (rgbd360_plane_fit,
 * _frame_planes[_dev], _cloud_planes, _sensor_planes): rgb is rows x cols x 3 uint8 with rgb_step bytes per row, and cloud pixel
 * (r, c) takes the colour of image pixel (r * step + step / 2, c * step + step / 2) -- step 1 for a panorama or a full-resolution
 * sensor cloud, the down-sampling step for a down-sampled one (DownsampleRGBD.h:240, 285-287: the colour of the block's centre
 * pixel).  on_device = 0: rgb is host memory and is copied at once; 1: device memory that must stay valid through those calls.
 * The planes of a call whose cloud does not have (rows / step) x (cols / step) points come back without colour.  rgb = NULL clears.
 * Channel order: the three bytes of a pixel are taken as R, G, B.  The descriptors of two planes are only ever compared channel by
 * channel, so an image in OpenCV's B, G, R order (the reference's panorama, Frame360.h:594-596) gives the same matches -- with
 * color_nrgb / color_mode channel-swapped and hist_h a mirrored hue circle relative to MRPT's; swap the channels first if the records
 * are to be exchanged with an MRPT PbMap. */
int rgbd360_set_plane_color_image(rgbd360_ctx* ctx, const uint8_t* rgb, size_t rgb_step, int rows, int cols, int step, int on_device);

/* Planar regions of an organised cloud with normals: pcl::OrganizedMultiPlaneSegmentation::segment as configured at
 * Frame360.h:958-977 (min_inliers 80, angular 0.0398 rad, distance 0.02) / Frame360_stereo.h:863-882 (40, 0.05, 0.05):
 * PlaneCoefficientComparator (depth-dependent distance threshold) + organised connected components + per-region
 * centroid / covariance / smallest eigenvector / curvature (the values Frame360.h:984-996 copies into
 * mrpt::pbmap::Plane).  labels_out (may be NULL): per pixel the region's root pixel index, -1 for non-finite points.
 * Planes are returned in PCL's order (by first pixel), at most max_planes; when more regions pass the filters the
 * max_planes LARGEST (inlier count) are kept, and rgbd360_planes_available reports how many there were.
 * The inlier sums are exact 64-bit integer sums of terms rounded to 2^-28 m (m^2) -- order independent, ~20 x finer than the float
 * accumulators of PCL 1.7's computeMeanAndCovarianceMatrix; a region a few millimetres across whose smallest eigenvalue lies within
 * ~1e-8 m^2 of max_curvature x trace may still fall on the other side of the filter than a float64 evaluation puts it.  Errors of the
 * plane calls: -7 more than 4096 regions exceed min_inliers; -8 a region's sums would leave their exact range, decided before they are
 * used from its count N and m = the largest |x|, |y|, |z| of its points (of the grown inlier set with the refinement on): refused when
 * N (m^2 2^28 + 1) >= 2^63, i.e. N m^2 >= 3.4e10 m^2 (a whole 4096 x 2048 frame that is one region beyond 64 m), or when m >= 2896 m
 * (m^2 2^28 >= 2^51: a single term no longer rounds exactly). */
int rgbd360_plane_fit(rgbd360_ctx* ctx, const float* xyz, const float* normals, int rows, int cols, int min_inliers,
                      float angular_threshold, float distance_threshold, float max_curvature, int depth_mode,
                      int32_t* labels_out, rgbd360_plane* planes_out, int max_planes, int* n_planes_out);

/* Number of regions that passed every filter in the context's last plane call (rgbd360_plane_fit, _frame_planes[_dev],
 * _cloud_planes, _sensor_planes); larger than the returned n_planes when the caller's max_planes cut the list -- grow the
 * buffer and call again. */
int rgbd360_planes_available(rgbd360_ctx* ctx);
/* The `refine` half of pcl::OrganizedMultiPlaneSegmentation::segmentAndRefine (what Frame360.h:977 / :868 / Frame360_stereo.h:882
 * call) for every later plane call of this context: after `segment`, planes grow into neighbouring pixels of regions that did
 * not become planes when the pixel's point lies within distance_threshold of the plane (PCL's refinement comparator: 0.02 m, not
 * depth dependent) -- PCL's two raster passes, solved on the device by Jacobi sweeps to the same labels.  labels_out then holds
 * the refined labels; a plane keeps centroid / normal / d / curvature of `segment` (as PCL's PlanarRegion does), count and the
 * extent descriptors (area, elongation, ppal_dir) follow the grown inlier set.  Off by default (enabled = 0: plain `segment`). */
int rgbd360_set_plane_refinement(rgbd360_ctx* ctx, int enabled, float distance_threshold);
/* Pixels relabelled and Jacobi sweeps of the last plane call with refinement on. */
int rgbd360_plane_refinement_stats(rgbd360_ctx* ctx, int* pixels_relabelled, int* sweeps);

/* Range panorama -> sphere cloud -> normals -> planar regions in one call (cloud and normals stay on the device
 * between the stages); xyz_out / normals_out / labels_out may be NULL. */
int rgbd360_frame_planes(rgbd360_ctx* ctx, const void* depth, size_t depth_step, int depth_type, int rows, int cols,
                         int convention, float max_depth_change_factor, float normal_smoothing_size, int min_inliers,
                         float angular_threshold, float distance_threshold, float max_curvature, int depth_mode,
                         float* xyz_out, float* normals_out, int32_t* labels_out, rgbd360_plane* planes_out, int max_planes,
                         int* n_planes_out);

/* One sensor's organised cloud as Frame360::buildSphereCloud_rgbd360 hands it to the plane extraction (Frame360.h:479-481):
 * CloudRGBD::getPointCloud (OpenNI2_Grabber/FrameRGBD/CloudRGBD.h:107-166: pinhole, focal 525 * cols / 640, centre (cols/2 - 0.5,
 * rows/2 - 0.5)) followed by DownsampleRGBD::downsamplePointCloud (DownsampleRGBD.h:209-300: per step x step block and per
 * coordinate the element n/2 of the sorted valid values; step 1 = the plain cloud, DOWNSAMPLE_160 = 2; at most 4).  depth: uint16 mm,
 * host, depth_step bytes per row; a pixel is valid when it has a depth and min_depth < z < max_depth (metres; DownsampleRGBD's
 * defaults 0.3 / 10 -- the reference's CloudRGBD.h:133-150 compares metres with millimetre thresholds, which is not reproduced).
 * xyz_out: (rows/step) * (cols/step) x 3 float32, NaN = invalid. */
int rgbd360_sensor_cloud(rgbd360_ctx* ctx, const uint16_t* depth, size_t depth_step, int rows, int cols, int step, float min_depth,
                         float max_depth, float* xyz_out);
/* The same from either kind of sensor image: depth_type 0 = uint16 millimetres (as above), 1 = float32 METRES -- the image
 * Frame360::undistort leaves (CloudRGBD_Ext.h:61-75, 116-118: m_depthEigUndistort), whose points getPointCloudUndist keeps when
 * z > 0 && min_depth <= z <= max_depth (inclusive, in metres: :118) before DownsampleRGBD takes the medians. */
int rgbd360_sensor_cloud_ex(rgbd360_ctx* ctx, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int step,
                            float min_depth, float max_depth, float* xyz_out);

/* Frame360::getPlanesSensor for one organised sensor cloud (host, rows*cols x 3 float32, NaN = invalid), with the smoothing
 * that precedes it: pcl::FastBilateralFilter when sigma_s > 0 (Frame360.h:493-499: 10, 0.05), the normal map (Frame360.h:949-957:
 * 0.02, 8; depth_mode 0 = PCL's z), the planar regions (Frame360.h:958-996: 80 inliers, 0.0398 rad, 0.02 m) -- the cloud stays on
 * the device between the three stages -- and, when Rt (column-major 4x4, Calib360::Rt_, sensor -> rig) is not NULL, the
 * plane.transform(Rt) of Frame360.h:1046.  Planes in PCL's order; n towards the (new) origin, n . x + d = 0. */
int rgbd360_cloud_planes(rgbd360_ctx* ctx, const float* xyz, int rows, int cols, float sigma_s, float sigma_r,
                         float max_depth_change_factor, float normal_smoothing_size, int min_inliers, float angular_threshold,
                         float distance_threshold, float max_curvature, int depth_mode, const float Rt[16],
                         rgbd360_plane* planes_out, int max_planes, int* n_planes_out);

/* rgbd360_sensor_cloud + rgbd360_cloud_planes (depth_mode 0) as one call: the depth image is uploaded once and the cloud never
 * leaves the device -- one sensor of Frame360::buildSphereCloud_rgbd360 + getPlanesSensor (Frame360.h:479-499, 949-996, 1046). */
int rgbd360_sensor_planes(rgbd360_ctx* ctx, const uint16_t* depth, size_t depth_step, int rows, int cols, int step, float min_depth,
                          float max_depth, float sigma_s, float sigma_r, float max_depth_change_factor, float normal_smoothing_size,
                          int min_inliers, float angular_threshold, float distance_threshold, float max_curvature, const float Rt[16],
                          rgbd360_plane* planes_out, int max_planes, int* n_planes_out);
/* rgbd360_sensor_planes from either kind of sensor image (depth_type as in rgbd360_sensor_cloud_ex). */
int rgbd360_sensor_planes_ex(rgbd360_ctx* ctx, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int step,
                             float min_depth, float max_depth, float sigma_s, float sigma_r, float max_depth_change_factor,
                             float normal_smoothing_size, int min_inliers, float angular_threshold, float distance_threshold,
                             float max_curvature, const float Rt[16], rgbd360_plane* planes_out, int max_planes, int* n_planes_out);

/* ---- the sensors' intrinsic depth model: Frame360::undistort (Frame360.h:293-311, undistortDepthSensor :1084-1097) ------------
 * Calib360::loadIntrinsicCalibration (Calib360.h:104-119) loads one clams::DiscreteDepthDistortionModel per sensor from
 * Calibration/Intrinsics/distortion_model<N> and calls downsampleParams(2); Frame360::undistort applies it to each sensor's depth image
 * in metres before the clouds are built.  The model (CLAMS, Teichman et al.; vendored by the reference under
 * OpenNI2_Grabber/third_party/CLAMS) cuts the image into bins of pixels, each with a multiplier per depth slice; z becomes z * m with m
 * interpolated between the two slices around z when both saw >= 50 training examples (rgbd360_amd/csrc/depth_model.h restates file
 * layout and arithmetic).  These entries are host only, no context needed; the same correction on the device, for a whole rig, is
 * rgbd360_depth_undistort below.
 *   load:      0 ok, 1 cannot open, 2 not a model file / truncated / bins not divisible by `downsample`, -1 bad arguments.
 *   info:      dims = {width, height, bin_width, bin_height, num_bins_x, num_bins_y} after the down-sampling.
 *   undistort: rows x cols float32 metres, in place (0 = no measurement stays 0); the image must have the model's size (-1 otherwise). */
typedef struct rgbd360_depth_model rgbd360_depth_model;
int  rgbd360_depth_model_load(const char* path, int downsample, rgbd360_depth_model** out);
void rgbd360_depth_model_free(rgbd360_depth_model* model);
int  rgbd360_depth_model_info(const rgbd360_depth_model* model, int dims[6], double* bin_depth);
int  rgbd360_depth_model_undistort(const rgbd360_depth_model* model, float* depth_m, size_t depth_step, int rows, int cols);

/* ---- training the depth model against the map (csrc/depth_train.h) ---------------------------------------------------------------------
 * The eight model files above belong to one physical rig.  This is the training half of the same CLAMS code -- DiscreteFrustum::addExample
 * and DiscreteDepthDistortionModel::accumulate(ground_truth, measurement), OpenNI2_Grabber/third_party/CLAMS/
 * discrete_depth_distortion_model.cpp:21-36 and 193-217 -- with the ground truth taken from the resident map: the depth image a sensor
 * should have seen at a pose is one surface cast (rgbd360_map_raycast_surface) of the sensor's pinhole rays.  The loop CLAMS describes:
 * map from trusted short-range data (a near box, or a short t_max), train, save the models where Calib360::loadIntrinsicCalibration reads
 * them (Calib360.h:104-119), undistort, re-map.  A trainer has the shape of DiscreteDepthDistortionModel's constructor (:116-139):
 * num_bins_x = width / bin_width, num_bins_y = height / bin_height, every frustum with max_dist = 10 and num_bins = ceil(10 / bin_depth)
 * slices (CLAMS' defaults: bins of 8 x 6 pixels, bin_depth 2.0, smoothing 1), and keeps three 64-bit integer words per (frustum, slice) on
 * the device -- count, num, den, [num_bins_y][num_bins_x][num_bins], zero after create and clear; 320 x 240 with 4 x 3 bins: under 1 MB.
 * The sums are integers added by integer atomics: their bits do not depend on the order of the frames, the launch shape or the run.
 * An example is a ground-truth z `gt` and a measured z `meas`, float32 metres widened to double; all arithmetic float64 + - x / floor
 * without contraction.
 *   1 measurement   meas is a measurement iff it is finite and > 0 (depth_type 0, uint16 millimetres: non-zero, 0.001f (float)v in float32
 *                   as rgbd360_set_target scales it).  Otherwise the pixel counts in n_no_measurement.
 *   2 range         meas > max_range or gt > max_range: n_out_of_range.
 *   3 multiplier    mult = gt / meas; mult > max_mult || mult < min_mult: n_mult_rejected (addExample's comparison, in double, against the
 *                   doubles of the float32 parameters).
 *   4 slice         idx = min(num_bins - 1, (int)floor(meas / bin_depth)).
 *   5 frustum       (min(v / bin_height, num_bins_y - 1), min(u / bin_width, num_bins_x - 1)) of pixel (v, u).
 *   6 sums          count += 1; num += llrint(gt gt 1048576.0); den += llrint(gt meas 1048576.0): CLAMS' sums of gt^2 and gt meas at a
 *                   resolution of 2^-20 m^2.  With max_range <= 16 a term is below 2^28; a call is refused (-1, nothing launched) once the
 *                   examples so far plus rows cols reach 2^34, so no word can wrap.  n_examples.
 * Every pixel lands in exactly one counter of rgbd360_depth_train_stats; they sum to n_pixels.
 * Finalisation (host, float64): N = smoothing + num 2^-20, D = smoothing + den 2^-20, multiplier = (float)(N / D), or 1 when D == 0;
 * counts = (float)(smoothing + count); the file's numerators and denominators are (float)N and (float)D.
 * Stated differences from CLAMS: it keeps float32 running sums in pixel order (they depend on the order and saturate) and re-forms the
 * multiplier after every example; here the sums are exact integers and the multiplier is formed once.
 * Out of scope: continuing from a model file's float32 sums; several GPUs inside one trainer (rgbd360_depth_trainer_add_sums is the
 * seam).  Applying and judging the models on the device: rgbd360_depth_models_* below.  The extrinsics of the same rig:
 * rgbd360_map_calibrate_rig_* above. */
typedef struct rgbd360_depth_trainer rgbd360_depth_trainer;
typedef struct {
    rgbd360_map_raycast_params ray;      /* the map route's surface cast: the two casts' own defaults */
    rgbd360_map_normal_params  normal;
    int   require_plane;                 /* map route: only hits whose plane depth was taken: 1 */
    float min_cos_incidence;             /* map route: smallest |cos| between ray and normal, [0, 1]: 0 (off; a setting, not a measurement) */
    float min_mult, max_mult;            /* MIN_MULT, MAX_MULT (stream_sequence/typedefs.h:6-7): 0.7, 1.3; 0 <= min_mult <= max_mult */
    float max_range;                     /* (0, 16]: 10 */
} rgbd360_depth_train_params;
typedef struct {
    long long n_pixels, n_no_measurement, n_no_hit, n_off_plane, n_grazing, n_out_of_range, n_mult_rejected, n_examples;
} rgbd360_depth_train_stats;
/* 0; -1 (where the source asserts): width % bin_width != 0 or height % bin_height != 0, a side outside 1 .. 16384, bin_depth not positive,
 * smoothing < 0, more than 2^26 bins; -103 out of memory.  The trainer lives on the context's device and stream; destroy it first. */
int  rgbd360_depth_trainer_create(rgbd360_ctx* ctx, int width, int height, int bin_width, int bin_height, double bin_depth, int smoothing,
                                  rgbd360_depth_trainer** out);
void rgbd360_depth_trainer_destroy(rgbd360_depth_trainer* trainer);
const char* rgbd360_depth_trainer_last_error(rgbd360_depth_trainer* trainer);
int  rgbd360_depth_trainer_clear(rgbd360_depth_trainer* trainer);
void rgbd360_depth_default_train_params(const rgbd360_map* map, rgbd360_depth_train_params* p);
/* CLAMS' accumulate(ground_truth, measurement): two images of the trainer's size and of one depth_type (0 uint16 millimetres, 1 float32
 * metres), host memory or (on_device 1) device memory on the context's device.  A gt pixel that is 0, negative or not finite counts in
 * n_no_hit; otherwise steps 1-6.  params NULL: the defaults (only min_mult, max_mult and max_range matter here).  stats (may be NULL) is
 * host memory; the call waits.  -1, nothing launched: an image that is not the trainer's size, a NULL image, a row step shorter than a
 * row, a bad depth_type, max_range outside (0, 16], min_mult negative or above max_mult, a full trainer.  rows cols == 0: 0, zero
 * statistics, nothing launched. */
int  rgbd360_depth_trainer_accumulate_images(rgbd360_depth_trainer* trainer, const void* gt, size_t gt_step, const void* meas, size_t meas_step,
                                             int depth_type, int rows, int cols, int on_device, const rgbd360_depth_train_params* params,
                                             rgbd360_depth_train_stats* stats);
/* The ground truth cast out of the map (a map of the trainer's context; it is not written).  The ray of pixel (v, u) starts at o = the
 * translation of sensor_pose (world <- sensor, column-major; frame pose x Calib360::Rt_[s] for a rig); in the sensor frame
 * f = ((u - cx) / fx, (v - cy) / fy, 1) in float32, every operation rounded on its own, and d_k = (R_k0 f_x + R_k1 f_y) + R_k2 f_z, the
 * rounding of rgbd360_map_raycast_sphere.  Because f_z = 1 the ray parameter t is the sensor-frame z: gt is the surface cast's t, bit for
 * bit what rgbd360_map_raycast_surface returns for (o, d) under params->ray and params->normal.  Gates, in this order: a pixel without a
 * measurement casts no ray (n_no_measurement); a miss of any status: n_no_hit; with require_plane, a hit whose plane depth was not
 * taken: n_off_plane; with min_cos_incidence > 0, a hit without a normal or with |q| < min_cos_incidence sqrt((d_x d_x + d_y d_y) + d_z d_z),
 * q = (n_x d_x + n_y d_y) + n_z d_z the surface step's product in double: n_grazing; then steps 2-6.  gt_out (rows x cols float32, may be
 * NULL; device memory with on_device 1): the gt of every pixel that reached step 2, 0 elsewhere.  The coarse layer and the normal layer
 * are built or reused exactly as the surface cast does.  Refusals: those of the image route and of the two casts' parameters, a NULL or
 * foreign map, a pose or pinhole that is not finite, fx or fy zero, min_cos_incidence outside [0, 1].  An empty map, or rows cols == 0,
 * returns 0 with zero statistics (and a zero gt_out) and launches nothing.  The map's robust settings (rgbd360_map_set_align_robust) play
 * no part here or in the evaluator. */
int  rgbd360_depth_trainer_accumulate_map(rgbd360_depth_trainer* trainer, rgbd360_map* map, const void* meas, size_t meas_step, int depth_type,
                                          int rows, int cols, float fx, float fy, float cx, float cy, const float sensor_pose[16], int on_device,
                                          const rgbd360_depth_train_params* params, float* gt_out, rgbd360_depth_train_stats* stats);
/* The sums as host arrays [num_bins_y][num_bins_x][num_bins], and the sums of another trainer of the same shape added to this one (other
 * processes, other GPUs, a checkpoint): -1 for negative words, words no trainer can hold, or a trainer that would be full. */
int  rgbd360_depth_trainer_sums(rgbd360_depth_trainer* trainer, int64_t* count, int64_t* num, int64_t* den);
int  rgbd360_depth_trainer_add_sums(rgbd360_depth_trainer* trainer, const int64_t* count, const int64_t* num, const int64_t* den);
/* The model of the sums as they stand (the finalisation above; free it with rgbd360_depth_model_free), the same from host arrays without
 * a context (-1: a shape rgbd360_depth_trainer_create refuses, a NULL pointer, a negative word), and the file of a model in the layout
 * rgbd360_depth_model_load reads (0; 1 cannot open or write; -1 bad arguments): load followed by save reproduces a file byte for byte. */
int  rgbd360_depth_trainer_model(rgbd360_depth_trainer* trainer, rgbd360_depth_model** out);
int  rgbd360_depth_model_from_sums(int width, int height, int bin_width, int bin_height, double bin_depth, int smoothing, const int64_t* count,
                                   const int64_t* num, const int64_t* den, rgbd360_depth_model** out);
int  rgbd360_depth_model_save(const rgbd360_depth_model* model, const char* path);

/* ---- applying the depth models on the device (csrc/depth_apply.h) ----------------------------------------------------------------------
 * The step "undistort" of CLAMS' loop -- map, train, save, undistort, re-map, calibrate, repeat -- from device memory: the models of a
 * rig's S sensors resident on the device, 1 <= S <= RGBD360_RIG_CALIB_MAX_SENSORS, a NULL model meaning identity, all others of one
 * width x height.  The resident form is one packed, pointer-free blob that keeps every frustum's own num_bins and bin_depth and, per
 * slice, the float32 multiplier and count as loaded; every model rgbd360_depth_model_load or _from_sums can hold is represented exactly,
 * and a set whose blob would exceed 1 GiB is refused.  ONE __host__ __device__ function corrects a pixel on that blob: DiscreteFrustum's
 * index / undistort / interpolatedUndistort as csrc/depth_model.h restates them, operation for operation, without contraction --
 * the float64 floor(z / bin_depth), the !(q < num_bins - 1) clamp, start = (float)(bin_depth idx), the half-slice test in double, the
 * float32 fall-back z multipliers[max(idx, 0)] when a neighbour slice is missing or saw fewer than 50 examples, else the float64
 * interpolation and (float)((double)z mult).  Frustum of pixel (v, u): (min(v / bin_height, nby - 1), min(u / bin_width, nbx - 1)).  A z
 * that is 0, negative or NaN is left as it is (payload included); +Inf takes the fall-back branch, as on the host.  The host run of the
 * same function: rgbd360_depth_models_undistort_packed_host (rgbd360_hip_diag.h).
 * The two millimetre conversions (they differ for 38850 of the 65535 non-zero raw values, first 5, 9, 10, 11):
 *   rgbd360_depth_undistort            (float)(0.001 (double)raw): Frame360::undistort's and OpenCV's convertTo(.., 0.001)
 *   rgbd360_rig_depth_clouds, rgbd360_map_calibrate_rig_depth_models, rgbd360_depth_evaluate_map
 *                                      0.001f (float)raw: rgbd360_set_target's, the trainer's and rgbd360_map_calibrate_rig_depth's
 * All entries: -1 with rgbd360_last_error(ctx) set (the map's error string for _calibrate_rig_depth_models), nothing launched or
 * uploaded, outputs untouched, for a NULL pointer, an image size that is not the set's, a row step shorter than a row, a bad depth_type,
 * a sensor outside 0 .. S - 1, a set of another context, a pinhole that is not finite or fx / fy zero.  No images or rows cols == 0:
 * 0, nothing launched. */
typedef struct rgbd360_depth_models rgbd360_depth_models;
/* models[n_sensors] (host objects; they are not kept).  The set lives on the context's device and stream; destroy it first.  _bytes: the
 * device memory of the blob.  _set replaces one sensor's model (NULL: identity) after a training round, under the same size rules; it
 * waits for the stream before the blob changes. */
int    rgbd360_depth_models_create(rgbd360_ctx* ctx, const rgbd360_depth_model* const* models, int n_sensors, rgbd360_depth_models** out);
void   rgbd360_depth_models_destroy(rgbd360_depth_models* set);
size_t rgbd360_depth_models_bytes(const rgbd360_depth_models* set);
int    rgbd360_depth_models_set(rgbd360_depth_models* set, int sensor, const rgbd360_depth_model* model);
/* n images (depth_type 0 uint16 millimetres, 1 float32 metres; host memory, or device memory with on_device 1, then out_m too) corrected
 * by the models of sensors sensor_of_image[i] into float32 metres out_m[i] (row step out_step): ONE launch over all images, one lane per
 * pixel, ONE synchronisation.  With depth_type 1 out_m[i] may be the input itself.  For every image the output equals
 * rgbd360_depth_model_undistort run on the host on the same float32 image, byte for byte; bytes beyond cols in a padded output row are
 * not written.  set NULL (sensor_of_image is then not read), or a sensor without a model: the converted input. */
int    rgbd360_depth_undistort(rgbd360_ctx* ctx, const rgbd360_depth_models* set, const rgbd360_map_batch_frame* images, const int* sensor_of_image,
                               int n_images, int depth_type, int rows, int cols, int on_device, float* const* out_m, size_t out_step);
/* What rgbd360_map_calibrate_rig_depth does in its first launch, public and with the correction: image k S + s becomes the packed cloud
 * xyz_out_dev[3 rows cols (k S + s) ..] (device memory) in the SENSOR's frame, a NaN triple where there is no measurement.  Conversion
 * and ray are that call's; with a set (of n_sensors sensors) z is first corrected by sensor s's model, and a corrected z that is not
 * finite and positive gives a NaN triple.  set NULL, or a sensor without a model: the bytes of rgbd360_map_calibrate_rig_depth's launch.
 * Re-mapping with corrected depth is this call followed by rgbd360_map_insert_cloud (device memory) per (k, s) at T_k E_s. */
int    rgbd360_rig_depth_clouds(rgbd360_ctx* ctx, const rgbd360_depth_models* set, const rgbd360_map_batch_frame* images, int n_frames, int n_sensors,
                                int depth_type, int rows, int cols, float fx, float fy, float cx, float cy, int on_device, float* xyz_out_dev);
/* rgbd360_map_calibrate_rig_depth on corrected depth: poses, extrinsics, result, sensor records and trace are byte for byte those of
 * rgbd360_rig_depth_clouds followed by rgbd360_map_calibrate_rig_clouds (on_device 1) on its output; with set NULL those of
 * rgbd360_map_calibrate_rig_depth.  The set is of the map's context and of n_sensors sensors. */
int    rgbd360_map_calibrate_rig_depth_models(rgbd360_map* map, const rgbd360_depth_models* set, const rgbd360_map_batch_frame* depth, int depth_type,
                                              int rows, int cols, float fx, float fy, float cx, float cy, int n_frames, int n_sensors, int on_device,
                                              float* poses, float* extrinsics, const rgbd360_rig_calib_params* params, rgbd360_rig_calib_result* result,
                                              rgbd360_rig_calib_sensor* sensors);
/* A model judged against the map.  Ground truth, gates and counters are those of rgbd360_depth_trainer_accumulate_map, steps
 * "measurement" to "multiplier", bit for bit (the same device code), all taken on the RAW measurement, so both sums below range over
 * the same pixels, the n_examples of stats.  Per example, float64 without contraction: e_raw = meas - gt, e_cor = z' - gt, z' the
 * measurement corrected by `sensor`'s model (set NULL: z' = meas), float32 widened to double.  n = the examples; *_e = sum of
 * llrint(e 2^30), signed (the bias, in units of 2^-30 m); *_ee = sum of llrint(e e 2^30) (the mean square, 2^-30 m^2).  64-bit integer
 * atomics only, one add per wave and word after a reduction over the wave: the bits do not depend on the launch shape, the run or the
 * order of calls, and the sums of several images are joined by integer addition.  With max_range <= 16 a raw term is below 2^38 (and a
 * corrected one as long as z' stays below 2 max_range); a call of more than 2^24 pixels is refused, so no word can wrap.  Refusals:
 * those above and what accumulate_map refuses.  An empty map: 0 with zero statistics and sums. */
typedef struct { long long n, raw_e, raw_ee, cor_e, cor_ee; } rgbd360_depth_eval_sums;
int    rgbd360_depth_evaluate_map(rgbd360_ctx* ctx, rgbd360_map* map, const rgbd360_depth_models* set, int sensor, const void* meas, size_t meas_step,
                                  int depth_type, int rows, int cols, float fx, float fy, float cx, float cy, const float sensor_pose[16], int on_device,
                                  const rgbd360_depth_train_params* params, rgbd360_depth_train_stats* stats, rgbd360_depth_eval_sums* sums);

/* ---- pinhole single-sensor alignment ------------------------------------------------------ */

/* RegisterPhotoICP::setCameraMatrix (RPI.h:254-257): fx, fy, ox, oy of the full-resolution sensor image; the pyramid
 * levels scale them by 2^-level (RPI.h:571-575). */
int rgbd360_set_camera(rgbd360_ctx* ctx, float fx, float fy, float ox, float oy);
/* RegisterPhotoICP::alignFrames(pose_guess, method, occlusion) (RPI.h:4254-4512): coarse-to-fine alignment of two
 * pinhole RGB-D images (the frames given to rgbd360_set_target / _source of a context created with mask_seams = 0) with
 * the reference's Levenberg-Marquardt schedule (lambda 0.01, x10 / /10, 10 iterations, tolerances 1e-4 hard-coded at
 * RPI.h:4303-4308), errorPhotoICP (RPI.h:560-748) and calcHessGrad (RPI.h:754-1104), CPose3D::exp (full exponential).
 * The per-pixel passes run on the device, the damping loop on the host.  Reference quirks kept (occlusion 0): the error
 * divides both residual sums by the number of depth-valid pixels, so PHOTO_CONSISTENCY alone gives NaN and the guess comes
 * back (status RGBD360_NO_VALID_PIXELS); the error pass applies no saliency test while the H,g pass does.
 * occlusion 1 / 2 select errorPhotoICP_Occ1 / calcHessGrad_Occ1 (RPI.h:1107-1544) and errorPhotoICP_Occ2 /
 * calcHessGrad_Occ2 (RPI.h:1547-2030) in the SEQUENTIAL semantics of their source (index order; the OpenMP loops race on the
 * z-buffer), as written: Occ2's error gate compares the target depth with the point's INVERSE depth, and both H,g variants
 * sum a pixel's depth row only where its photometric residual is non-zero (DEPTH_CONSISTENCY alone: H = 0, ILL-POSED).
 * No application of the reference calls them (MethodsRegisterRGBD360.cpp:348 passes 0). */
int rgbd360_align_pinhole(rgbd360_ctx* ctx, const float guess[16], int method, int occlusion, float pose_out[16],
                          rgbd360_result* res);
/* RegisterPhotoICP::useSaliency(bool) (RPI.h:266-269) with thresSaliency (RPI.h:217: 0.01): the pinhole error pass
 * (occlusion 0) sums over vSalientPixels only -- the interior pixels whose TARGET gray gradient exceeds the threshold in x
 * or y (calcGradientXY_saliency RPI.h:401-425), used as SOURCE pixel indices (RPI.h:590-690, as written); H, g keep every
 * pixel (their salient branch is commented out, RPI.h:813-870).  No other path of this library reads the list. */
int rgbd360_use_saliency(rgbd360_ctx* ctx, int on, float thres_saliency);
/* One fused pinhole pass at `pose` (stage-level, for parity tests): error sums / counts of errorPhotoICP and H, g of
 * calcHessGrad; n_rows = Jacobian rows that entered the normal equations. */
int rgbd360_eval_pinhole(rgbd360_ctx* ctx, int level, const float pose[16], int method, double err2_split[2],
                         long long n_split[2], float H[36], float g[6], double H64[36], double g64[6], long long* n_rows);
/* The same with the occlusion mode (0: identical to rgbd360_eval_pinhole): error sums / counts of errorPhotoICP_Occ1/2 and
 * H, g of calcHessGrad_Occ1/2 at `pose`; n_rows = numVisiblePixels as the reference counts it (a target pixel's first
 * arrival counts twice, RPI.h:1421-1430). */
int rgbd360_eval_pinhole_occ(rgbd360_ctx* ctx, int level, const float pose[16], int method, int occlusion, double err2_split[2],
                             long long n_split[2], float H[36], float g[6], double H64[36], double g64[6], long long* n_rows);
int rgbd360_warp_indices_pinhole(rgbd360_ctx* ctx, int level, const float pose[16], int32_t* host_out_rc);
/* rgbd360_warp_images for the pinhole path (needs rgbd360_set_camera; calcHessGrad RPI.h:805-811, 1025-1026, 1050-1051):
 * visibility is rgbd360_warp_indices_pinhole's; warped_depth takes the transformed z (RPI.h:1051) WITHOUT a test of the target
 * depth, with method 2 under the same photometric `continue` (RPI.h:1031-1032).  Host outputs, same return codes. */
int rgbd360_warp_images_pinhole(rgbd360_ctx* ctx, int level, const float pose[16], int method, float* warped_gray,
                                float* warped_depth, float* diff_gray, float* diff_depth, int32_t* winner);

/* The same chain with the depth image already in HBM and the maps left there: *xyz_dev, *normals_dev (rows*cols*3 floats) and
 * *labels_dev (rows*cols int32; root pixel index of the region, -1 for invalid points) point into buffers owned by the context,
 * valid until its next Frame360 call; only the plane list comes back to the host (0.33 ms of kernels at 2048x1024 against
 * 8-10 ms when 56 MB of maps travel to pageable host memory). */
int rgbd360_frame_planes_dev(rgbd360_ctx* ctx, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols,
                             int convention, float max_depth_change_factor, float normal_smoothing_size, int min_inliers,
                             float angular_threshold, float distance_threshold, float max_curvature, int depth_mode,
                             rgbd360_plane* planes_out, int max_planes, int* n_planes_out, const float** xyz_dev,
                             const float** normals_dev, const int32_t** labels_dev);

/* ---- Frame360 input side (the two steps before the path) ------------------------------------------------------- */

/* Frame360::loadFrame (Frame360.h:231-266): reads one `sphere_images_%d.bin` (Boost binary archive of 8 x {RGB 8UC3,
 * depth 16UC1 mm} cv::Mat records).  Host-only.  rgb_out: 8*rows*cols*3 bytes, depth_out: 8*rows*cols uint16; pass
 * NULL buffers to query rows / cols first.  Returns 0, -2 cannot open, -3 truncated, -4 unexpected record. */
int rgbd360_load_frame_bin(const char* path, uint8_t* rgb_out, uint16_t* depth_out, int* rows, int* cols);

/* Frame360::stitchSphericalImage (Frame360.h:386-405, stitchImage :1099-1148): the 8 sensor images (contiguous
 * [8][sensor_rows][sensor_cols][3] uint8 and [8][sensor_rows][sensor_cols] uint16 mm, host) -> panorama of
 * W = sensor_rows*8 columns and H = int(W*0.5*60/180) rows (sphere_rgb_out H*W*3, sphere_depth_out H*W range in mm).
 * Rt_inv: 8 column-major 4x4 (Calib360::Rt_inv), K = {fx, fy, cx, cy} (Calib360.h:74-77). */
int rgbd360_stitch_sphere(rgbd360_ctx* ctx, const uint8_t* rgb8, const uint16_t* depth8, int sensor_rows, int sensor_cols,
                          const float Rt_inv[128], const float K[4], uint8_t* sphere_rgb_out, uint16_t* sphere_depth_out,
                          int* out_rows, int* out_cols);

/* ---- PbMap plane registration: the initial-guess provider in front of the path -------------- */

/* Thresholds of mrpt::pbmap::SubgraphMatcher (config_files/configLocaliser_spherical.ini / ..._sphericalOdometry.ini,
 * loaded at RegisterRGBD360.h:97-100) that the geometric and colour constraints below use. */
typedef struct {
    /* [unary] */
    float dist_d;                 /* odometry modes: |d_ref - d_trg| below this (m) */
    float angle_deg;              /* odometry modes: angle between the two normals below this (deg) */
    float elongation_threshold;   /* ratio of elongations below this */
    float area_threshold;         /* ratio of areas below this */
    /* [binary] */
    float dist_threshold;         /* ratio of the two centre distances below this */
    float angle_threshold_deg;    /* difference of the two inter-normal angles below this (deg) */
    float height_threshold;       /* difference of the perpendicular offsets of one centre over the other plane (m) */
    float cos_normal_threshold;   /* after the fit: n_ref . (R n_trg) of every matched pair above this */
    /* [global] */
    int   min_planes_recognition; /* fewer matches than this = "Insuficient matching" (RegisterRGBD360.h:312-316) */
    float max_curvature_plane;    /* planes above it never enter the subgraphs (RegisterRGBD360.h:121-150; Miscellaneous.h:54) */
    float min_area_plane;         /* Frame360.h:1034 drops smaller planes before they reach the PbMap (Miscellaneous.h:57) */
    float max_elongation_plane;   /* Frame360.h:1041 drops narrower planes (Miscellaneous.h:60) */
    /* planar modes: the rig moves on the floor; normals keep their component along this axis (0 = x, up in the sphere
     * frame of RPI.h:4567-4582) within planar_normal_tol, and horizontal planes keep d within dist_d */
    int   up_axis;
    float planar_normal_tol;
    /* pose fit */
    float max_conditioning;       /* largest / smallest eigenvalue of sum w n n^T above this = ill-conditioned translation */
    float sigma_dist, sigma_normal; /* scale of the information matrix: st. dev. of a plane offset (m) / normal (rad) */
    int   max_nodes;              /* budget of the interpretation-tree search (nodes); 0 = unlimited */
    /* [unary], colour (applied to a pair of planes that both carry colour, color_count > 0) */
    int   use_color;              /* 0: no colour test at all */
    float color_threshold;        /* |difference| of every channel of color_nrgb below this (ini: 0.07) */
    float intensity_threshold;    /* |difference| of intensity below this (ini: 150 on the 0..765 scale); <= 0: not tested */
    float hue_threshold;          /* Bhattacharyya distance sqrt(1 - sum sqrt(h1 h2)) of the two hist_h below this (ini: 0.45); <= 0: not
                                   * tested -- the default: the reference's own use of it is commented out (Frame360.h:673) */
} rgbd360_pbmap_params;

/* odometry = 0: configLocaliser_spherical.ini, 1: configLocaliser_sphericalOdometry.ini */
void rgbd360_pbmap_default_params(rgbd360_pbmap_params* p, int odometry);

/* RegisterRGBD360::RegisterPbMap (RegisterRGBD360.h:276-338): subgraph selection (setReference / setTarget :110-195:
 * planes under max_curvature_plane; if max_match_planes > 0 and there are more, the max_match_planes largest areas),
 * interpretation-tree matching of the two plane sets under unary + binary geometric constraints
 * (mrpt::pbmap::SubgraphMatcher::compareSubgraphs -- third-party; restated from the published method, Fernandez-Moral
 * et al., "Fast place recognition with plane-based maps", ICRA 2013), then the closed-form pose of the matched planes
 * with its information matrix (mrpt::pbmap::ConsistencyTest::estimatePoseWithCovariance -- third-party, restated:
 * rotation = SVD of sum w n_ref n_trg^T, translation = least squares on the plane offsets).  Host code, no device work.
 *   regist_mode: 0 DEFAULT_6DoF, 1 PLANAR_3DoF, 2 ODOMETRY_6DoF, 3 PLANAR_ODOMETRY_3DoF (RegisterRGBD360.h:258-264).
 *   pose_out: column-major 4x4, pose of the target frame seen from the reference, p_ref = R p_trg + t.
 *   info_out: column-major 6x6 information matrix in [t; w] order (left perturbation, like RPI.h:4697).
 *   match_out: n_ref entries, index of the matched target plane or -1.  area_matched_out: matched area in the
 *   reference frame (calcAreaMatched).  Any output pointer may be NULL.
 * Returns 0 good alignment, 1 insufficient matching (< min_planes_recognition; pose_out = identity),
 * 2 ill-conditioned (rotation or translation not observable from the matched normals) or inconsistent fit, -1 bad arguments. */
int rgbd360_register_planes(const rgbd360_plane* ref, int n_ref, const rgbd360_plane* trg, int n_trg, int max_match_planes,
                            int regist_mode, const rgbd360_pbmap_params* params, float pose_out[16], float info_out[36],
                            int32_t* match_out, int* n_matched_out, float* area_matched_out);

/* Frame360::mergePlanes (Frame360.h:655-733): the pieces several sensors (or several regions) hold of one surface become one
 * plane.  Same surface = the reference's explicit test: n_j . n_k > cos_normal (0.99), |d_j - d_k| < dist_d (0.45 m), and outlines
 * closer than proximity (0.3 m) at a pair of points whose difference lies within normal_offset (0.06 m) of plane j -- on the HULL
 * POLYGONS of the two records, as the reference does (Frame360.h:680-691 vertex against vertex, :694-711 edge against edge: the 3-D
 * segment-to-segment distance; round 6: no containment test -- the reference has none, a panel inside a wall's hull but farther than
 * `proximity` from its outline stays a plane of its own).  Records without a polygon (hull_n = 0: caller-made) are tested on the rectangle with their in-plane moments instead (corners,
 * edge midpoints, centre).  The merged plane is the exact pooled fit of the two pieces (covariances rebuilt from the records, combined
 * by inlier count -- mrpt's mergePlane2 pools the inliers and refits); its polygon is the convex hull of the two polygons' vertices
 * projected onto the pooled plane (mergePlane2 re-hulls the two contours), its area and centre that polygon's.
 * Planes above max_curvature are never merged (Frame360.h:659-661).  Regions smaller than min_area (0.12 m2) or narrower than
 * max_elongation (6) are dropped first: Frame360.h:1034,1041 never stores them, so the reference's merge never sees them (and the
 * record of a thin strip pins its normal too loosely to be pooled); malformed records are dropped too.  Host only.
 * out may not alias planes; returns -1 when max_out is too small (*n_out = needed). */
int rgbd360_merge_planes(const rgbd360_plane* planes, int n, float max_curvature, float min_area, float max_elongation, float cos_normal,
                         float dist_d, float proximity, float normal_offset, rgbd360_plane* out, int max_out, int* n_out);

/* Frame360::groupPlanes (Frame360.h:741-833), the step of Frame360::getPlanes (:615-639) between the eight getPlanesSensor calls and
 * mergePlanes: `planes` holds the sensors' plane lists one after the other (n_per_sensor[s] records of sensor s, in the rig frame:
 * rgbd360_sensor_planes / rgbd360_cloud_planes with that sensor's Rt), the output is the frame's list.  A plane of sensor s is pooled
 * (mergePlane2, as in rgbd360_merge_planes) into a plane that came from -- or absorbed a piece of -- sensor s - 1 when both are larger
 * than min_area (0.5 m2) and flatter than max_curvature (0.0013) as the source tests them (:764: area OR curvature for the new piece,
 * :770: area AND curvature for the absorbing one), n_j . n_k > cos_normal (0.99), |d_j - d_k| < dist_d (0.45 m) and their hull polygons
 * come within max_dist_hull (0.5 m) at a pair of points / edges whose difference lies within max_dist_parallel_hull (0.09 m) of the
 * absorbing plane (:788-815); otherwise it is appended.  The last sensor's candidates include the first sensor's planes (the ring of
 * sensors closes, :827-828).  Nothing is filtered here.  Host only.  out may not alias planes; -1 when max_out is too small
 * (*n_out = needed) or on bad arguments. */
int rgbd360_group_planes(const rgbd360_plane* planes, const int* n_per_sensor, int n_sensors, float max_curvature, float min_area,
                         float cos_normal, float dist_d, float max_dist_hull, float max_dist_parallel_hull, rgbd360_plane* out, int max_out,
                         int* n_out);

/* The tail of Frame360::getPlanesSensor (Frame360.h:1034-1068), between one sensor's regions (rgbd360_sensor_planes / _cloud_planes, already
 * in the rig frame) and local_planes_[sensor]: regions smaller than min_area (0.12 m2, :1034) or narrower than max_elongation (6, :1041)
 * are dropped; each remaining region flatter than max_curvature (0.0013) is pooled (mergePlane2, as in rgbd360_merge_planes) into the
 * first plane already kept, also flatter, that mrpt::pbmap::Plane::isSamePlane(plane, cos_normal 0.99, dist_normal 0.05 m,
 * proximity 0.2 m) accepts (:1056-1068) -- normals, the centres' distance along the kept plane's normal, and the outlines nearer than
 * proximity (centres, vertices, edges; MRPT, third-party: restated, unpinned) -- else appended, in input order.  Host only.
 * out may not alias planes; -1 when max_out is too small (*n_out = needed) or on bad arguments. */
int rgbd360_pool_sensor_planes(const rgbd360_plane* planes, int n, float max_curvature, float min_area, float max_elongation, float cos_normal,
                               float dist_normal, float proximity, rgbd360_plane* out, int max_out, int* n_out);

/* ---- planar regions of the map (csrc/map_planes.h) ---------------------------------------------------------------------------------
 * The voxel map segmented into planes: connected components of the occupied voxels under the per-voxel normals of "surface normals of
 * the map" above, each flat enough component an rgbd360_plane -- a PbMap of the global map, the other operand of
 * rgbd360_register_planes when a frame has to be placed in the map WITHOUT an initial guess (the reference's Relocalizer360,
 * include/Relocalizer360.h:78-93, runs RegisterPbMap of the lost frame against the planes of what it has mapped).  The result is a
 * function of the voxel set and the parameters alone: it does not depend on the order of insertion, the table's capacity, slot
 * indices, rehashes or the run.  Nothing here writes the table.  tests/map_planes_reference.py restates the definition in numpy.
 * Predicates: float64 + - x on the float32 values as stored, every operation rounded on its own (no contraction); a dot product is
 * ((x x' + y y') + z z').
 *   eligible  a voxel whose status is RGBD360_NORMAL_OK in the normal layer of this call's (min_count, min_support, max_flatness) -- the
 *             layer is built or reused exactly as the surface cast does -- and whose stored curvature is <= max_voxel_curvature.
 *   link      two eligible voxels u, v whose keys differ by one of the 26 non-zero offsets of {-1, 0, 1}^3 (an index outside the 21-bit
 *             range does not exist; tombstones and empty cells are absent) are linked iff |n_u . n_v| >= cos_angle (the absolute value:
 *             the canonical sign of a normal can flip between neighbours) and, with e = c_v - c_u of the read-out centroids (float64),
 *             |n_u . e| <= max_offset leaf and |n_v . e| <= max_offset leaf; the bound is the one product (double)max_offset x
 *             (double)leaf.  Symmetric bit for bit; an unordered pair counts once in n_links.
 *   region    a connected component of the link graph (a singleton is one).  Its root is the member with the smallest packed key, the
 *             (i_z, i_y, i_x) order of rgbd360_map_extract; the root's key3 is the region's label.
 *   sums      exact integers, unit weight per voxel (point density does not bias a wall's extent): N = member voxels, P = the sum of
 *             their counts and, with r the root's centroid and q_k = rint(((double)c_k - (double)r_k) x 2^16) (half to even), the three
 *             sums of q_k and the six of q_j q_k in 64-bit integers.
 *   range     with E = the largest |i_k - i_k(root)| over the members and the three axes, a region is in range iff
 *             N ((E + 2) (double)leaf 2^16)^2 < 2^62 in float64 (rgbd360_map_plane_sums_in_range, the diagnostics header): |q_k| is below
 *             (E + 2) leaf 2^16, so no sum can leave the int64 range.  Decided from N and E BEFORE any sum is read; a region with
 *             N >= min_voxels that is out of range makes the call return -8 (the frame plane calls' "region moments out of range") with
 *             no output touched.  At leaf 0.1 a region of 10^5 voxels may span 100 m.
 *   plane     from the sums alone, on the host in float64 (rgbd360_map_plane_from_sums): a region with N >= min_voxels whose curvature
 *             l0 / trace of the covariance of the voxel centroids is <= max_curvature.  centroid, normal, curvature, elongation, ppal_dir
 *             and area_moment as the frame plane calls derive them from their moments; the normal faces `viewpoint` (NULL: the world's
 *             origin), d = -n . centroid, count = P, root = the plane's ordinal in the returned list (its label, the root's key3, comes
 *             in root_key3_out), color_count = color_mode_count = 0: the matcher skips its colour tests.
 *   hull      the region's extreme members in the 64 in-plane directions RGBD360_MAP_PLANE_DIRS[k] = (a_k, b_k), about 1024 (cos, sin)
 *             of 2 pi k / 64, literal so that no library's cosine enters: with (u, v) a member centroid's float64 coordinates about the
 *             record's float32 centroid in the float32 basis (e1, e2) the host derived from the sums (the two in-plane eigenvectors), the
 *             member with the largest u a_k + v b_k, a tie going to the smaller key.  area, center_hull, hull_points, hull_n and hull[]
 *             are the frame plane calls' hull of those extremes; the vertices run counter-clockwise seen from the normal's side.
 *   selection planes come back by root key ascending.  When more than max_planes pass the filters the max_planes of largest N are kept,
 *             ties going to the smaller root key, still in root-key order; n_planes_available counts all that passed.
 * Known limits, not bugs: pairwise linking walks round gently curved surfaces and the region's curvature filter then drops the WHOLE
 * region (the behaviour of PCL's organised segmentation); a wall thicker than one voxel gives two parallel regions; regions are not
 * merged across gaps (rgbd360_merge_planes does that for callers who want it).
 * The label layer (32 bytes per table slot) lies in device memory beside the table and belongs to the map: built by the first call that
 * needs it, reused while the map is unwritten and the parameters stand, freed with the map or by rgbd360_map_release_planes, reported by
 * rgbd360_map_plane_bytes (rgbd360_map_bytes stays the table's size).  The calls work on a level of the pyramid as every reader does.
 * Out of scope: colour descriptors of map planes, device-side outputs, merging across gaps, incremental upkeep of the labels, labels
 * inside the ICPs, the keyframe loop and acceptance thresholds of Relocalizer360::relocalize (caller policy), several GPUs.  The map's
 * robust settings (rgbd360_map_set_align_robust) are not honoured here. */
typedef struct {
    int   min_count;             /* the normal layer's three (rgbd360_map_normal_params): 1 */
    int   min_support;           /* 5 */
    float max_flatness;          /* 0.05 */
    float max_voxel_curvature;   /* an eligible voxel's largest stored curvature, >= 0: +inf */
    float cos_angle;             /* smallest |n_u . n_v| of a link, in [0, 1]: cos 5 deg (voxel normals on a noisy wall were measured up to
                                    1.4 deg off, so two neighbours can differ by about 3 deg) */
    float max_offset;            /* largest offset of a neighbour's centroid along either normal, in leaves, >= 0: 0.5 */
    int   min_voxels;            /* smallest N of a plane, >= 1: 50 (0.125 m2 of voxels at the default leaf 0.05 m: the reference's
                                    min_area_plane, 0.12 m2) */
    float max_curvature;         /* largest region curvature of a plane, >= 0: 0.0013 (the reference's plane constant) */
    /* The defaults are settings, not measurements.  Probe (the numpy restatement on the relocalisation scene of
     * tests/map_planes_reference.py, an asymmetric room of nine faces at leaf 0.1 m, axis-aligned and again turned by 25 degrees): every
     * face is one region in both maps.  With min_voxels = 20, the first value tried, the turned copy also returned three slivers of 21, 21
     * and 42 voxels, columns of voxels along the junctions of oblique walls; 50 leaves exactly the nine faces in both, and the matcher
     * accepts the pair.  The other values stood as first chosen. */
} rgbd360_map_plane_seg_params;
typedef struct { long long n_voxels, n_eligible, n_links, n_regions, n_planes_available, n_voxels_in_planes; } rgbd360_map_plane_seg_stats;
static const short RGBD360_MAP_PLANE_DIRS[64][2] = {
    {1024, 0}, {1019, 100}, {1004, 200}, {980, 297}, {946, 392}, {903, 483}, {851, 569}, {792, 650}, {724, 724}, {650, 792}, {569, 851},
    {483, 903}, {392, 946}, {297, 980}, {200, 1004}, {100, 1019}, {0, 1024}, {-100, 1019}, {-200, 1004}, {-297, 980}, {-392, 946},
    {-483, 903}, {-569, 851}, {-650, 792}, {-724, 724}, {-792, 650}, {-851, 569}, {-903, 483}, {-946, 392}, {-980, 297}, {-1004, 200},
    {-1019, 100}, {-1024, 0}, {-1019, -100}, {-1004, -200}, {-980, -297}, {-946, -392}, {-903, -483}, {-851, -569}, {-792, -650},
    {-724, -724}, {-650, -792}, {-569, -851}, {-483, -903}, {-392, -946}, {-297, -980}, {-200, -1004}, {-100, -1019}, {0, -1024},
    {100, -1019}, {200, -1004}, {297, -980}, {392, -946}, {483, -903}, {569, -851}, {650, -792}, {724, -724}, {792, -650}, {851, -569},
    {903, -483}, {946, -392}, {980, -297}, {1004, -200}, {1019, -100}};
void      rgbd360_map_default_plane_seg_params(const rgbd360_map* map, rgbd360_map_plane_seg_params* p);
/* The planes of the map.  planes_out (max_planes records) and root_key3_out (3 ints per plane) receive min(max_planes, passed) planes,
 * n_planes_out their number; stats (exact counts, whatever max_planes; n_voxels_in_planes sums N over all planes that passed).  Any
 * output pointer may be NULL; params NULL: the defaults; viewpoint NULL: the origin.  Host arrays; the call waits.  Returns 0; an empty
 * map returns 0 with zero statistics and launches nothing.  -1 with rgbd360_map_last_error set and no output byte touched: min_count < 1,
 * min_support outside 1 .. 27, a negative or NaN threshold, cos_angle outside [0, 1], min_voxels < 1, max_planes < 0, a viewpoint that is
 * not finite.  -8: a region out of range (above). */
int       rgbd360_map_planes(rgbd360_map* map, const rgbd360_map_plane_seg_params* params, const float viewpoint[3], int max_planes,
                             rgbd360_plane* planes_out, int32_t* root_key3_out, int* n_planes_out, rgbd360_map_plane_seg_stats* stats);
/* One record per voxel with count > 0, in NO specified order; returns the voxel count, writes at most max_out records.  key3: the
 * voxel; label_key3: its region's root key3 (an ineligible voxel: its own key); plane_index: the ordinal, by root key ascending, of its
 * region among ALL planes that passed the filters -- the plane's place in rgbd360_map_planes' list whenever max_planes does not cut it
 * -- or -1 (no plane, or an ineligible voxel).  Refusals as above, and max_out < 0. */
long long rgbd360_map_plane_labels(rgbd360_map* map, const rgbd360_map_plane_seg_params* params, long long max_out, int32_t* key3,
                                   int32_t* label_key3, int32_t* plane_index);
/* Device memory of the label layer and its region lists (0: none); rgbd360_map_release_planes frees it, the next call rebuilds. */
size_t    rgbd360_map_plane_bytes(const rgbd360_map* map);
int       rgbd360_map_release_planes(rgbd360_map* map);

#ifdef __cplusplus
}
#endif

/* sensed-space overlap of stored frames (rgbd360_store_overlap*, rgbd360_overlap_*): part of this ABI, declared in a header of its own */
#include "rgbd360_overlap.h"

#endif /* RGBD360_HIP_H */
