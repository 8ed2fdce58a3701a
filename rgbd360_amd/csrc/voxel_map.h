// voxel_map.h -- a resident voxel-grid global map built from posed frames: the map half of the reference's odometry loop
//   filter.filterEuclidean(frame->sphereCloud); currentPose = currentPose * rigidTransf;
//   pcl::transformPointCloud(*frame->sphereCloud, *tc, currentPose); *viewer.globalMap += *tc; filter.filterVoxel(viewer.globalMap);
// (OdometryRGBD360.cpp:242-268; the same steps at OdometryKeyFrame360.cpp:316-343, SphereGraphSLAM.cpp:116-137, 193-209,
// KFsphere_SLAM.cpp:236, 558; the filter class is FilterPointCloud.h:63-99).  Part of the Frame360 translation unit
// (rgbd360_frame360.hip includes it behind its helpers: F360State, HIPC, sphere_tables_dev; map_align.h, the alignment of a frame against
// the map, follows it).
//
// Definition, per input point and in this order (tests/voxel_map_reference.py restates it in numpy):
//   1 point   from a sphere image: r360::sphere_point of the pixel, the bits of rgbd360_sphere_cloud; from a cloud: the three floats.
//             Skipped unless all three are finite.
//   2 box     in the frame's own coordinates, BEFORE the pose (filterEuclidean precedes transformPointCloud): kept iff
//             lo[k] <= p[k] <= hi[k], limits included (pcl::PassThrough).
//   3 pose    w_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k in float32, every product and sum rounded on its own (no fused multiply-add).
//   4 range   dropped and counted if a w_k is not finite or |w_k| >= 4096.
//   5 voxel   i_k = (int)floorf(w_k * inv_leaf), inv_leaf = 1.0f / leaf (PCL's floor(x * inverse_leaf_size)); the cell boundaries
//             do not depend on the cloud's bounds.
//   6 sums    per voxel: count, S_k += llrint((double)w_k * 2^20) in int64 (the product is exact, half to even), integer sums of
//             r, g, b.  Integer sums do not depend on the order of arrival: the map is the same from run to run and whatever the
//             order of the frames (the fixed-point moments of the plane stage, frame360_kernels.h).
// Read-out per occupied voxel: centroid_k = (float)((double)S_k / ((double)count * 2^20)), colour = S_c / count (integer division),
// the key and the count.
//
// Two deliberate differences from the reference:
//   * every point has weight one: the map is pcl::VoxelGrid applied ONCE to the concatenation of all inserted clouds.  The reference
//     re-filters the accumulated map for every frame (O(map) per frame), which turns the previous centroid into a single point of
//     the next average: there the order of the frames decides the result.  Insertion here is O(frame).
//   * the sums are integers, not PCL's float accumulators.
//
// The table: open addressing with linear probing in HBM, a power of two of 64-byte slots {key, count, Sx, Sy, Sz, Sr, Sg, Sb}, all
// 64-bit words.  key = the three biased 21-bit indices packed (i_z, i_y, i_x from the top: ascending keys are the order of PCL's
// idx = i0 + i1 dx + i2 dx dy), ~0 = empty, claimed by compare-and-swap; a key never changes once set.  Removal (map_edit.h, DESIGN.md
// 3.15) subtracts the integer terms an insertion added; a slot whose count reaches 0 keeps its key -- a TOMBSTONE: the probe runs stay
// intact -- and every reader takes count == 0 as absent; a later insert of that voxel finds the key and revives the slot.
//
//   k_vmap_insert   one lane per point (four per thread, 256 apart: the shape of k_sphere_cloud_s4; load_points, which the evaluation
//                   kernels of map_align.h and map_align_plane.h share).  Neighbouring pixels share
//                   voxels, so the block first merges its 1024 points in a 512-entry LDS hash (LDS atomics); then one lane per
//                   occupied LDS entry finds or claims the global slot, and eight lanes per entry add its seven sums over the
//                   slot's 64 contiguous bytes: one global update per distinct key per workgroup.  (The add phase walks all 512
//                   entries and skips the empty ones, so a wave-instruction carries as many slots as eight consecutive entries
//                   hold; listing the occupied entries densely first is the open alternative, to be decided by measurement.)  A
//                   point whose LDS probe sequence (16) is exhausted goes to the global table on its own.  A new voxel that finds
//                   no free slot is dropped and counted; points of voxels already in the table are still added.
//   probe bound     a key's probe sequence in HBM ends after kMaxProbes = 2048 slots (the whole table when it is smaller): a key not
//                   found by then is dropped and counted as if the table were full.  Without the bound a full table would make
//                   every new key walk all of it (a frame of new voxels in a full 2^22-slot table: 10^11 dependent loads, one
//                   kernel running for minutes).  With it a key costs at most 128 KiB of loads.  A linear-probing run of length L at
//                   load a has probability about exp(-(a - 1 - ln a) L): below 1e-11 at a = 0.85 and L = 2048, so the bound binds
//                   only above about 90 % load -- size the table for twice the voxels expected.
//   removal         the same kernel text with MODE = kRemove: the same load, classify and LDS merge; the slot phase looks the key up
//                   read-only (find: removal never claims) and takes the entry's points off the count word in a compare-and-swap
//                   loop that refuses to go below zero; the eight-lane phase adds the two's-complement negatives of the six sums.
//                   MODE = kInsertRevive is the insert of a map that may hold tombstones: a new voxel is then the count add that
//                   returned 0 (a claim or a revival), not the claim, which costs a returning atomic per entry; a map that never had
//                   a voxel emptied keeps kInsert, the claim count.
//   k_vmap_extract  one lane per slot; a wave reserves its output range with one counter add and every lane stores its record.
//   host            every entry of the map that takes a frame or a cloud (here, map_edit.h, map_align.h, map_align_plane.h) describes it as
//                   one MapInput, has vmap_check refuse it before anything is touched and vmap_to_device make it the kernels' Source
//                   (MapSource: with which of its two forms it is; vmap_grid: its launch grid) -- DESIGN.md 3.16.  One launch of the
//                   extract kernel (vmap_launch_extract), one read-back of the counter words (vmap_copy_stats / vmap_read_stats), one
//                   scaffold of the rgbd360_map_time_* entries (VmapTimer).
#pragma once
#include <memory>

#include "map_table.h"

// a planar region that passed the filters (map_planes.h), as the map keeps it between calls: what rgbd360_map_plane_from_sums takes, the
// in-plane frame its extremes were taken in and those extremes
struct VmapPlaneRec {
    unsigned long long root_key;
    long long n_voxels, n_points, sums[9];
    float root_centroid[3], origin[3], e1[3], e2[3];
    float uv[64][2];
};

struct rgbd360_map {
    rgbd360_ctx* ctx = nullptr;
    F360State* s = nullptr;              // the context's Frame360 state: device, stream, the resident angle tables (not owned)
    float leaf = 0.f, inv_leaf = 0.f;
    unsigned long long n_slots = 0;      // a power of two
    bool has_box = true;
    float lo[3] = {-2.f, -4.f, -4.f}, hi[3] = {1.f, 4.f, 4.f};      // FilterPointCloud.h:66-71
    long long n_voxels = 0;              // slots with count > 0
    bool may_hold_tombstones = false;    // a removal has emptied a voxel since the last clear / rehash: inserts count revivals (kInsertRevive)
    long long last_updates = 0;          // global updates of the last insert call (measurement)
    std::string err;
    DevBuf<unsigned long long> table, d_stats;
    PinnedBuf<unsigned long long> h_stats;
    DevBuf<uint8_t> up_depth, up_rgb;    // a host frame / cloud on its way to the kernel
    DevBuf<uint8_t> up_normal;           // ... and a host cloud's normals (map_align_gicp.h)
    DevBuf<float> x_xyz;                 // the host read-out's device side
    DevBuf<uint8_t> x_rgb;
    DevBuf<int32_t> x_count, x_key;
    // alignment against the map (map_align.h): one partial row per workgroup, the loop's state with its trace behind it, the state's
    // pinned copy, and the trace of the last alignment as the host keeps it
    DevBuf<double> a_part;
    DevBuf<unsigned char> a_state;
    PinnedBuf<unsigned char> a_host;
    std::vector<rgbd360_map_align_trace> a_trace;
    // ... the robust kernel of each method (RGBD360_MAP_METHOD_*; map_align_robust.h): a setting, no layer and no revision; a level reads
    // its root's.  What the last single alignment and the jobs of the last batch did with it.
    rgbd360_map_robust robust[4] = {};
    rgbd360_map_robust_info a_robust = {};
    std::vector<rgbd360_map_robust_info> b_robust;
    // ... and of many in lock step (map_align_batch.h): the jobs and the prefix of their workgroup counts, on the device and pinned; the
    // traces of the last batch, one per job
    DevBuf<unsigned char> b_desc;
    PinnedBuf<unsigned char> b_desc_host;
    std::vector<std::vector<rgbd360_map_align_trace>> b_trace;
    // ... and of a rig calibration (rig_calib.h): the block that is copied back with its pinned copy, the work records, the clouds and
    // image descriptors of a _depth call, the trace of the last call
    DevBuf<unsigned char> c_out, c_work, c_img;
    PinnedBuf<unsigned char> c_host, c_img_host;
    DevBuf<float> c_cloud;
    std::vector<rgbd360_rig_calib_step> c_trace;
    // the map rendered as a spherical frame (map_render.h, in the other translation unit through map_table.h): the two work planes, the
    // counters with their pinned copy, the host entry's outputs on the device
    DevBuf<uint32_t> r_dist;
    DevBuf<unsigned long long> r_key, r_stats;
    PinnedBuf<unsigned long long> r_hstats;
    DevBuf<uint8_t> r_stage;
    // ray casting (map_raycast.h).  revision: bumped on the host by every entry that writes the table (insert, remove, move, clear, rehash);
    // the coarse layer and the live-key bounds are those of revision rc_rev and are rebuilt when the two differ
    unsigned long long revision = 1, rc_rev = 0;
    DevBuf<unsigned long long> rc_bkeys, rc_masks, rc_stats;      // brick keys, brick masks (eight words each), the counters
    DevBuf<uint32_t> rc_bidx;                                     // per brick slot: the brick's number
    DevBuf<unsigned> rc_words;                                    // the layer scan's bounds and brick count ...
    PinnedBuf<unsigned> rc_hwords;                                // ... and their pinned copy
    PinnedBuf<unsigned long long> rc_hstats;
    unsigned long long rc_bslots = 0, rc_bricks = 0;
    int rc_lo[3] = {0, 0, 0}, rc_hi[3] = {-1, -1, -1};            // the live box, unbiased cell indices
    DevBuf<float> rc_tab, rc_rays;                                // a panorama's angle tables (of rc_tab_rows x rc_tab_cols); a host list's rays
    int rc_tab_rows = 0, rc_tab_cols = 0;
    DevBuf<uint8_t> rc_stage;                                     // the host entries' outputs on the device: 27 bytes per ray
    bool rc_plain = false;                                        // the one-level traversal (rgbd360_map_raycast_set_plain)
    // surface normals (map_normals.h): one 16-byte record per slot, those of revision nm_rev under the three fit parameters nm_*; rebuilt
    // when the revision or a parameter differs
    unsigned long long nm_rev = 0;
    int nm_min_count = 0, nm_min_support = 0;
    float nm_max_flatness = 0.f;
    DevBuf<uint4> nm_layer;
    DevBuf<unsigned long long> nm_stats;                          // the build's counters and the read-out's record counter ...
    PinnedBuf<unsigned long long> nm_hstats;                      // ... and their pinned copy
    DevBuf<uint8_t> nm_stage;                                     // the host read-out's records on the device: 48 bytes each
    // colour (map_colour.h): one 16-byte record per slot (intensity with the status in its two top bits, the tangent-plane gradient), those
    // of revision cl_rev under the five fit parameters cl_params; rebuilt when the revision or a parameter differs
    unsigned long long cl_rev = 0;
    rgbd360_map_colour_params cl_params = {};
    DevBuf<uint4> cl_layer;
    DevBuf<unsigned long long> cl_stats;
    PinnedBuf<unsigned long long> cl_hstats;
    DevBuf<uint8_t> cl_stage;                                     // the host read-out's records on the device: 48 bytes each
    // free-space observation and carving (map_carve.h): one vote word per slot (through-votes low, end-votes high), taken on the table of
    // revision vt_rev; vt_rays_n: the measurements accumulated in it, vt_voted: the slots with a non-zero word; vt_spent: a carve has used it
    DevBuf<unsigned long long> vt_votes, vt_stats;
    PinnedBuf<unsigned long long> vt_hstats;
    DevBuf<int32_t> vt_out;                                       // the read-out's records on the device: six words each
    DevBuf<float> vt_rays;                                        // a host list's origins and endpoints
    unsigned long long vt_rev = 0;
    long long vt_rays_n = 0, vt_voted = 0;
    bool vt_have = false, vt_spent = false;
    // planar regions (map_planes.h): the label layer (32 bytes per slot) and the region lists of revision pl_rev under the parameters
    // pl_params, with the planes that passed the filters as the host keeps them (root key ascending); rebuilt when either differs
    unsigned long long pl_rev = 0;
    rgbd360_map_plane_seg_params pl_params = {};
    DevBuf<unsigned long long> pl_layer;                          // per slot: smallest key, points | root slot, voxels, extent, region id
    DevBuf<unsigned long long> pl_roots, pl_sums, pl_stats;       // eight words / nine sums per qualifying region; the counters
    PinnedBuf<unsigned long long> pl_hstats;
    DevBuf<int> pl_plane_of, pl_cursor;                           // per qualifying region: its plane's ordinal or -1; per plane: members scattered
    DevBuf<unsigned long long> pl_offset, pl_members;             // per plane: where its members start; three words per member (u, v, key)
    DevBuf<float> pl_frames;                                      // per plane: origin, e1, e2 (nine floats, padded to twelve)
    DevBuf<unsigned long long> pl_ranges, pl_partial, pl_extremes;      // the extremes' work: ranges of the lists, the chunks' winners, the planes' 64
    DevBuf<int32_t> pl_stage;                                     // the label read-out's records on the device: seven words each
    std::vector<VmapPlaneRec> pl_planes;
    rgbd360_map_plane_seg_stats pl_host_stats = {};
    bool pl_merge_waves = true;                                   // (rgbd360_map_time_planes: the sums pass without its per-wave merge)
    // the map pyramid (map_pyramid.h).  levels[s - 1]: level s of this map, the map of leaf * 2^s merged out of this table, owned here and
    // built on demand.  parent != null: this map IS such a level (of shift `shift`), a borrowed handle that every reading entry takes and
    // every writing entry refuses (vmap_refuse_level); lv_rev: the parent's revision its content is that of (0: never built)
    rgbd360_map* parent = nullptr;
    int shift = 0;
    unsigned long long lv_rev = 0;
    std::vector<std::unique_ptr<rgbd360_map>> levels;
    // composing maps (map_merge.h): a record list on the device, the read-out's or a host list's on its way to the kernel
    DevBuf<unsigned long long> mg_records;
};

namespace vmap {

constexpr int kThreads = 256, kPerThread = 4, kTile = kThreads * kPerThread;
constexpr int kLdsSlots = 512, kLdsProbes = 16;
// (the slot layout kFields / kEmpty / kBias / kFix, the probe bound kMaxProbes and the hash mix64: map_table.h)
enum { kStValid, kStBox, kStRange, kStAdded, kStDropped, kStNew, kStUpdates, kStExtract, kStUnderflow, kStWords };
// what k_vmap_insert does with the points.  kRemove reads the counters as: kStAdded points removed, kStDropped points whose key is not in
// the table (missing), kStNew voxels emptied, kStUnderflow points refused because the count would go below zero
enum { kInsert, kRemove, kInsertRevive };
constexpr int kStInsertWords = kStUnderflow;      // the words an insert uses: its clear in front of the kernel stays ONE 64-byte fill

struct Params {
    float pose[16];
    float lo[3], hi[3];
    int has_box;
    float inv_leaf;
};
struct Source {                  // SRC 0: a sphere image; SRC 1: a cloud of n points
    const void* depth;
    size_t depth_step;
    const uint8_t* rgb;          // 8UC3 rows / n x 3 bytes; null: the colour sums stay 0
    size_t rgb_step;
    int depth_type, rows, cols, convention;
    const float *sin_theta, *cos_theta, *sin_phi, *cos_phi;
    const float* xyz;
    long long n;
};

// step 5: the key of the voxel that the posed point w (step 4 passed: |w_k| < 4096) feeds
__device__ __forceinline__ unsigned long long point_key(const float w[3], float inv_leaf) {
#pragma clang fp contract(off)
    unsigned long long i[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) i[k] = (unsigned long long)((int)floorf(w[k] * inv_leaf) + kBias);
    return pack_key(i[0], i[1], i[2]);
}
// steps 1-6 of one point: 0 skipped, 1 outside the box, 2 out of range, 3 kept (key, the three fixed-point terms and the posed point w)
__device__ __forceinline__ int classify(const Params& P, float x, float y, float z, unsigned long long& key, long long f[3], float w[3]) {
#pragma clang fp contract(off)
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return 0;
    if (P.has_box && !(P.lo[0] <= x && x <= P.hi[0] && P.lo[1] <= y && y <= P.hi[1] && P.lo[2] <= z && z <= P.hi[2])) return 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = ((P.pose[k] * x + P.pose[k + 4] * y) + P.pose[k + 8] * z) + P.pose[k + 12];
    if (!(fabsf(w[0]) < 4096.f && fabsf(w[1]) < 4096.f && fabsf(w[2]) < 4096.f)) return 2;
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = llrint((double)w[k] * kFix);
    key = point_key(w, P.inv_leaf);
    return 3;
}
__device__ __forceinline__ int classify(const Params& P, float x, float y, float z, unsigned long long& key, long long f[3]) {
    float w[3];
    return classify(P, x, y, z, key, f, w);
}

// The source load of a thread: its N points (kPerThread unless stated; map_carve.h takes one), kThreads apart in the workgroup's tile of
// kThreads N points, all loads first.  in[k]: slot k holds a point of the source; index[k]: its place in the per-point arrays (a place
// inside the source where !in[k]: every load is in bounds).  (bx, by): the workgroup's tile and image row -- blockIdx in a launch over
// one source (the second form below), the job's own in a launch over many (map_align_batch.h).
template <int SRC, int N = kPerThread>
__device__ __forceinline__ void load_points(const Source& src, unsigned bx, unsigned by, float x[N], float y[N], float z[N], bool in[N], long long index[N]) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    if (SRC == 0) {
        const int r = by;
        const uint8_t* drow = (const uint8_t*)src.depth + (size_t)r * src.depth_step;
        const float sp = src.sin_phi[r], cp = src.cos_phi[r];
        float d[N], st[N], ct[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int col = bx * (kThreads * N) + t + kThreads * k;
            in[k] = col < src.cols;
            const int cc = in[k] ? col : src.cols - 1;
            index[k] = (long long)r * src.cols + cc;
            d[k] = src.depth_type == 0 ? 0.001f * (float)((const uint16_t*)drow)[cc] : ((const float*)drow)[cc];
            st[k] = src.sin_theta[cc];
            ct[k] = src.cos_theta[cc];
        }
#pragma unroll
        for (int k = 0; k < N; ++k) r360::sphere_point(src.convention, d[k], sp, cp, st[k], ct[k], x[k], y[k], z[k]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const long long i = (long long)bx * (kThreads * N) + t + kThreads * k;
            in[k] = i < src.n;
            const size_t ii = in[k] ? (size_t)i : 0;
            index[k] = (long long)ii;
            x[k] = src.xyz[3 * ii];
            y[k] = src.xyz[3 * ii + 1];
            z[k] = src.xyz[3 * ii + 2];
        }
    }
}
template <int SRC, int N = kPerThread>
__device__ __forceinline__ void load_points(const Source& src, float x[N], float y[N], float z[N], bool in[N], long long index[N]) {
    load_points<SRC, N>(src, blockIdx.x, blockIdx.y, x, y, z, in, index);
}

// the slot of `key`, claimed if the key is new; -1: the key is new and no free slot lies within the probe bound
__device__ __forceinline__ long long find_or_claim(unsigned long long* table, unsigned long long mask, unsigned long long key, bool& claimed) {
    unsigned long long slot = mix64(key) & mask;
    const unsigned long long n_probes = mask < kMaxProbes ? mask + 1 : kMaxProbes;
    for (unsigned long long p = 0; p < n_probes; ++p) {
        unsigned long long* kp = table + slot * kFields;
        unsigned long long k0 = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k0 == kEmpty) {
            k0 = atomicCAS(kp, kEmpty, key);
            if (k0 == kEmpty) {
                claimed = true;
                return (long long)slot;
            }
        }
        if (k0 == key) return (long long)slot;
        slot = (slot + 1) & mask;
    }
    return -1;
}

// removal's slot step for the `n` points of `key`: the slot, its count lowered by n.  -1 and a counter raised: the key is not in the table
// (n missing), or the slot holds fewer than n points: the decrement is clamped to what is there -- the count never wraps -- the rest is
// refused (underflow) and the sums of the whole group are left alone.  Clamping, rather than refusing all n, makes the counters what a
// point-by-point removal gives, min(held, asked) per voxel, however the points are grouped and whichever workgroup comes first.
__device__ __forceinline__ long long find_and_take(unsigned long long* table, unsigned long long mask, unsigned long long key, unsigned n, unsigned* s_stat) {
    const unsigned long long first = mix64(key) & mask;
    unsigned probes = 0;
    const long long slot = find(table, mask, key, first, table[first * kFields], probes);
    if (slot < 0) {
        atomicAdd(&s_stat[kStDropped], n);
        return -1;
    }
    unsigned long long* cp = table + (unsigned long long)slot * kFields + 1;
    unsigned long long cur = __hip_atomic_load(cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned take;
    for (;;) {
        take = cur < n ? (unsigned)cur : n;
        if (take == 0) break;
        const unsigned long long seen = atomicCAS(cp, cur, cur - take);
        if (seen == cur) break;
        cur = seen;
    }
    if (take && cur == take) atomicAdd(&s_stat[kStNew], 1u);
    if (take) atomicAdd(&s_stat[kStAdded], take);
    if (take < n) {
        atomicAdd(&s_stat[kStUnderflow], n - take);
        return -1;
    }
    atomicAdd(&s_stat[kStUpdates], 1u);
    return slot;
}

template <int SRC, int MODE>
__global__ __launch_bounds__(kThreads) void k_vmap_insert(Params P, Source src, unsigned long long* __restrict__ table, unsigned long long mask,
                                                          unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_key[kLdsSlots];
    __shared__ unsigned long long s_sum[3][kLdsSlots];
    __shared__ unsigned s_cnt[kLdsSlots], s_rgb[3][kLdsSlots];
    __shared__ long long s_slot[kLdsSlots];
    __shared__ unsigned s_stat[kStWords];
    const int t = threadIdx.x;
    for (int h = t; h < kLdsSlots; h += kThreads) {
        s_key[h] = kEmpty;
        s_sum[0][h] = s_sum[1][h] = s_sum[2][h] = 0;
        s_cnt[h] = s_rgb[0][h] = s_rgb[1][h] = s_rgb[2][h] = 0;
    }
    if (t < kStWords) s_stat[t] = 0;

    float x[kPerThread], y[kPerThread], z[kPerThread];
    bool in[kPerThread];
    long long index[kPerThread];
    load_points<SRC>(src, x, y, z, in, index);
    // the colour of each point, by its index: in the cloud (SRC 1), or in the image's row, whose pointer is moved back by the row's first
    // index (SRC 0; the row step may be longer than 3 * cols)
    unsigned c[kPerThread][3];
    const uint8_t* crow = !src.rgb ? nullptr : SRC == 0 ? src.rgb + (size_t)blockIdx.y * src.rgb_step - 3 * (size_t)blockIdx.y * src.cols : src.rgb;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
#pragma unroll
        for (int q = 0; q < 3; ++q) c[k][q] = crow ? crow[3 * (size_t)index[k] + q] : 0u;
    }
    __syncthreads();

    unsigned tally = 0;      // this thread's points: valid | outside the box << 10 | out of range << 20 (a wave's sums stay below 1024)
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        unsigned long long key = 0;
        long long f[3] = {0, 0, 0};
        const int cls = in[k] ? classify(P, x[k], y[k], z[k], key, f) : 0;
        tally += (cls >= 1 ? 1u : 0u) + (cls == 1 ? 1u << 10 : 0u) + (cls == 2 ? 1u << 20 : 0u);
        if (cls != 3) continue;
        unsigned h = (unsigned)(mix64(key) >> 40) & (kLdsSlots - 1);      // (bits the global table's index does not use below 2^40 slots)
        bool merged = false;
        for (int p = 0; p < kLdsProbes && !merged; ++p) {
            unsigned long long k0 = __hip_atomic_load(&s_key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (k0 == kEmpty) {
                k0 = atomicCAS(&s_key[h], kEmpty, key);
                if (k0 == kEmpty) k0 = key;
            }
            if (k0 == key) {
                atomicAdd(&s_cnt[h], 1u);
#pragma unroll
                for (int q = 0; q < 3; ++q) atomicAdd(&s_sum[q][h], (unsigned long long)f[q]);
                if (src.rgb) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) atomicAdd(&s_rgb[q][h], c[k][q]);
                }
                merged = true;
            }
            h = (h + 1) & (kLdsSlots - 1);
        }
        if (!merged && MODE == kRemove) {      // (as below, one point)
            const long long slot = find_and_take(table, mask, key, 1u, s_stat);
            if (slot >= 0) {
                unsigned long long* rec = table + (unsigned long long)slot * kFields;
#pragma unroll
                for (int q = 0; q < 3; ++q) atomicAdd(rec + 2 + q, 0ull - (unsigned long long)f[q]);
                if (src.rgb) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) atomicAdd(rec + 5 + q, 0ull - (unsigned long long)c[k][q]);
                }
            }
        } else if (!merged) {       // the block's table is crowded around this key: the point goes to the map on its own
            bool claimed = false;
            const long long slot = find_or_claim(table, mask, key, claimed);
            if (MODE == kInsert && claimed) atomicAdd(&s_stat[kStNew], 1u);
            if (slot < 0) {
                atomicAdd(&s_stat[kStDropped], 1u);
            } else {
                unsigned long long* rec = table + (unsigned long long)slot * kFields;
                if (MODE == kInsert) atomicAdd(rec + 1, 1ull);
                else if (atomicAdd(rec + 1, 1ull) == 0) atomicAdd(&s_stat[kStNew], 1u);
#pragma unroll
                for (int q = 0; q < 3; ++q) atomicAdd(rec + 2 + q, (unsigned long long)f[q]);
                if (src.rgb) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) atomicAdd(rec + 5 + q, (unsigned long long)c[k][q]);
                }
                atomicAdd(&s_stat[kStAdded], 1u);
                atomicAdd(&s_stat[kStUpdates], 1u);
            }
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) tally += __shfl_xor(tally, off);
    if ((t & 63) == 0 && tally) {
        atomicAdd(&s_stat[kStValid], tally & 1023u);
        atomicAdd(&s_stat[kStBox], (tally >> 10) & 1023u);
        atomicAdd(&s_stat[kStRange], tally >> 20);
    }
    __syncthreads();

    // one lane per merged entry: its slot in the map
    for (int h = t; h < kLdsSlots; h += kThreads) {
        long long slot = -1;
        if (s_key[h] != kEmpty && MODE == kRemove) {
            slot = find_and_take(table, mask, s_key[h], s_cnt[h], s_stat);
        } else if (s_key[h] != kEmpty) {
            bool claimed = false;
            slot = find_or_claim(table, mask, s_key[h], claimed);
            if (MODE == kInsert && claimed) atomicAdd(&s_stat[kStNew], 1u);
            atomicAdd(&s_stat[slot < 0 ? kStDropped : kStAdded], s_cnt[h]);
            if (slot >= 0) atomicAdd(&s_stat[kStUpdates], 1u);
        }
        s_slot[h] = slot;
    }
    __syncthreads();
    // eight lanes per entry: lane q adds word q of the slot (word 0 is the key); empty entries are skipped.  Removal has taken the count
    // in the slot phase and adds the negatives of the six sums.
    for (int e = t >> 3; e < kLdsSlots; e += kThreads / 8) {
        const int q = t & 7;
        const long long slot = s_slot[e];
        if (slot < 0 || q == 0 || (MODE == kRemove && q == 1)) continue;
        const unsigned long long v = q == 1 ? (unsigned long long)s_cnt[e] : q <= 4 ? s_sum[q - 2][e] : (unsigned long long)s_rgb[q - 5][e];
        if (!v) continue;
        unsigned long long* word = table + (unsigned long long)slot * kFields + q;
        if (MODE == kRemove) atomicAdd(word, 0ull - v);
        else if (MODE == kInsertRevive && q == 1) {
            if (atomicAdd(word, v) == 0) atomicAdd(&s_stat[kStNew], 1u);
        } else atomicAdd(word, v);
    }
    if (MODE == kInsertRevive) __syncthreads();      // (its new voxels are counted in the phase above)
    if (t < kStWords && s_stat[t]) atomicAdd(stats + t, (unsigned long long)s_stat[t]);
}

__global__ __launch_bounds__(256) void k_vmap_clear(unsigned long long* __restrict__ table, unsigned long long n_words) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) table[i] = (i & (kFields - 1)) == 0 ? kEmpty : 0ull;
}

// any output may be null; records beyond max_out are counted, not written
__global__ __launch_bounds__(256) void k_vmap_extract(const unsigned long long* __restrict__ table, unsigned long long n_slots, long long max_out,
                                                      unsigned long long* __restrict__ counter, float* __restrict__ xyz, uint8_t* __restrict__ rgb3,
                                                      int32_t* __restrict__ count, int32_t* __restrict__ key3) {
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long* rec = table + (s < n_slots ? s : 0) * kFields;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(rec);      // key, count
    const unsigned long long key = kc.x;
    const bool occupied = s < n_slots && key != kEmpty && kc.y != 0;      // (count 0: a tombstone)
    const unsigned long long wave = __ballot(occupied);
    unsigned long long base = 0;
    if (lane == 0 && wave) base = atomicAdd(counter, (unsigned long long)__popcll(wave));      // one add per wave
    base = __shfl(base, 0);
    const unsigned long long o = base + (unsigned long long)__popcll(wave & ((1ull << lane) - 1ull));
    if (!occupied || (long long)o >= max_out) return;
    const unsigned long long n = kc.y;
    if (xyz) {
        const double den = (double)n * kFix;
#pragma unroll
        for (int k = 0; k < 3; ++k) xyz[3 * o + k] = (float)((double)(long long)rec[2 + k] / den);
    }
    if (rgb3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb3[3 * o + k] = (uint8_t)(rec[5 + k] / n);
    }
    if (count) count[o] = (int32_t)n;
    if (key3) unpack_key3(key, key3 + 3 * o);
}

}  // namespace vmap

namespace {

int vmap_fail(rgbd360_map* m, int code, const char* msg) {
    m->err = msg;
    return code;
}
// what every entry that writes a map says to a level of the pyramid (map_pyramid.h), before anything is touched
int vmap_refuse_level(rgbd360_map* m) {
    return m->parent ? vmap_fail(m, -1, "a level of a map pyramid is read-only: write its parent") : 0;
}
// the vote array (map_carve.h) goes: rgbd360_map_release_votes, and rgbd360_map_rehash, which moves every voxel to another slot
void vmap_drop_votes(rgbd360_map* m) {
    hipSetDevice(m->s->p.device);
    m->vt_votes.release();
    m->vt_have = m->vt_spent = false;
    m->vt_rays_n = m->vt_voted = 0;
}
// Two events around work on a stream (the rgbd360_map_time_* entries).  rc: the first failure, of the timer or of a body; once it is set
// nothing more is recorded or run.  The events go with the timer.
struct VmapTimer {
    rgbd360_map* m;
    hipStream_t stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // add()'s microseconds per slot
    VmapTimer(rgbd360_map* m_, hipStream_t stream_) : m(m_), stream(stream_) {
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            (void)hipGetLastError();
            rc = vmap_fail(m, -103, "hipEventCreate failed");
        }
    }
    VmapTimer(const VmapTimer&) = delete;
    VmapTimer& operator=(const VmapTimer&) = delete;
    ~VmapTimer() {
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
    }
    // out: microseconds per call of `count` calls of body() (0: fine) between the two events
    template <class Body>
    void timed(float& out, int count, Body&& body) {
        float ms = 0.f;
        if (rc != 0) return;
        if (hipEventRecord(e0, stream) != hipSuccess) rc = vmap_fail(m, -100, "hipEventRecord failed");
        for (int r = 0; r < count && rc == 0; ++r) rc = body();
        if (rc == 0 && (hipEventRecord(e1, stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
            rc = vmap_fail(m, -100, "timing the kernels failed");
        out = ms * 1000.f / (float)count;
    }
    // one call of body() between the events, its time added to slot `which`
    template <class Body>
    void add(int which, Body&& body) {
        float us = 0.f;
        timed(us, 1, body);
        sum[which] += (double)us;
    }
    // how a time_* entry ends: the first failure, or a launch error left behind, or avg_us[0 .. n) = the slots' sums over `reps`
    int finish(float* avg_us, int n, int reps) {
        if (rc) {
            (void)hipGetLastError();
            return rc;
        }
        HIPC(m, hipGetLastError());
        for (int k = 0; k < n; ++k) avg_us[k] = (float)(sum[k] / reps);
        return 0;
    }
};

// What a map call works on, as the caller handed it over: a sphere image or a cloud, in host memory or, on_device, in
// device memory.  Every entry builds one, vmap_check refuses a bad one before anything is touched, vmap_to_device makes it the kernels'.
struct MapInput {
    bool cloud = false;
    int on_device = 0;
    const uint8_t* rgb = nullptr;        // the image's 8UC3 rows / the cloud's n x 3 bytes; null: no colour
    size_t rgb_step = 0;
    const void* depth = nullptr;
    size_t depth_step = 0;
    int depth_type = 0, rows = 0, cols = 0, convention = 0;
    const float* xyz = nullptr;
    long long n = 0;
    const float* normal = nullptr;       // a cloud's normals, 3 n floats where the points are (generalized ICP alone, map_align_gicp.h); null: none
};
MapInput sphere_input(const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                      int on_device) {
    MapInput in;
    in.on_device = on_device;
    in.rgb = rgb, in.rgb_step = rgb_step, in.depth = depth, in.depth_step = depth_step;
    in.depth_type = depth_type, in.rows = rows, in.cols = cols, in.convention = convention;
    return in;
}
MapInput cloud_input(const float* xyz, const uint8_t* rgb3, long long n, int on_device) {
    MapInput in;
    in.cloud = true;
    in.on_device = on_device;
    in.rgb = rgb3, in.xyz = xyz, in.n = n;
    return in;
}
// ... and in device memory: the kernels' Source with which of its two forms it is
struct MapSource : vmap::Source {
    bool cloud = false;
};

// What every entry checks of its input before anything is launched, uploaded or allocated; have_pose: the call's pose(s) are there.
// 1: an empty image or no points (nothing to do; no points need no xyz and no pose)
int vmap_check(rgbd360_map* m, const MapInput& in, bool have_pose) {
    if (in.cloud) {
        if (in.n < 0 || in.n >= (1ll << 40)) return vmap_fail(m, -1, "bad point count");
        if (in.n > 0 && (!in.xyz || !have_pose)) return vmap_fail(m, -1, "xyz and pose must not be null");
        return in.n == 0 ? 1 : 0;
    }
    if (!in.depth || !have_pose) return vmap_fail(m, -1, "depth and pose must not be null");
    if (in.convention < 0 || in.convention > 2 || (in.depth_type != 0 && in.depth_type != 1)) return vmap_fail(m, -1, "bad convention or depth type");
    if (in.rows < 0 || in.cols < 0 || (long long)in.rows * in.cols >= (1ll << 30)) return vmap_fail(m, -1, "bad image size");
    if (in.rows == 0 || in.cols == 0) return 1;
    if (in.depth_step < (size_t)in.cols * (in.depth_type == 0 ? 2 : 4) || (in.rgb && in.rgb_step < (size_t)in.cols * 3))
        return vmap_fail(m, -1, "row step shorter than a row");
    return 0;
}
// ... and of a time_* entry's device image
int vmap_check_timed(rgbd360_map* m, const MapInput& in, const float* pose, int reps, const float* avg_us) {
    const int chk = vmap_check(m, in, pose != nullptr);
    if (chk < 0) return chk;
    return chk == 1 || reps < 1 || !avg_us ? vmap_fail(m, -1, "bad arguments") : 0;
}
// A checked, non-empty input as the kernels take it.  A host input goes up first, as packed copies on the map's stream (the colour only
// when there is one) -- the caller's memory is free once the stream has been waited for, which every entry does before it returns; a
// sphere image gets the context's angle tables of its geometry.
int vmap_to_device(rgbd360_map* m, const MapInput& in, MapSource& src) {
    hipSetDevice(m->s->p.device);
    const size_t n_rows = in.cloud ? 1 : (size_t)in.rows;
    const void* points = in.cloud ? (const void*)in.xyz : in.depth;
    const uint8_t* rgb = in.rgb;
    size_t prow = in.cloud ? (size_t)in.n * 3 * sizeof(float) : (size_t)in.cols * (in.depth_type == 0 ? 2 : 4), pstep = in.depth_step;
    size_t crow = in.cloud ? (size_t)in.n * 3 : (size_t)in.cols * 3, cstep = in.rgb_step;
    auto upload = [&](DevBuf<uint8_t>& buf, const void* host, size_t step, size_t row) {
        if (const hipError_t e = buf.ensure(row * n_rows)) return e;
        return in.cloud ? hipMemcpyAsync(buf, host, row, hipMemcpyHostToDevice, m->s->stream)
                        : hipMemcpy2DAsync(buf, row, host, step, row, n_rows, hipMemcpyHostToDevice, m->s->stream);
    };
    if (!in.on_device) {
        HIPC(m, upload(m->up_depth, points, pstep, prow));
        points = m->up_depth.get(), pstep = prow;
        if (rgb) {
            HIPC(m, upload(m->up_rgb, rgb, cstep, crow));
            rgb = m->up_rgb.get(), cstep = crow;
        }
    }
    if (in.cloud) {
        src = {{nullptr, 0, rgb, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, static_cast<const float*>(points), in.n}, true};
        return 0;
    }
    if (const int rc = sphere_tables_dev(m->s, in.rows, in.cols, in.convention)) {
        m->err = m->s->err;
        return rc;
    }
    const float* tab = m->s->f_tab;
    src = {{points, pstep, rgb, cstep, in.depth_type, in.rows, in.cols, in.convention, tab, tab + in.cols, tab + 2 * in.cols, tab + 2 * in.cols + in.rows, nullptr, 0},
           false};
    return 0;
}
// the launch grid of a source: a workgroup per tile of kTile points, of an image row or of the cloud
dim3 vmap_grid(const MapSource& src) {
    return src.cloud ? dim3((unsigned)((src.n + vmap::kTile - 1) / vmap::kTile)) : dim3((src.cols + vmap::kTile - 1) / vmap::kTile, src.rows);
}

int vmap_clear_dev(rgbd360_map* m) {
    const unsigned long long words = m->n_slots * vmap::kFields;
    hipLaunchKernelGGL(vmap::k_vmap_clear, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, m->s->stream, m->table, words);
    HIPC(m, hipGetLastError());
    m->n_voxels = 0;
    m->may_hold_tombstones = false;
    ++m->revision;
    return 0;
}
vmap::Params vmap_params(const rgbd360_map* m, const float pose[16]) {
    vmap::Params P;
    memcpy(P.pose, pose, sizeof(P.pose));
    for (int k = 0; k < 3; ++k) {
        P.lo[k] = m->lo[k];
        P.hi[k] = m->hi[k];
    }
    P.has_box = m->has_box ? 1 : 0;
    P.inv_leaf = m->inv_leaf;
    return P;
}
void vmap_fill_stats(const rgbd360_map* m, const unsigned long long* w, rgbd360_map_stats* st) {
    if (!st) return;
    st->n_valid = w ? (long long)w[vmap::kStValid] : 0;
    st->n_box_rejected = w ? (long long)w[vmap::kStBox] : 0;
    st->n_out_of_range = w ? (long long)w[vmap::kStRange] : 0;
    st->n_added = w ? (long long)w[vmap::kStAdded] : 0;
    st->n_dropped_full = w ? (long long)w[vmap::kStDropped] : 0;
    st->n_voxels = m->n_voxels;
}
// `words` counter words from d_stats into h_stats[at ..): enqueued on the stream (vmap_copy_stats), or there when the call returns
int vmap_copy_stats(rgbd360_map* m, int words, int at = 0) {
    HIPC(m, hipMemcpyAsync(m->h_stats + at, m->d_stats, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->s->stream));
    return 0;
}
int vmap_read_stats(rgbd360_map* m, int words, int at = 0) {
    if (const int rc = vmap_copy_stats(m, words, at)) return rc;
    HIPC(m, hipStreamSynchronize(m->s->stream));
    return 0;
}
// the insert kernel over `src` in `mode` (vmap::kInsert ..), enqueued on the stream; the statistics words are cleared in front of it.
// vmap_launch_insert is an insert as the map stands: revivals are counted once a removal has emptied a voxel.
int vmap_launch(rgbd360_map* m, const vmap::Params& P, const MapSource& src, int mode) {
    ++m->revision;
    HIPC(m, hipMemsetAsync(m->d_stats, 0, (mode == vmap::kRemove ? vmap::kStWords : vmap::kStInsertWords) * sizeof(unsigned long long), m->s->stream));
    const dim3 grid = vmap_grid(src);
    with_choice<0, 1>(src.cloud, [&](auto S) {
        with_int<vmap::kInsert, vmap::kInsertRevive>(mode, [&](auto M) {
            hipLaunchKernelGGL((vmap::k_vmap_insert<decltype(S)::value, decltype(M)::value>), grid, dim3(vmap::kThreads), 0, m->s->stream, P, src, m->table,
                               m->n_slots - 1, m->d_stats);
        });
    });
    HIPC(m, hipGetLastError());
    return 0;
}
int vmap_launch_insert(rgbd360_map* m, const vmap::Params& P, const MapSource& src) {
    return vmap_launch(m, P, src, m->may_hold_tombstones ? vmap::kInsertRevive : vmap::kInsert);
}
// how an insert ends once its counters `w` are on the host: the map's size brought up to date, the statistics, the status
int vmap_close_insert(rgbd360_map* m, const unsigned long long* w, rgbd360_map_stats* stats) {
    m->n_voxels += (long long)w[vmap::kStNew];
    m->last_updates = (long long)w[vmap::kStUpdates];
    vmap_fill_stats(m, w, stats);
    if (w[vmap::kStDropped]) {
        m->err = "the map is full: points of new voxels were dropped";
        return RGBD360_MAP_FULL;
    }
    return 0;
}
int vmap_finish_insert(rgbd360_map* m, rgbd360_map_stats* stats) {
    if (const int rc = vmap_read_stats(m, vmap::kStInsertWords)) return rc;
    return vmap_close_insert(m, m->h_stats, stats);
}
// an insert call: rgbd360_map_insert_sphere / _cloud
int vmap_insert(rgbd360_map* m, const MapInput& in, const float* pose, rgbd360_map_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;
    const int chk = vmap_check(m, in, pose != nullptr);
    if (chk < 0) return chk;
    vmap_fill_stats(m, nullptr, stats);
    if (chk == 1) return 0;
    MapSource src;
    if (const int rc = vmap_to_device(m, in, src)) return rc;
    if (const int rc = vmap_launch_insert(m, vmap_params(m, pose), src)) return rc;
    return vmap_finish_insert(m, stats);
}
// the extract kernel into device arrays (any may be null; records beyond max_out are counted, not written), enqueued behind the clear of
// its counter
int vmap_launch_extract(rgbd360_map* m, long long max_out, float* xyz, uint8_t* rgb3, int32_t* count, int32_t* key3) {
    unsigned long long* counter = m->d_stats + vmap::kStExtract;
    HIPC(m, hipMemsetAsync(counter, 0, sizeof(unsigned long long), m->s->stream));
    hipLaunchKernelGGL(vmap::k_vmap_extract, dim3((unsigned)((m->n_slots + 255) / 256)), dim3(256), 0, m->s->stream, m->table, m->n_slots, max_out, counter,
                       xyz, rgb3, count, key3);
    HIPC(m, hipGetLastError());
    return 0;
}
// ... complete when the call returns
int vmap_extract_dev(rgbd360_map* m, long long max_out, float* xyz, uint8_t* rgb3, int32_t* count, int32_t* key3) {
    if (const int rc = vmap_launch_extract(m, max_out, xyz, rgb3, count, key3)) return rc;
    HIPC(m, hipStreamSynchronize(m->s->stream));
    return 0;
}
// the scan alone (xyz only, into x_xyz), as the time_* entries measure it
int vmap_launch_extract_scan(rgbd360_map* m) { return vmap_launch_extract(m, m->n_voxels, m->x_xyz, nullptr, nullptr, nullptr); }
}  // namespace

extern "C" int rgbd360_map_create(rgbd360_ctx* ctx_, float leaf, long long capacity_voxels, rgbd360_map** out) {
    if (out) *out = nullptr;
    if (!ctx_ || !out) return -1;
    F360_ENTER(ctx_);
    if (!(leaf >= 0.004f) || !std::isfinite(leaf) || capacity_voxels < 1 || capacity_voxels > (1ll << 30))
        return fail(ctx, -1, "rgbd360_map_create: leaf must be >= 0.004 m and capacity in 1 .. 2^30 voxels");
    hipSetDevice(ctx->p.device);
    rgbd360_map* m = new rgbd360_map();
    m->ctx = ctx_;
    m->s = ctx;
    m->leaf = leaf;
    m->inv_leaf = 1.0f / leaf;
    m->n_slots = 1;
    while (m->n_slots < (unsigned long long)capacity_voxels) m->n_slots <<= 1;
    if (m->table.ensure(m->n_slots * vmap::kFields) != hipSuccess || m->d_stats.ensure(vmap::kStWords) != hipSuccess ||
        m->h_stats.ensure(2 * vmap::kStWords) != hipSuccess) {      // (twice: a move keeps the counters of both its launches)
        (void)hipGetLastError();
        delete m;
        return fail(ctx, -103, "rgbd360_map_create: out of memory");
    }
    if (vmap_clear_dev(m) != 0 || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        ctx->err = "rgbd360_map_create: " + m->err;
        delete m;
        return -103;
    }
    *out = m;
    return 0;
}
extern "C" void rgbd360_map_destroy(rgbd360_map* m) {
    if (!m || m->parent) return;      // (a level goes with its parent)
    hipSetDevice(m->s->p.device);
    hipStreamSynchronize(m->s->stream);
    delete m;
}
extern "C" const char* rgbd360_map_last_error(rgbd360_map* m) { return m ? m->err.c_str() : "null map"; }
extern "C" size_t rgbd360_map_bytes(const rgbd360_map* m) { return m ? (size_t)m->n_slots * vmap::kFields * sizeof(unsigned long long) : 0; }
extern "C" int rgbd360_map_set_box(rgbd360_map* m, const float lo[3], const float hi[3]) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;
    if (!lo != !hi) return vmap_fail(m, -1, "both limits or none");
    m->has_box = lo != nullptr;
    for (int k = 0; k < 3 && lo; ++k) {
        m->lo[k] = lo[k];
        m->hi[k] = hi[k];
    }
    return 0;
}

extern "C" int rgbd360_map_insert_sphere(rgbd360_map* m, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type,
                                         int rows, int cols, int convention, const float pose[16], int on_device, rgbd360_map_stats* stats) {
    return vmap_insert(m, sphere_input(rgb, rgb_step, depth, depth_step, depth_type, rows, cols, convention, on_device), pose, stats);
}
extern "C" int rgbd360_map_insert_cloud(rgbd360_map* m, const float* xyz, const uint8_t* rgb3, long long n, const float pose[16], int on_device,
                                        rgbd360_map_stats* stats) {
    return vmap_insert(m, cloud_input(xyz, rgb3, n, on_device), pose, stats);
}

extern "C" long long rgbd360_map_size(rgbd360_map* m) { return m ? m->n_voxels : -1; }
extern "C" int rgbd360_map_clear(rgbd360_map* m) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;
    hipSetDevice(m->s->p.device);
    if (const int rc = vmap_clear_dev(m)) return rc;
    HIPC(m, hipStreamSynchronize(m->s->stream));
    return 0;
}

extern "C" long long rgbd360_map_extract_dev(rgbd360_map* m, long long max_out, float* xyz, uint8_t* rgb3, int32_t* count, int32_t* key3) {
    if (!m) return -1;
    m->err.clear();
    if (max_out < 0) return vmap_fail(m, -1, "max_out must not be negative");
    hipSetDevice(m->s->p.device);
    if (m->n_voxels == 0 || max_out == 0) return m->n_voxels;
    if (const int rc = vmap_extract_dev(m, max_out, xyz, rgb3, count, key3)) return rc;
    return m->n_voxels;
}

extern "C" long long rgbd360_map_extract(rgbd360_map* m, long long max_out, float* xyz, uint8_t* rgb3, int32_t* count, int32_t* key3) {
    if (!m) return -1;
    m->err.clear();
    if (max_out < 0) return vmap_fail(m, -1, "max_out must not be negative");
    const size_t n = (size_t)m->n_voxels, n_out = std::min(n, (size_t)max_out);
    if (n_out == 0) return m->n_voxels;
    hipSetDevice(m->s->p.device);
    // the whole map unsorted (the first max_out of the SORTED map are wanted), then the order of the keys on the host
    HIPC(m, m->x_xyz.ensure(3 * n));
    HIPC(m, m->x_rgb.ensure(3 * n));
    HIPC(m, m->x_count.ensure(n));
    HIPC(m, m->x_key.ensure(3 * n));
    if (const int rc = vmap_extract_dev(m, (long long)n, m->x_xyz, m->x_rgb, m->x_count, m->x_key)) return rc;
    std::vector<float> h_xyz(3 * n);
    std::vector<uint8_t> h_rgb(3 * n);
    std::vector<int32_t> h_count(n), h_key(3 * n);
    HIPC(m, hipMemcpy(h_key.data(), m->x_key, 3 * n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (xyz) HIPC(m, hipMemcpy(h_xyz.data(), m->x_xyz, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    if (rgb3) HIPC(m, hipMemcpy(h_rgb.data(), m->x_rgb, 3 * n, hipMemcpyDeviceToHost));
    if (count) HIPC(m, hipMemcpy(h_count.data(), m->x_count, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<size_t> order(n);
    for (size_t k = 0; k < n; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {      // (i_z, i_y, i_x) ascending: PCL's idx = i0 + i1 dx + i2 dx dy
        for (int q = 2; q >= 0; --q)
            if (h_key[3 * a + q] != h_key[3 * b + q]) return h_key[3 * a + q] < h_key[3 * b + q];
        return false;
    });
    for (size_t o = 0; o < n_out; ++o) {
        const size_t k = order[o];
        for (int q = 0; q < 3; ++q) {
            if (xyz) xyz[3 * o + q] = h_xyz[3 * k + q];
            if (rgb3) rgb3[3 * o + q] = h_rgb[3 * k + q];
            if (key3) key3[3 * o + q] = h_key[3 * k + q];
        }
        if (count) count[o] = h_count[k];
    }
    return m->n_voxels;
}

// the seam to map_render.h (map_table.h)
void rgbd360_map_view(const rgbd360_map* m, vmap::RenderView* v) {
    *v = {m->s->p.device, m->s->stream, m->table.get(), m->n_slots, m->leaf, m->n_voxels, m->r_dist.get(), m->r_key.get(), m->r_stats.get(), m->r_hstats.get(),
          m->r_stage.get()};
}
int rgbd360_map_render_view(rgbd360_map* m, size_t n_pixels, bool stage, vmap::RenderView* v) {
    hipSetDevice(m->s->p.device);
    HIPC(m, m->r_dist.ensure(n_pixels));
    HIPC(m, m->r_key.ensure(n_pixels));
    HIPC(m, m->r_stats.ensure(vmap::kRnWords));
    HIPC(m, m->r_hstats.ensure(vmap::kRnWords));
    if (stage) HIPC(m, m->r_stage.ensure(n_pixels * 23));
    rgbd360_map_view(m, v);
    return 0;
}
int rgbd360_map_set_error(rgbd360_map* m, int code, const char* msg) { return vmap_fail(m, code, msg); }
int rgbd360_map_time_extract_scan(rgbd360_map* m, int reps, float* avg_us) {
    hipSetDevice(m->s->p.device);
    if (m->x_xyz.ensure(3 * (size_t)m->n_voxels + 3) != hipSuccess) return vmap_fail(m, -103, "out of memory");
    VmapTimer timer(m, m->s->stream);
    timer.timed(*avg_us, reps, [&] { return vmap_launch_extract_scan(m); });       // (with the clear of its counter, as in every extract call)
    return timer.finish(avg_us, 0, reps);
}

// measurement (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_time_kernels(rgbd360_map* m, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev, size_t depth_step, int depth_type,
                                        int rows, int cols, int convention, const float pose[16], int reps, float avg_us[5],
                                        long long* global_updates) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;      // (it clears and fills the map)
    const MapInput in = sphere_input(rgb_dev, rgb_step, depth_dev, depth_step, depth_type, rows, cols, convention, 1);
    if (const int rc = vmap_check_timed(m, in, pose, reps, avg_us)) return rc;
    F360State* ctx = m->s;
    hipSetDevice(ctx->p.device);
    if (const int rc = f360_begin(ctx, rows, cols, 1)) {
        m->err = ctx->err;
        return rc;
    }
    MapSource src;
    if (const int rc = vmap_to_device(m, in, src)) return rc;
    const vmap::Params P = vmap_params(m, pose);
    const size_t drow = (size_t)cols * (depth_type == 0 ? 2 : 4), crow = rgb_dev ? (size_t)cols * 3 : 0;
    HIPC(m, m->up_depth.ensure(drow * rows));
    if (crow) HIPC(m, m->up_rgb.ensure(crow * rows));
    VmapTimer timer(m, ctx->stream);         // made last
    int& rc = timer.rc;
    rgbd360_map_stats st;
    for (int r = 0; r < reps && rc == 0; ++r) {
        if ((rc = vmap_clear_dev(m)) != 0) break;
        // (the statistics' clear is a 64-byte memset in front of the kernel, inside the window: it is part of every insert)
        timer.add(0, [&] { return vmap_launch_insert(m, P, src); });       // an empty map
        if (rc == 0) rc = std::min(vmap_finish_insert(m, &st), 0);
        if (global_updates) *global_updates = m->last_updates;
        timer.add(1, [&] { return vmap_launch_insert(m, P, src); });       // the map holds the frame's voxels: odometry's steady state
        if (rc == 0) rc = std::min(vmap_finish_insert(m, &st), 0);
        if (rc == 0 && m->x_xyz.ensure(3 * (size_t)m->n_voxels + 3) != hipSuccess) rc = vmap_fail(m, -103, "out of memory");
        timer.add(2, [&] { return vmap_launch_extract_scan(m); });         // (with the clear of its counter, as in every extract call)
        timer.add(3, [&] {
            hipLaunchKernelGGL(r360::k_sphere_cloud_s4, dim3((cols + 1023) / 1024, rows), dim3(256), 0, ctx->stream, depth_dev, depth_step, depth_type, rows, cols,
                               convention, src.sin_theta, src.cos_theta, src.sin_phi, src.cos_phi, ctx->f_xyz);
            return 0;
        });
        timer.add(4, [&] {       // the input bytes once through the device: the copy rate of the floor
            hipMemcpy2DAsync(m->up_depth, drow, depth_dev, depth_step, drow, rows, hipMemcpyDeviceToDevice, ctx->stream);
            if (crow) hipMemcpy2DAsync(m->up_rgb, crow, rgb_dev, rgb_step, crow, rows, hipMemcpyDeviceToDevice, ctx->stream);
            return 0;
        });
    }
    return timer.finish(avg_us, 5, reps);
}
