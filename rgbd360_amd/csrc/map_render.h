// map_render.h -- the resident voxel map (voxel_map.h) rendered as a spherical RGB-D frame at a pose: a z-buffered splat of the table
// into the full-sphere panorama of the dense alignment.  It stands in for the reference's view of its global map
//   viewer.globalMap in a PCL window                      OdometryRGBD360.cpp:242-268
// and turns the map into what the dense alignment takes as its target (the keyframe target of OdometryKeyFrame360.cpp: here the model
// is everything inserted so far): depth and rgb go straight into rgbd360_set_target with depth_type 1.
// Part of the alignment translation unit (rgbd360_api.hip), because the projection IS the dense alignment's warp front end
// (warp_pixel_rc, photo_icp_kernels.h, in the device arithmetic); the map lives in the other unit and is reached through map_table.h.
//
// Definition (include/rgbd360_hip.h, "the map rendered as a spherical frame"; tests/map_render_reference.py restates it):
//   1 inverse pose  on the host: Rinv = R^T, tinv_k = -(R_0k t_x + R_1k t_y + R_2k t_z) in double, left to right, rounded to float32.
//   2 voxel         every occupied slot with count >= min_count; centroid and colour are the read-out's expressions.
//   3 projection    warp_pixel_rc with lv.libm == 0 at the inverse pose, the centroid as the source point: (r', c'), d2, visibility;
//                   dist = sqrt_rn(d2).  Skipped (n_near) when not visible, dist not finite or dist < near.
//   4 footprint     h = min(max_half, (int)(foot * rcp_rn(dist))), foot = (splat * leaf) * angle_res_inv; rows r' - h .. r' + h clipped,
//                   columns c' - h .. c' + h modulo cols, every column once when 2 h + 1 >= cols.
//   5 visibility    the smallest dist wins a pixel (positive floats compare as their bits); on equal bits the smaller packed key.
//   6 outputs       depth, rgb, count, key3 of the winner, zeros in holes; exact integer statistics.
//
// Three launches on the map's stream, the kernel boundaries the only synchronisation (warp_images.h's pattern; integer atomics only, no
// tickets, no fences), behind the clears of the two planes:
//   k_vmap_render_depth     one lane per slot: {key, count} as one 16-byte load, the six sums (three 16-byte loads) only where the slot
//                           takes part -- a lane's four loads cover its 64-byte slot, the access shape of k_vmap_extract.  Steps 2-4,
//                           then per covered pixel a uint32 atomicMin of dist's bits into the distance plane (cleared to 0xFFFFFFFF).
//   k_vmap_render_key       the same scan and projection (same bits); where the plane holds this voxel's bits, a 64-bit atomicMin of its
//                           key into the key plane (cleared to ~0).
//   k_vmap_render_resolve   one lane per pixel: the winning key looked up read-only (vmap::find, the alignment's lookup), the four
//                           output planes stored.
// Integer minima do not depend on the order of arrival: the image is the same from run to run and whatever the order of insertion or
// the table's capacity.  The table is never written.
// Two forms of the footprint loop (FORM): 0, every lane walks its own voxel's footprint; 1, the wave walks the footprints of its voxels
// one after the other, 64 pixels at a time (consecutive lanes, consecutive pixels of a footprint row).  kRenderForm is the one the
// entries use; tools/map_render_perf.py times both.
#pragma once
#include "map_table.h"
#include "photo_icp_kernels.h"

namespace vmap {

constexpr int kRenderThreads = 256;
constexpr int kRenderMaxHalf = 64;
constexpr int kRenderForm = 0;

struct RenderArgs {
    const unsigned long long* table;
    unsigned long long n_slots;
    unsigned long long min_count;
    float near, foot;
    int max_half;
    uint32_t* plane_dist;
    unsigned long long* plane_key;
    unsigned long long* stats;
};
struct RenderOut {        // any pointer may be null
    float* depth;
    uint8_t* rgb;
    int32_t* count;
    int32_t* key3;
};

// one covered pixel: the depth pass, or the key pass
template <bool KEY>
__device__ __forceinline__ void render_pixel(const RenderArgs& A, int p, uint32_t bits, unsigned long long key) {
    if (KEY) {
        if (A.plane_dist[p] == bits) atomicMin(&A.plane_key[p], key);
    } else {
        atomicMin(&A.plane_dist[p], bits);
    }
}

// steps 2-5 over the table; KEY 0: the depth pass (it also counts), 1: the key pass
template <bool KEY, int FORM>
__device__ __forceinline__ void render_scan(const r360::LevelDev& lv, const r360::Pose16& inv_pose, const RenderArgs& A) {
    const unsigned long long s = (unsigned long long)blockIdx.x * kRenderThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const r360::PoseRT T = r360::load_pose(inv_pose.v);
    const ulonglong2* rec = reinterpret_cast<const ulonglong2*>(A.table + (s < A.n_slots ? s : 0) * kFields);
    const ulonglong2 kc = rec[0];                        // key, count
    const bool occupied = s < A.n_slots && kc.x != kEmpty && kc.y != 0;      // (count 0: a tombstone of a removal, absent)
    const bool takes = occupied && kc.y >= A.min_count;
    float c[3] = {0.f, 0.f, 0.f};
    if (takes) {
        const ulonglong2 s01 = rec[1], s2r = rec[2];     // Sx, Sy | Sz, Sr
        const double den = (double)kc.y * kFix;
        c[0] = (float)((double)(long long)s01.x / den);
        c[1] = (float)((double)(long long)s01.y / den);
        c[2] = (float)((double)(long long)s2r.x / den);
    }
    // (no branch around the warp: its predicates are whole-wave lane masks; a lane without a voxel warps the origin and drops out below)
    float X, Y, Z, rho2, d2, inv_rho;
    int tr, tc;
    unsigned long long vis_mask;
    const r360::WarpConsts wc = {T.tx, T.ty, T.tz, lv.half_nRows, lv.pi_k};
    r360::warp_pixel_rc(T, wc, c[0], c[1], c[2], lv, X, Y, Z, rho2, d2, tr, tc, vis_mask, inv_rho);
    const bool vis = __builtin_amdgcn_inverse_ballot_w64(vis_mask);
    const float dist = r360::sqrt_rn(d2);
    const bool on = takes && vis && isfinite(dist) && dist >= A.near;
    // h = min(max_half, (int)q) wherever the cast is defined; q not a number (0 x inf) or beyond the int range never reaches the cast
    const float q = A.foot * r360::rcp_rn(dist);
    const int h = q >= (float)A.max_half ? A.max_half : (q > 0.f ? (int)q : 0);
    const uint32_t bits = __builtin_bit_cast(uint32_t, dist);
    const int r0 = max(tr - h, 0), r1 = min(tr + h, lv.rows - 1);
    const bool all_cols = 2 * h + 1 >= lv.cols;
    const int w = all_cols ? lv.cols : 2 * h + 1;
    int c0 = all_cols ? 0 : tc - h;
    if (c0 < 0) c0 += lv.cols;
    const int area = on ? (r1 - r0 + 1) * w : 0;

    if (!KEY) {
        const unsigned long long b_occ = __ballot(occupied), b_low = __ballot(occupied && !takes), b_near = __ballot(takes && !on), b_on = __ballot(on);
        unsigned n_atomics = (unsigned)area;
#pragma unroll
        for (int off = 32; off; off >>= 1) n_atomics += __shfl_xor(n_atomics, off);
        if (lane == 0 && b_occ) {        // one add per wave and counter
            atomicAdd(A.stats + kRnVoxels, (unsigned long long)__popcll(b_occ));
            if (b_low) atomicAdd(A.stats + kRnBelowMin, (unsigned long long)__popcll(b_low));
            if (b_near) atomicAdd(A.stats + kRnNear, (unsigned long long)__popcll(b_near));
            if (b_on) atomicAdd(A.stats + kRnSplatted, (unsigned long long)__popcll(b_on));
            if (n_atomics) atomicAdd(A.stats + kRnAtomics, (unsigned long long)n_atomics);
        }
    }

    if (FORM == 0) {
        if (!on) return;
        for (int r = r0; r <= r1; ++r) {
            const int row = r * lv.cols;
            for (int j = 0; j < w; ++j) {
                int cc = c0 + j;
                if (cc >= lv.cols) cc -= lv.cols;
                render_pixel<KEY>(A, row + cc, bits, kc.x);
            }
        }
    } else {
        unsigned long long todo = __ballot(on);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int v_r0 = __shfl(r0, src), v_w = __shfl(w, src), v_c0 = __shfl(c0, src), v_area = __shfl(area, src);
            const uint32_t v_bits = __shfl(bits, src);
            const unsigned long long v_key = __shfl(kc.x, src);
            for (int i = lane; i < v_area; i += 64) {
                int dr, j;
                r360::divmod24(i, v_w, dr, j);
                int cc = v_c0 + j;
                if (cc >= lv.cols) cc -= lv.cols;
                render_pixel<KEY>(A, (v_r0 + dr) * lv.cols + cc, v_bits, v_key);
            }
        }
    }
}

template <int FORM>
__global__ __launch_bounds__(kRenderThreads) void k_vmap_render_depth(r360::LevelDev lv, r360::Pose16 inv_pose, RenderArgs A) {
    render_scan<false, FORM>(lv, inv_pose, A);
}
template <int FORM>
__global__ __launch_bounds__(kRenderThreads) void k_vmap_render_key(r360::LevelDev lv, r360::Pose16 inv_pose, RenderArgs A) {
    render_scan<true, FORM>(lv, inv_pose, A);
}

__global__ __launch_bounds__(kRenderThreads) void k_vmap_render_resolve(RenderArgs A, int n, RenderOut out) {
    const int p = blockIdx.x * kRenderThreads + threadIdx.x;
    const int pc = min(p, n - 1);
    const unsigned long long key = A.plane_key[pc];
    bool hit = p < n && key != kEmpty;
    unsigned long long cnt = 0, col[3] = {0, 0, 0};
    if (hit) {
        const unsigned long long mask = A.n_slots - 1, first = mix64(key) & mask;
        unsigned probes = 0;
        const long long slot = find(A.table, mask, key, first, A.table[first * kFields], probes);
        hit = slot >= 0;
        if (hit) {
            const unsigned long long* rec = A.table + (unsigned long long)slot * kFields;
            cnt = rec[1];
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = rec[5 + k] / (cnt ? cnt : 1);
        }
    }
    const unsigned long long covered = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && covered) atomicAdd(A.stats + kRnPixels, (unsigned long long)__popcll(covered));
    if (p >= n) return;
    if (out.depth) out.depth[p] = hit ? __builtin_bit_cast(float, A.plane_dist[p]) : 0.f;
    if (out.rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out.rgb[3 * (size_t)p + k] = (uint8_t)col[k];
    }
    if (out.count) out.count[p] = (int32_t)cnt;
    if (out.key3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out.key3[3 * (size_t)p + k] = hit ? (int32_t)((key >> (21 * k)) & 0x1fffffull) - kBias : 0;
    }
}

}  // namespace vmap

namespace {

#define RENDER_HIPC(m, expr)                                                              \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return rgbd360_map_set_error(m, -(int)e_ - 1000, hipGetErrorString(e_)); \
    } while (0)

struct RenderJob {
    int rows = 0, cols = 0, n = 0;
    rgbd360_map_render_params p;
    LevelDev lv;
    Pose16 inv;
    float foot = 0.f;
};

// what a render call checks before anything is launched or allocated; 1: nothing to render (rows cols == 0)
int render_check(rgbd360_map* m, const vmap::RenderView& v, int rows, int cols, const float* pose, const rgbd360_map_render_params* params, RenderJob& job) {
    if (!pose) return rgbd360_map_set_error(m, -1, "pose must not be null");
    if (params) job.p = *params;
    else rgbd360_map_default_render_params(m, &job.p);
    const rgbd360_map_render_params& p = job.p;
    if (p.min_count < 1) return rgbd360_map_set_error(m, -1, "min_count must be at least 1");
    if (p.max_half < 0 || p.max_half > vmap::kRenderMaxHalf) return rgbd360_map_set_error(m, -1, "max_half must lie in 0 .. 64");
    if (!(p.splat >= 0.f) || !std::isfinite(p.splat)) return rgbd360_map_set_error(m, -1, "splat must be finite and not negative");
    if (!(p.near >= 0.f) || !std::isfinite(p.near)) return rgbd360_map_set_error(m, -1, "near must be finite and not negative");
    if (rows < 0 || cols < 0) return rgbd360_map_set_error(m, -1, "bad image size");
    job.rows = rows;
    job.cols = cols;
    if (rows == 0 || cols == 0) return 1;
    rgbd360_params one_level;
    rgbd360_default_params(&one_level);
    one_level.n_pyr = 1;
    if (const char* why = check_image_size(one_level, rows, cols)) return rgbd360_map_set_error(m, -1, why);
    const LevelGeom g = level_geom(rows, cols, 1);
    job.n = g.n;
    job.lv = LevelDev{};
    fill_level_dev(job.lv, g);
    // step 1: the inverse of a rotation and a translation (R is taken to be a rotation; this is not checked)
    memset(job.inv.v, 0, sizeof(job.inv.v));
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) job.inv.v[r + 4 * c] = pose[c + 4 * r];
    for (int k = 0; k < 3; ++k) {
        double s = (double)pose[4 * k] * (double)pose[12];
        s += (double)pose[1 + 4 * k] * (double)pose[13];
        s += (double)pose[2 + 4 * k] * (double)pose[14];
        job.inv.v[12 + k] = (float)-s;
    }
    job.inv.v[15] = 1.f;
    const float sl = p.splat * v.leaf;
    job.foot = sl * g.angle_res_inv;
    return 0;
}

vmap::RenderArgs render_args(const vmap::RenderView& v, const RenderJob& job) {
    return vmap::RenderArgs{v.table, v.n_slots, (unsigned long long)job.p.min_count, job.p.near, job.foot, job.p.max_half, v.plane_dist, v.plane_key, v.stats};
}
// which: 0 the depth pass, 1 the key pass, 2 the resolve pass
template <int FORM>
void render_launch_one(const vmap::RenderView& v, const RenderJob& job, int which, const vmap::RenderOut& out) {
    const vmap::RenderArgs A = render_args(v, job);
    const dim3 scan((unsigned)((v.n_slots + vmap::kRenderThreads - 1) / vmap::kRenderThreads)), block(vmap::kRenderThreads);
    if (which == 0) hipLaunchKernelGGL(vmap::k_vmap_render_depth<FORM>, scan, block, 0, v.stream, job.lv, job.inv, A);
    if (which == 1) hipLaunchKernelGGL(vmap::k_vmap_render_key<FORM>, scan, block, 0, v.stream, job.lv, job.inv, A);
    if (which == 2) hipLaunchKernelGGL(vmap::k_vmap_render_resolve, dim3((job.n + vmap::kRenderThreads - 1) / vmap::kRenderThreads), block, 0, v.stream, A, job.n, out);
}
// the clears and the three passes, enqueued on the map's stream; `out`: device memory
template <int FORM>
int render_enqueue(rgbd360_map* m, const vmap::RenderView& v, const RenderJob& job, const vmap::RenderOut& out) {
    RENDER_HIPC(m, hipMemsetAsync(v.plane_dist, 0xff, (size_t)job.n * sizeof(uint32_t), v.stream));
    RENDER_HIPC(m, hipMemsetAsync(v.plane_key, 0xff, (size_t)job.n * sizeof(unsigned long long), v.stream));
    RENDER_HIPC(m, hipMemsetAsync(v.stats, 0, vmap::kRnWords * sizeof(unsigned long long), v.stream));
    for (int which = 0; which < 3; ++which) render_launch_one<FORM>(v, job, which, out);
    RENDER_HIPC(m, hipGetLastError());
    return 0;
}
void render_fill_stats(const unsigned long long* w, rgbd360_map_render_stats* st) {
    if (!st) return;
    st->n_voxels = w ? (long long)w[vmap::kRnVoxels] : 0;
    st->n_below_min_count = w ? (long long)w[vmap::kRnBelowMin] : 0;
    st->n_near = w ? (long long)w[vmap::kRnNear] : 0;
    st->n_splatted = w ? (long long)w[vmap::kRnSplatted] : 0;
    st->n_pixels_covered = w ? (long long)w[vmap::kRnPixels] : 0;
}

}  // namespace

extern "C" void rgbd360_map_default_render_params(const rgbd360_map* m, rgbd360_map_render_params* p) {
    if (!p) return;
    float leaf = 0.05f;
    if (m) {
        vmap::RenderView v;
        rgbd360_map_view(m, &v);
        leaf = v.leaf;
    }
    p->min_count = 1;
    p->near = leaf;
    p->splat = 1.0f;
    p->max_half = 8;
}

extern "C" int rgbd360_map_render_sphere(rgbd360_map* m, int rows, int cols, const float pose[16], const rgbd360_map_render_params* params, float* depth,
                                         uint8_t* rgb, int32_t* count, int32_t* key3, rgbd360_map_render_stats* stats) {
    if (!m) return -1;
    rgbd360_map_set_error(m, 0, "");
    vmap::RenderView v;
    rgbd360_map_view(m, &v);
    RenderJob job;
    const int chk = render_check(m, v, rows, cols, pose, params, job);
    if (chk < 0) return chk;
    render_fill_stats(nullptr, stats);
    if (chk == 1) return 0;
    const size_t n = (size_t)job.n;
    if (v.n_voxels == 0) {       // nothing to splat: no launch
        if (depth) memset(depth, 0, n * sizeof(float));
        if (rgb) memset(rgb, 0, n * 3);
        if (count) memset(count, 0, n * sizeof(int32_t));
        if (key3) memset(key3, 0, n * 3 * sizeof(int32_t));
        return 0;
    }
    if (const int rc = rgbd360_map_render_view(m, n, true, &v)) return rc;
    // the staging: depth, count, key3, rgb (4-byte planes first)
    const vmap::RenderOut dev = {depth ? reinterpret_cast<float*>(v.stage) : nullptr, rgb ? v.stage + 20 * n : nullptr,
                                 count ? reinterpret_cast<int32_t*>(v.stage + 4 * n) : nullptr, key3 ? reinterpret_cast<int32_t*>(v.stage + 8 * n) : nullptr};
    if (const int rc = render_enqueue<vmap::kRenderForm>(m, v, job, dev)) return rc;
    if (depth) RENDER_HIPC(m, hipMemcpyAsync(depth, dev.depth, n * sizeof(float), hipMemcpyDeviceToHost, v.stream));
    if (rgb) RENDER_HIPC(m, hipMemcpyAsync(rgb, dev.rgb, n * 3, hipMemcpyDeviceToHost, v.stream));
    if (count) RENDER_HIPC(m, hipMemcpyAsync(count, dev.count, n * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
    if (key3) RENDER_HIPC(m, hipMemcpyAsync(key3, dev.key3, n * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
    RENDER_HIPC(m, hipMemcpyAsync(v.stats_host, v.stats, vmap::kRnWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, v.stream));
    RENDER_HIPC(m, hipStreamSynchronize(v.stream));
    render_fill_stats(v.stats_host, stats);
    return 0;
}

extern "C" int rgbd360_map_render_sphere_dev(rgbd360_map* m, int rows, int cols, const float pose[16], const rgbd360_map_render_params* params,
                                             float* depth_dev, uint8_t* rgb_dev, int32_t* count_dev, int32_t* key3_dev, rgbd360_map_render_stats* stats_dev) {
    if (!m) return -1;
    rgbd360_map_set_error(m, 0, "");
    vmap::RenderView v;
    rgbd360_map_view(m, &v);
    RenderJob job;
    const int chk = render_check(m, v, rows, cols, pose, params, job);
    if (chk < 0) return chk;
    hipSetDevice(v.device);
    if (chk == 1 || v.n_voxels == 0) {       // nothing to splat: the outputs are cleared on the stream, no kernel
        const size_t n = chk == 1 ? 0 : (size_t)job.n;
        if (depth_dev && n) RENDER_HIPC(m, hipMemsetAsync(depth_dev, 0, n * sizeof(float), v.stream));
        if (rgb_dev && n) RENDER_HIPC(m, hipMemsetAsync(rgb_dev, 0, n * 3, v.stream));
        if (count_dev && n) RENDER_HIPC(m, hipMemsetAsync(count_dev, 0, n * sizeof(int32_t), v.stream));
        if (key3_dev && n) RENDER_HIPC(m, hipMemsetAsync(key3_dev, 0, n * 3 * sizeof(int32_t), v.stream));
        if (stats_dev) RENDER_HIPC(m, hipMemsetAsync(stats_dev, 0, sizeof(rgbd360_map_render_stats), v.stream));
        return 0;
    }
    if (const int rc = rgbd360_map_render_view(m, (size_t)job.n, false, &v)) return rc;
    if (const int rc = render_enqueue<vmap::kRenderForm>(m, v, job, vmap::RenderOut{depth_dev, rgb_dev, count_dev, key3_dev})) return rc;
    static_assert(sizeof(rgbd360_map_render_stats) == 5 * sizeof(unsigned long long), "the statistics are the first five counters");
    if (stats_dev) RENDER_HIPC(m, hipMemcpyAsync(stats_dev, v.stats, sizeof(rgbd360_map_render_stats), hipMemcpyDeviceToDevice, v.stream));
    return 0;
}

// measurement (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_time_render(rgbd360_map* m, int rows, int cols, const float pose[16], const rgbd360_map_render_params* params, int form, int reps,
                                       float avg_us[5], rgbd360_map_render_stats* stats, long long* atomics) {
    if (!m) return -1;
    rgbd360_map_set_error(m, 0, "");
    vmap::RenderView v;
    rgbd360_map_view(m, &v);
    RenderJob job;
    const int chk = render_check(m, v, rows, cols, pose, params, job);
    if (chk < 0) return chk;
    if (chk == 1 || v.n_voxels == 0 || reps < 1 || !avg_us || form < 0 || form > 1) return rgbd360_map_set_error(m, -1, "bad arguments");
    if (const int rc = rgbd360_map_render_view(m, (size_t)job.n, true, &v)) return rc;
    const size_t n = (size_t)job.n;
    const vmap::RenderOut dev = {reinterpret_cast<float*>(v.stage), v.stage + 20 * n, reinterpret_cast<int32_t*>(v.stage + 4 * n),
                                 reinterpret_cast<int32_t*>(v.stage + 8 * n)};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        if (e0) hipEventDestroy(e0);
        return rgbd360_map_set_error(m, -103, "hipEventCreate failed");
    }
    int rc = 0;
    auto enqueue = [&] { return form == 0 ? render_enqueue<0>(m, v, job, dev) : render_enqueue<1>(m, v, job, dev); };
    auto one = [&](int which) { form == 0 ? render_launch_one<0>(v, job, which, dev) : render_launch_one<1>(v, job, which, dev); };
    rc = enqueue();      // once untimed; it leaves the planes as every timed pass finds them (minima: repeating a pass changes nothing)
    for (int what = 0; what < 4 && rc == 0; ++what) {
        bool ok = hipEventRecord(e0, v.stream) == hipSuccess;
        for (int k = 0; k < reps && rc == 0; ++k) {
            if (what < 3) one(what);
            else rc = enqueue();
        }
        float ms = 0.f;
        ok = ok && hipEventRecord(e1, v.stream) == hipSuccess && hipGetLastError() == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
             hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        if (rc == 0 && !ok) rc = rgbd360_map_set_error(m, -100, "timing the render kernels failed");
        avg_us[what] = ms * 1000.f / (float)reps;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (rc) return rc;
    // the counters of the last whole render
    RENDER_HIPC(m, hipMemcpyAsync(v.stats_host, v.stats, vmap::kRnWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, v.stream));
    RENDER_HIPC(m, hipStreamSynchronize(v.stream));
    render_fill_stats(v.stats_host, stats);
    if (atomics) *atomics = (long long)v.stats_host[vmap::kRnAtomics];
    return rgbd360_map_time_extract_scan(m, reps, &avg_us[4]);
}

#undef RENDER_HIPC
