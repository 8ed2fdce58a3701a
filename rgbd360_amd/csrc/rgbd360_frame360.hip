// rgbd360_frame360.hip -- the Frame360 side of the C ABI (include/rgbd360_hip.h): sphere / sensor clouds, the PCL normal map, planar
// regions with their moments, hulls and colour descriptors, the bilateral grid filter, the spherical stitcher (SURVEY.md 8 rows
// a13-a15, 8f rank 2).  A translation unit of its own since round 6: an experiment on the alignment kernels (rgbd360_api.hip) no longer
// rebuilds these 50 kernels and vice versa.  It sees a context only through f360_state.h: the stages' scratch lives in an F360State the
// context owns (created on the first Frame360 call, on the context's device and stream), every buffer of it an owner of its memory
// (dev_buf.h); runtime choices reach the kernels' template parameters through dispatch.h.  No CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rgbd360_hip.h"
#include "../../include/rgbd360_hip_diag.h"
#include "knobs.h"
#include "host_wait.h"
#include "dispatch.h"
#include "dev_buf.h"
#include "device_math.h"
#include "frame360_kernels.h"
#include "pbmap_register.h"
#include "f360_state.h"

using namespace r360;

constexpr int kF360MaxSlots = 4096;

// What the stages keep between calls.  `ctx` in this file is an F360State: the member names are those the code used while it lived in
// rgbd360_ctx (stream, p.device, tag, err + the f_* / b_* scratch).  Every buffer owns its memory (dev_buf.h): the state's destructor
// frees them, f360_ensure and the stages grow them.
struct F360State {
    struct { int device = 0; } p;
    hipStream_t stream = nullptr;       // the owning context's stream (not owned)
    hostwait::SpinTag tag;              // pinned sequence number the stages' last kernel stores (host_wait.h); this state's own
    std::string err;                    // copied into the context's error string when an entry point returns (F360Enter)
    // Frame360 stage scratch (normals / plane segmentation), grown with the frame (f360_ensure)
    DevBuf<float> f_xyz, f_normals, f_dist;
    DevBuf<uint8_t> f_change, f_hd, f_depth_raw;
    f360::EdgeCloudSrc f_cloud_pending = {nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr};      // a sphere cloud the depth-edge kernel is to form (frame_planes)
    DevBuf<int> f_label, f_slot_of_root, f_root_of_slot, f_nslots, f_window, f_count_of_slot;
    DevBuf<unsigned long long> f_count, f_mom;
    PinnedBuf<unsigned char> f_pack_host{hostwait::kPublishedFlags};      // packed region records: written by the device straight into pinned host memory
    DevBuf<f360::SlotFrame> f_frames;                             // per region slot: centroid + in-plane basis (hull stage)
    DevBuf<unsigned long long> f_ext;                             // per region slot: 256 directional extremes {ordered dot, pixel} (overflow path of the block tables)
    DevBuf<int> f_hull_keys;                                      // per block of k_f360_hull_extremes: the slots of its table rows ...
    DevBuf<unsigned long long> f_hull_vals;                       // ... and the rows (256 extremes each)
    // colour image of the next plane calls (rgbd360_set_plane_color_image) and the per-region colour table (k_f360_colour)
    DevBuf<uint8_t> f_col_owned;                                  // device copy of a host image
    f360::ColourImage f_col_img = {nullptr, 0, 1};
    int f_col_rows = 0, f_col_cols = 0;                           // size of the registered image
    DevBuf<unsigned long long> f_col;                             // [kF360MaxSlots][kColWords]: device table ...
    PinnedBuf<unsigned long long> f_col_host{hostwait::kPublishedFlags};      // ... and the pinned copy of the rows in use
    DevBuf<int> f_samp_off, f_samp_n;                             // the dominant colour's samples: where a slot's start in the pool, how many arrived
    DevBuf<int2> f_samp_grid;                                     // ... and the slot's sample grid {sr, sc}
    DevBuf<unsigned> f_samp_pool;                                 // one entry per pixel of the largest frame seen
    bool f_col_ran = false;                                       // the last plane call filled f_col_host
    DevBuf<unsigned char> b_sum;                                  // bilateral grid: fixed-point sums, then the counts (one allocation, one memset) ...
    DevBuf<float2> b_a, b_b;                                      // ... and two float2 ping-pong arrays
    PinnedBuf<float4> f_models_host;                              // pinned staging of the refinement's plane models
    DevBuf<unsigned> b_mm;                                        // per-block {min, max} codes of the depth range
    PinnedBuf<unsigned> b_mm_host{hostwait::kPublishedFlags};     // ... the pair, published into pinned memory
    // applying the depth models (depth_apply.h): host images on their way to a kernel, the image records, the results of a host call,
    // the counters and sums of an evaluation
    DevBuf<uint8_t> da_up;
    DevBuf<unsigned char> da_img;
    PinnedBuf<unsigned char> da_img_host;
    DevBuf<float> da_out;
    DevBuf<unsigned long long> da_words;
    PinnedBuf<unsigned long long> da_words_host;
    hipEvent_t da_ev[2] = {nullptr, nullptr};      // measurement (rgbd360_depth_apply_timing): around the kernel of a depth_apply.h entry
    bool da_timing = false, da_timed = false;
    DevBuf<float> f_tab;
    int f_tab_rows = 0, f_tab_cols = 0, f_tab_conv = -1;      // what the resident angle tables were built for
    // measurement (rgbd360_frame_planes_stage_timing): events on `stream` at the stage boundaries of a frame_planes call -- before the
    // cloud / depth-edge kernel, behind it (row a13), behind the normal map (a14), behind the last kernel of the plane stage (a15)
    hipEvent_t f_stage_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool f_stage_timing = false, f_stage_valid = false;
    int f_planes_available = 0;     // regions that passed every filter in the last plane call (may exceed the caller's max_planes)
    bool f_planes_ran = false;      // the pinned pack holds the records of a plane call (rgbd360_debug_plane_sums)
    int f_refine = 0;               // segmentAndRefine's refinement after `segment` (rgbd360_set_plane_refinement)
    float f_refine_dist = 0.02f;    // PlaneRefinementComparator's default distance threshold
    int f_refine_changed = 0, f_refine_sweeps = 0;      // pixels relabelled / Jacobi sweeps of the last call
    DevBuf<float4> f_models;        // per slot {a, b, c, d} of the planes `segment` produced (x = NaN: no plane)
    PinnedBuf<int> f_flags_host{hostwait::kPublishedFlags};      // device-visible: per-sweep "something changed" flags + the relabelled-pixel counter
};

namespace {
#define HIPC(ctx, expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                               \
            return -(int)e_ - 1000;                                                                       \
        }                                                                                                 \
    } while (0)

int fail(F360State* ctx, int code, const char* msg) {
    ctx->err = msg;
    return code;
}

// Every entry point: the context's F360State (created on first use) as `ctx`; whatever error text the call leaves goes into the context
// (rgbd360_last_error) on every return path.
struct F360Enter {
    rgbd360_ctx* c;
    F360State* s;
    explicit F360Enter(rgbd360_ctx* c_) : c(c_), s(c_ ? rgbd360_ctx_f360(c_) : nullptr) {
        if (s) s->err.clear();
    }
    ~F360Enter() {
        if (s && !s->err.empty()) rgbd360_ctx_set_error(c, s->err.c_str());
    }
};
#define F360_ENTER(c_)                                                    \
    F360Enter enter_((c_));                                               \
    F360State* ctx = enter_.s;                                            \
    if (!ctx) return (c_) ? -103 : -1
}  // namespace

F360State* f360_state_create(int device, hipStream_t stream) {
    F360State* s = new F360State();
    s->p.device = device;
    s->stream = stream;
    if (hostwait::spin_tag_init(&s->tag) != hipSuccess) {
        delete s;
        return nullptr;
    }
    return s;
}
void f360_state_destroy(F360State* ctx) {
    if (!ctx) return;
    for (hipEvent_t e : ctx->f_stage_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : ctx->da_ev)
        if (e) hipEventDestroy(e);
    hostwait::spin_tag_free(&ctx->tag);
    delete ctx;
}

// ---------------------------------------------------------------------------------------------------------
// Frame360 stages: normal map (row a14) and planar regions + inlier moments (row a15)
// ---------------------------------------------------------------------------------------------------------
namespace {
// the scratch of a frame of n pixels: every buffer and its element count (a buffer that is large enough stays as it is; the tables
// per region slot have one size for good)
int f360_ensure(F360State* ctx, size_t n) {
    using namespace f360;
    const size_t hull_blocks = (n + (size_t)kHullBlock * kHullChunks - 1) / ((size_t)kHullBlock * kHullChunks);
    HIPC(ctx, ctx->f_xyz.ensure(n * 3));
    HIPC(ctx, ctx->f_normals.ensure(n * 3));
    HIPC(ctx, ctx->f_dist.ensure(n));
    HIPC(ctx, ctx->f_change.ensure(n));
    HIPC(ctx, ctx->f_hd.ensure(3 * n + 64));       // depth-change bit mask: rows x ceil(cols / 64) words <= n/8 + 8 rows bytes, cols >= 3
    HIPC(ctx, ctx->f_label.ensure(n));
    HIPC(ctx, ctx->f_count.ensure(n));             // (the refinement's two work label planes later: 2 n ints)
    HIPC(ctx, ctx->f_slot_of_root.ensure(n));
    HIPC(ctx, ctx->f_window.ensure(n));
    HIPC(ctx, ctx->f_hull_keys.ensure(hull_blocks * kHullHash));
    HIPC(ctx, ctx->f_hull_vals.ensure(hull_blocks * kHullHash * kHullDirs));
    HIPC(ctx, ctx->f_depth_raw.ensure(n * 4));
    HIPC(ctx, ctx->f_root_of_slot.ensure(kF360MaxSlots));
    HIPC(ctx, ctx->f_nslots.ensure(1));
    static_assert(kF360MaxSlots * sizeof(unsigned int) % sizeof(unsigned long long) == 0, "the maxima fill whole words of f_mom");
    HIPC(ctx, ctx->f_mom.ensure((size_t)kMomReplicas * kF360MaxSlots * 9       // + the per-slot maxima (mom_max_of), unsigned ints
                                + (size_t)kF360MaxSlots * sizeof(unsigned int) / sizeof(unsigned long long)));
    HIPC(ctx, ctx->f_count_of_slot.ensure(kF360MaxSlots));
    // pinned: header, one moment record per slot, one hull record per slot behind them
    HIPC(ctx, ctx->f_pack_host.ensure(kF360PackHeader + (size_t)kF360MaxSlots * (sizeof(F360SlotRecord) + sizeof(F360HullRecord))));
    HIPC(ctx, ctx->f_frames.ensure(kF360MaxSlots));
    HIPC(ctx, ctx->f_ext.ensure((size_t)kF360MaxSlots * kHullPhases * kHullDirs));
    return 0;
}

// distance to the nearest depth change of the organised cloud in ctx->f_xyz -> ctx->f_dist (device); f_hd holds the bit mask
static void launch_distance_map(F360State* ctx, int rows, int cols, float max_depth_change_factor, int depth_mode, unsigned* clear_words = nullptr,
                                int n_clear = 0) {
    using namespace f360;
    const int pitch = (cols + 63) / 64;
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(ctx->f_hd.get());
    const dim3 ge((cols + kEdgeTW - 1) / kEdgeTW, (rows + kEdgeTH - 1) / kEdgeTH);
    if (ctx->f_cloud_pending.depth) {       // rgbd360_frame_planes: the cloud has not been formed yet -- this kernel does it on the way
        const EdgeCloudSrc& cs = ctx->f_cloud_pending;
        const int spec = (cs.convention >= 0 && cs.convention <= 2 && (cs.depth_type | 1) == 1 && (depth_mode | 1) == 1) ? cs.convention * 4 + cs.depth_type * 2 + depth_mode : -1;
        with_int<-1, 11>(spec, [&](auto S) {
            hipLaunchKernelGGL((k_f360_edge_bits<true, S>), ge, dim3(kEdgeTW), 0, ctx->stream, ctx->f_xyz, rows, cols, max_depth_change_factor, depth_mode,
                               pitch, bits, ctx->f_cloud_pending, ctx->f_xyz);
        });
        ctx->f_cloud_pending.depth = nullptr;
    } else {
        hipLaunchKernelGGL((k_f360_edge_bits<false>), ge, dim3(kEdgeTW), 0, ctx->stream, ctx->f_xyz, rows, cols, max_depth_change_factor, depth_mode,
                           pitch, bits, ctx->f_cloud_pending, ctx->f_xyz);
    }
    if (ctx->f_stage_timing) hipEventRecord(ctx->f_stage_ev[1], ctx->stream);
    hipLaunchKernelGGL(k_f360_distmap, dim3(pitch, (rows + kDistTH - 1) / kDistTH), dim3(kDistThreads), 0, ctx->stream, bits, rows, cols,
                       pitch, ctx->f_dist, clear_words, n_clear);
}

// normals of the organised cloud in ctx->f_xyz -> ctx->f_normals (device)
int f360_normals_dev(F360State* ctx, int rows, int cols, float max_depth_change_factor, float smoothing_size, int depth_mode) {
    using namespace f360;
    // (the upper bound leaves smoothing_size <= 9.5: the widest sweep window is R = 9, and no k_f360_normals_sweep<10> is built)
    if (smoothing_size < 1.f || smoothing_size + 2.5f > (float)kF360R)
        return fail(ctx, -1, "normal_smoothing_size out of range (the distance map is truncated at 12 px)");
    const dim3 gt((cols + kNT_W - 1) / kNT_W, (rows + kNT_H - 1) / kNT_H);
    // Register sweep for the pixels whose window is int(smoothing_size) squared (nearly all of them), the tiled integral-image kernel
    // for the 32 x 16 tiles the sweep lists (depth edges, far points).  Claim flags + tile list: the first bytes of f_change, which the
    // distance map does not touch (the plane stage rewrites it); the distance-map kernel clears them on its way.
    const int R = (int)smoothing_size;
    const bool use_sweep = R >= 3 && R <= 9 && ((size_t)gt.x * gt.y * 2 + 2) * sizeof(unsigned) <= (size_t)rows * cols &&
                           (size_t)rows * cols * 12 < ((size_t)1 << 31);      // the sweep addresses its rows with 32-bit buffer offsets
    const int n_tiles = (int)(gt.x * gt.y);
    unsigned *flags = nullptr, *list = nullptr;            // {claimed flag per tile}, {count, tile ids ...}
    if (use_sweep) {
        flags = reinterpret_cast<unsigned*>(ctx->f_change.get());
        list = flags + n_tiles;
    }
    launch_distance_map(ctx, rows, cols, max_depth_change_factor, depth_mode, flags, use_sweep ? n_tiles + 1 : 0);
    if (use_sweep) {
        // rows per wave: 3 waves per SIMD stay resident (146 VGPRs: 3072 on the chip); a wave costs R - 1 warm-up rows + its rows, and
        // the kernel ends with the most loaded SIMD, so the wave count is kept within one residency round.  16 rows per wave is the
        // measured optimum at 2048 x 1024 (28.6 us; 8: 28.5, 24: 31.6, 32: 39.4), 16-32 at 4096 x 2048 (85-88 us; 48: 101) --
        // tools/normals_seg_sweep.sh
        const int OW = 63 - R;
        const int strips = (cols + OW - 1) / OW;
        const int rounds = std::max(1, (int)lround((double)strips * rows / 32.0 / 3072.0));
        const int segs = std::max(1, 3072 * rounds / strips);
        // after R - 1 warm-up rows a wave sweeps whole passes of R output rows (its unrolled loop body)
        int seg = std::max(2 * R, (rows + segs - 1) / segs);
        seg = (seg + R - 1) / R * R;
        if (const char* e = knobs::debug("RGBD360_SWEEP_SEG")) {      // tuning knob
            const int v = atoi(e);
            if (v >= 4 && v <= 4096) seg = v;
        }
        const int units = strips * ((rows + seg - 1) / seg);
        const dim3 gs((units + kSweepWaves - 1) / kSweepWaves), bs(64 * kSweepWaves);
        // (no window plane: nothing downstream reads the per-pixel window size -- it was a 4 B/px store of both normal-map kernels,
        // 33 MB at 4096 x 2048, kept from the days the two kernels were compared through it; round 6)
        with_int<3, 9>(R, [&](auto RR) {
            hipLaunchKernelGGL((k_f360_normals_sweep<RR>), gs, bs, 0, ctx->stream, ctx->f_xyz, ctx->f_dist, rows, cols, smoothing_size, depth_mode, seg,
                               ctx->f_normals, (int*)nullptr, flags, list, (int)gt.x);
        });
    }
    // two tiles fit a CU: 512 blocks walk the sweep's list (every tile of the frame when there was no sweep)
    hipLaunchKernelGGL(k_f360_normals_tiled, dim3(list ? std::min(n_tiles, 512) : n_tiles), dim3(kNT_THREADS), 0, ctx->stream, ctx->f_xyz,
                       ctx->f_dist, rows, cols, smoothing_size, depth_mode, ctx->f_normals, (int*)nullptr, (const unsigned*)list, (int)gt.x,
                       n_tiles);
    if (ctx->f_stage_timing) hipEventRecord(ctx->f_stage_ev[2], ctx->stream);
    HIPC(ctx, hipGetLastError());
    return 0;
}

// pcl::FastBilateralFilter on the organised cloud in ctx->f_xyz (device), z filtered in place
int f360_bilateral_dev(F360State* ctx, int rows, int cols, float sigma_s, float sigma_r) {
    using namespace f360;
    if (!(sigma_s > 0.f) || !(sigma_r > 0.f)) return fail(ctx, -1, "sigma_s and sigma_r must be positive");
    const int n = rows * cols;
    constexpr int kMmBlocks = 64;
    HIPC(ctx, ctx->b_mm.ensure(2 * kMmBlocks));
    HIPC(ctx, ctx->b_mm_host.ensure(2));
    // the depth range: per-block pairs, folded and published by a one-wave kernel; the host spins on the tag (no memset, copy or stream synchronise)
    const int mm_blocks = std::min(kMmBlocks, (n + 4 * kBilatMmThreads - 1) / (4 * kBilatMmThreads));
    hipLaunchKernelGGL(k_bilat_minmax, dim3(mm_blocks), dim3(kBilatMmThreads), 0, ctx->stream, ctx->f_xyz, n, ctx->b_mm);
    hipLaunchKernelGGL(k_bilat_minmax_publish, dim3(1), dim3(64), 0, ctx->stream, ctx->b_mm, mm_blocks, ctx->b_mm_host, ctx->tag.h, ++ctx->tag.seq);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hostwait::wait(ctx->tag, ctx->stream));
    const unsigned mm[2] = {reinterpret_cast<const volatile unsigned*>(ctx->b_mm_host.get())[0], reinterpret_cast<const volatile unsigned*>(ctx->b_mm_host.get())[1]};
    if (mm[0] > mm[1]) return 0;                                   // no finite z: the cloud stays as it is
    auto decode = [](unsigned e) {
        const unsigned u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
        float v;
        memcpy(&v, &u, sizeof(v));
        return v;
    };
    BilatGrid g;
    g.sigma_s = sigma_s; g.sigma_r = sigma_r;
    g.base_min = decode(mm[0]); g.base_max = decode(mm[1]);
    const float base_delta = g.base_max - g.base_min;
    g.nx = (int)((float)(cols - 1) / sigma_s) + 1 + 2 * kBilatPadXY;
    g.ny = (int)((float)(rows - 1) / sigma_s) + 1 + 2 * kBilatPadXY;
    const double nz = (double)(base_delta / sigma_r) + 1 + 2 * kBilatPadZ;
    const double cells_d = (double)g.nx * g.ny * nz;
    if (!(cells_d < 64e6)) return fail(ctx, -1, "bilateral grid too large (depth range / sigma_r)");
    g.nz = (int)(base_delta / sigma_r) + 1 + 2 * kBilatPadZ;
    const size_t cells = (size_t)g.nx * g.ny * g.nz;
    HIPC(ctx, ctx->b_sum.ensure(cells * (sizeof(unsigned long long) + sizeof(int))));      // sums, then counts: one allocation, one memset
    HIPC(ctx, ctx->b_a.ensure(cells));
    HIPC(ctx, ctx->b_b.ensure(cells));
    unsigned long long* b_sum = reinterpret_cast<unsigned long long*>(ctx->b_sum.get());
    int* b_cnt = reinterpret_cast<int*>(b_sum + cells);      // (behind THIS call's cells: the buffer may be larger)
    HIPC(ctx, hipMemsetAsync(b_sum, 0, cells * (sizeof(unsigned long long) + sizeof(int)), ctx->stream));
    const dim3 gp((n + 255) / 256), gc((unsigned)((cells + 255) / 256)), b(256);
    hipLaunchKernelGGL(k_bilat_scatter, gp, b, 0, ctx->stream, ctx->f_xyz, rows, cols, g, b_sum, b_cnt);
    hipLaunchKernelGGL(k_bilat_init, gc, b, 0, ctx->stream, b_sum, b_cnt, cells, ctx->b_a, ctx->b_b);
    float2 *data = ctx->b_a, *buffer = ctx->b_b;
    const int offs[3] = {g.ny * g.nz, g.nz, 1};
    for (int dim = 0; dim < 3; ++dim)
        for (int it = 0; it < 2; ++it) {
            std::swap(data, buffer);
            hipLaunchKernelGGL(k_bilat_blur, gc, b, 0, ctx->stream, buffer, data, g, offs[dim]);
        }
    hipLaunchKernelGGL(k_bilat_interp, gp, b, 0, ctx->stream, ctx->f_xyz, rows, cols, g, data);
    HIPC(ctx, hipGetLastError());
    return 0;
}

// Convex hull of the directional extremes of a region (<= kHullRecPts points), its area (shoelace) and mass centre -- the roles of
// mrpt::pbmap::Plane::calcConvexHull / computeMassCenterAndArea (Frame360.h:1025-1031) in the region's own in-plane frame.
struct HullStats {
    int n = 0;                  // hull vertices
    double area = 0, cu = 0, cv = 0;
    int np = 0;                 // vertices kept for the plane record (<= RGBD360_HULL_MAX), counter-clockwise in (u, v)
    double pu[RGBD360_HULL_MAX], pv[RGBD360_HULL_MAX];
};
struct HullPt {
    double x, y;                // (no constructor: the work arrays below are not cleared -- 48 KB per plane when they were std::pairs)
    bool operator<(const HullPt& o) const { return x < o.x || (x == o.x && y < o.y); }
    bool operator==(const HullPt& o) const { return x == o.x && y == o.y; }
};
HullStats hull_stats(const float (*uv)[2], int K) {
    // The points arrive roughly in boundary order (direction order), but the four direction sets each saw their own sample of the
    // region's pixels, so neighbours may be swapped along an edge: Andrew's monotone chain on the sorted points, which assumes nothing.
    HullPt p[f360::kHullRecPts];
    int n = 0;
    for (int k = 0; k < K && k < f360::kHullRecPts; ++k) {
        const float a = uv[k][0], b = uv[k][1];            // (one read each of the pinned record)
        if (std::isfinite(a) && std::isfinite(b)) { p[n].x = a; p[n].y = b; ++n; }
    }
    std::sort(p, p + n);
    n = (int)(std::unique(p, p + n) - p);
    HullStats h;
    if (n < 3) return h;
    auto cross = [](const HullPt& o, const HullPt& a, const HullPt& b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); };
    HullPt H[2 * f360::kHullRecPts + 2];
    int m = 0;
    for (int i = 0; i < n; ++i) {                          // lower hull
        while (m >= 2 && cross(H[m - 2], H[m - 1], p[i]) <= 0) --m;
        H[m++] = p[i];
    }
    for (int i = n - 2, lo = m + 1; i >= 0; --i) {         // upper hull
        while (m >= lo && cross(H[m - 2], H[m - 1], p[i]) <= 0) --m;
        H[m++] = p[i];
    }
    --m;                                                   // the first point again
    if (m < 3) return h;
    double a2 = 0, cu = 0, cv = 0;
    for (int i = 0; i < m; ++i) {
        const HullPt &a = H[i], &b = H[(i + 1) % m];
        const double cr = a.x * b.y - a.y * b.x;
        a2 += cr;
        cu += (a.x + b.x) * cr;
        cv += (a.y + b.y) * cr;
    }
    if (!(fabs(a2) > 0)) return h;
    h.n = m;
    h.area = fabs(a2) / 2;
    h.cu = cu / (3 * a2);
    h.cv = cv / (3 * a2);
    // the polygon of the record: the hull itself, or its extreme vertices in RGBD360_HULL_MAX evenly spaced directions (Andrew's chain
    // leaves the vertices counter-clockwise, so the picks come out in hull order)
    if (m <= RGBD360_HULL_MAX) {
        for (int i = 0; i < m; ++i) { h.pu[i] = H[i].x; h.pv[i] = H[i].y; }
        h.np = m;
    } else {
        // (the directions turn counter-clockwise like the vertices: the extreme vertex only ever moves forward -- one full scan for the
        // first direction, then a walk; with a scan per direction this loop was 4 us per plane, 0.19 ms of a 4096 x 2048 frame's call)
        static const struct Dirs {
            double c[RGBD360_HULL_MAX], s[RGBD360_HULL_MAX];
            Dirs() { for (int k = 0; k < RGBD360_HULL_MAX; ++k) { const double th = 2.0 * 3.14159265358979323846 * k / RGBD360_HULL_MAX; c[k] = cos(th); s[k] = sin(th); } }
        } D;
        auto proj = [&](int i, int k) { return ((double)H[i].x - h.cu) * D.c[k] + ((double)H[i].y - h.cv) * D.s[k]; };
        int best = 0;
        for (int i = 1; i < m; ++i)
            if (proj(i, 0) > proj(best, 0)) best = i;
        int last = -1, first = -1;
        for (int k = 0; k < RGBD360_HULL_MAX; ++k) {
            for (int steps = 0; steps < m && proj((best + 1) % m, k) > proj(best, k); ++steps) best = (best + 1) % m;
            if (best == last || best == first) continue;
            if (first < 0) first = best;
            last = best;
            h.pu[h.np] = H[best].x; h.pv[h.np] = H[best].y; ++h.np;
        }
    }
    return h;
}
// area / centre of plane P from the hull record of its slot (pinned, written by k_f360_hull_pack); the moment rectangle stays in
// area_moment, and is the fallback when a region has fewer than three extreme points
void apply_hull(rgbd360_plane& P, const f360::F360HullRecord& R) {
    const HullStats h = hull_stats(R.uv, std::min(std::max(R.n, 0), f360::kHullRecPts));
    P.hull_points = h.n;
    P.hull_n = 0;
    if (h.n >= 3) {
        P.area = (float)h.area;
        for (int k = 0; k < 3; ++k) P.center_hull[k] = (float)((double)R.c[k] + h.cu * (double)R.e1[k] + h.cv * (double)R.e2[k]);
        // counter-clockwise seen from the side the record's normal points to: (e1, e2, e1 x e2) is right-handed, so the (u, v) order is
        // counter-clockwise about e1 x e2 -- reversed when the normal points the other way
        const double e3[3] = {(double)R.e1[1] * R.e2[2] - (double)R.e1[2] * R.e2[1], (double)R.e1[2] * R.e2[0] - (double)R.e1[0] * R.e2[2],
                              (double)R.e1[0] * R.e2[1] - (double)R.e1[1] * R.e2[0]};
        const bool flip = e3[0] * P.normal[0] + e3[1] * P.normal[1] + e3[2] * P.normal[2] < 0;
        P.hull_n = h.np;
        for (int i = 0; i < h.np; ++i) {
            const int src = flip ? h.np - 1 - i : i;
            for (int k = 0; k < 3; ++k) P.hull[i][k] = (float)((double)R.c[k] + h.pu[src] * (double)R.e1[k] + h.pv[src] * (double)R.e2[k]);
        }
    } else {
        P.area = P.area_moment;
        for (int k = 0; k < 3; ++k) P.center_hull[k] = P.centroid[k];
    }
}
const f360::F360HullRecord* hull_records(const F360State* ctx) {
    return reinterpret_cast<const f360::F360HullRecord*>(ctx->f_pack_host + f360::kF360PackHeader + (size_t)kF360MaxSlots * sizeof(f360::F360SlotRecord));
}
// ... and its moment records, behind the header (read after the wait that follows the kernels which wrote them)
const f360::F360SlotRecord* slot_records(const F360State* ctx) {
    return reinterpret_cast<const f360::F360SlotRecord*>(ctx->f_pack_host + f360::kF360PackHeader);
}
// the extremes of the CURRENT labels (ctx->f_label) against the frames of the slots, packed for the host; enqueued on the stream
int launch_hull(F360State* ctx, int rows, int cols, bool clear_first) {
    using namespace f360;
    const int n = rows * cols;
    if (clear_first) hipLaunchKernelGGL(k_f360_hull_clear, dim3((kF360MaxSlots * kHullPhases * kHullDirs + 255) / 256), dim3(256), 0, ctx->stream, ctx->f_nslots, kF360MaxSlots, ctx->f_ext);
    const int nblk = (n + kHullBlock * kHullChunks - 1) / (kHullBlock * kHullChunks);      // (f_hull_keys / f_hull_vals hold the rows of the context's largest frame)
    static const int n_cus = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return v;
    }();
    const auto extremes = nblk > n_cus ? k_f360_hull_extremes_two : k_f360_hull_extremes;       // more blocks than CUs: the two-per-CU build of the kernel
    hipLaunchKernelGGL(extremes, dim3(nblk), dim3(kHullBlock), 0, ctx->stream, ctx->f_xyz, ctx->f_label, ctx->f_slot_of_root, rows, cols,
                       ctx->f_frames, ctx->f_ext, ctx->f_hull_keys, ctx->f_hull_vals, kHullFramesLds);
    hipLaunchKernelGGL(k_f360_hull_merge, dim3(64, kHullMergeSplit), dim3(kHullDirs), 0, ctx->stream, ctx->f_nslots, kF360MaxSlots, ctx->f_hull_keys, ctx->f_hull_vals,
                       nblk, ctx->f_ext);
    hipLaunchKernelGGL(k_f360_hull_pack, dim3(256), dim3(kHullDirs), 0, ctx->stream, ctx->f_xyz, ctx->f_frames, ctx->f_ext, ctx->f_nslots, kF360MaxSlots,
                       const_cast<F360HullRecord*>(hull_records(ctx)));
    return 0;
}

// eigenpairs of a symmetric 3x3 in ascending order (cyclic Jacobi, float64) -- pcl::eigen33's role for the smallest one
void sorted_eigen3(const double C[3][3], double evals[3], double evecs[3][3]) {    // evecs[k] = eigenvector of evals[k]
    double ev[3], V[3][3];
    pbm::jacobi3(C, ev, V);
    int o[3] = {0, 1, 2};
    std::stable_sort(o, o + 3, [&](int a, int c) { return ev[a] < ev[c]; });
    for (int k = 0; k < 3; ++k) {
        evals[k] = ev[o[k]];
        for (int i = 0; i < 3; ++i) evecs[k][i] = V[i][o[k]];
    }
}
// What a region's exact sums say about it (float64): centroid, covariance, its eigenpairs in ascending order -- evecs[0] is the plane
// normal -- and the extent descriptors of rgbd360_hip.h from the two in-plane moments.
struct RegionFit {
    double c[3], C[3][3], evals[3], evecs[3][3];
    float area_moment, elongation, ppal_dir[3];
};
// m: the three first and six second moments in metres, N: what they were summed over (the frame's regions here, the map's in map_planes.h)
RegionFit region_fit_moments(const double m[9], double N) {
    RegionFit f;
    const double cx = m[0] / N, cy = m[1] / N, cz = m[2] / N;
    const double C[3][3] = {{m[3] / N - cx * cx, m[4] / N - cx * cy, m[5] / N - cx * cz},
                            {m[4] / N - cx * cy, m[6] / N - cy * cy, m[7] / N - cy * cz},
                            {m[5] / N - cx * cz, m[7] / N - cy * cz, m[8] / N - cz * cz}};
    f.c[0] = cx; f.c[1] = cy; f.c[2] = cz;
    memcpy(f.C, C, sizeof(C));
    sorted_eigen3(C, f.evals, f.evecs);
    const double l1 = std::max(f.evals[1], 0.0), l2 = std::max(f.evals[2], 0.0);    // in-plane moments
    f.area_moment = (float)(12.0 * sqrt(l1 * l2));
    f.elongation = (float)(l1 > 0 ? sqrt(l2 / l1) : INFINITY);
    for (int q = 0; q < 3; ++q) f.ppal_dir[q] = (float)f.evecs[2][q];
    return f;
}
RegionFit region_fit(const f360::F360SlotRecord& R) {
    double m[9];
    for (int q = 0; q < 9; ++q) m[q] = (double)(long long)R.mom[q] / f360::kMomScale;      // fixed point -> metres
    return region_fit_moments(m, (double)R.count);
}
// ... into the plane record (f360_planes_dev for the regions of `segment`, f360_refine_dev again for the grown inlier sets)
void apply_extent(rgbd360_plane& P, const RegionFit& f, int count) {
    P.count = count;
    P.area_moment = f.area_moment;
    P.elongation = f.elongation;
    for (int q = 0; q < 3; ++q) P.ppal_dir[q] = f.ppal_dir[q];
}

// Colour descriptors of the regions in their slots (k_f360_colour over the CURRENT labels), enqueued on the stream: the table rows in
// use land in pinned host memory.  Only when a colour image of this cloud's geometry is registered.
bool launch_colour(F360State* ctx, int rows, int cols) {
    using namespace f360;
    ctx->f_col_ran = false;
    const ColourImage& im = ctx->f_col_img;
    if (!im.rgb || im.sub < 1 || ctx->f_col_rows / im.sub != rows || ctx->f_col_cols / im.sub != cols) return false;
    const int n = rows * cols;
    // the table, its pinned copy, and the dominant colour's sample pool (one entry per pixel bounds the sum of min(count, kModeCap) over the regions)
    const size_t words = (size_t)kF360MaxSlots * kColWords;
    if (ctx->f_col.ensure(words) != hipSuccess || ctx->f_col_host.ensure(words) != hipSuccess || ctx->f_samp_off.ensure(kF360MaxSlots) != hipSuccess ||
        ctx->f_samp_n.ensure(kF360MaxSlots) != hipSuccess || ctx->f_samp_grid.ensure(kF360MaxSlots) != hipSuccess || ctx->f_samp_pool.ensure((size_t)n) != hipSuccess)
        return false;
    const ColourSamples smp = {ctx->f_count_of_slot, ctx->f_samp_off, ctx->f_samp_n, ctx->f_samp_grid, ctx->f_samp_pool};
    hipLaunchKernelGGL(k_f360_colour_offsets, dim3(1), dim3(1024), 0, ctx->stream, ctx->f_nslots, kF360MaxSlots, ctx->f_count_of_slot, ctx->f_samp_off, ctx->f_samp_n,
                       ctx->f_samp_grid, ctx->f_col);
    hipLaunchKernelGGL(k_f360_colour, dim3((n + kAggThreads * kColPerThread - 1) / (kAggThreads * kColPerThread)), dim3(kAggThreads), 0, ctx->stream,
                       ctx->f_label, ctx->f_slot_of_root, rows, cols, im, ctx->f_col, smp);
    hipLaunchKernelGGL(k_f360_colour_mode, dim3(256), dim3(kModeThreads), 0, ctx->stream, ctx->f_nslots, kF360MaxSlots, smp, ctx->f_col, ctx->f_col_host);
    ctx->f_col_ran = true;
    return true;
}
// sums of a slot's row -> the plane's colour fields (rgbd360_hip.h); the record stays colourless when no colour pass ran
void apply_colour(const F360State* ctx, rgbd360_plane& P, int slot) {
    P.color_count = 0;
    for (int k = 0; k < 3; ++k) P.color_nrgb[k] = P.color_dev[k] = 0.f;
    P.intensity = 0.f;
    for (int k = 0; k < 74; ++k) P.hist_h[k] = 0.f;
    P.color_mode_count = 0;
    for (int k = 0; k < 3; ++k) P.color_mode[k] = 0.f;
    P.intensity_mode = P.color_concentration = 0.f;
    if (!ctx->f_col_ran) return;
    const volatile unsigned long long* w = ctx->f_col_host + (size_t)slot * f360::kColWords;
    const double n = (double)w[7];
    unsigned long long total = 0;
    for (int k = 0; k < f360::kColBins; ++k) total += w[f360::kColSums + k];
    if (total == 0) return;
    P.color_count = (int)w[7];
    if (n > 0) {
        for (int k = 0; k < 3; ++k) {
            const double m = (double)w[k] / n / 65536.0;
            const double var = (double)w[3 + k] / n / (65536.0 * 65536.0) - m * m;
            P.color_nrgb[k] = (float)m;
            P.color_dev[k] = (float)sqrt(std::max(var, 0.0));
        }
        P.intensity = (float)((double)w[6] / n);
    }
    for (int k = 0; k < f360::kColBins; ++k) P.hist_h[k] = (float)((double)w[f360::kColSums + k] / (double)total);
    const volatile unsigned long long* md = w + f360::kColSums + f360::kColBins;      // k_f360_colour_mode: N, kept, mode q (3), sum S, iterations, threshold^2
    if (md[0] > 0 && md[1] > 0) {
        P.color_mode_count = (int)md[0];
        for (int k = 0; k < 3; ++k) P.color_mode[k] = (float)((double)md[2 + k] / 65536.0);
        P.intensity_mode = (float)((double)md[5] / (double)md[1]);
        P.color_concentration = (float)((double)md[1] / (double)md[0]);
    }
}

// regions of (ctx->f_xyz, ctx->f_normals) -> labels (device ctx->f_label) + plane list (host)
// segmentAndRefine's refinement on the device (frame360_kernels.h k_f360_refine_tile): block-Jacobi steps of the two raster passes
// until nothing changes, then the grown inliers are added to their planes' integer sums and the extent descriptors recomputed.
int f360_refine_dev(F360State* ctx, int rows, int cols, int nslots, std::vector<rgbd360_plane>& planes, const std::vector<int>& plane_slot) {
    using namespace f360;
    const int n = rows * cols;
    HIPC(ctx, ctx->f_models.ensure(kF360MaxSlots + 1));      // + one slot: the relabelled-pixel counter
    int* d_changed = reinterpret_cast<int*>(ctx->f_models + kF360MaxSlots);     // (device memory: 166 k atomics into pinned host memory took 8 ms)
    int* d_activity = d_changed + 1;                                            // bumped by every relaxation step that changed a label
    constexpr int kFlags = 64;
    HIPC(ctx, ctx->f_flags_host.ensure(kFlags + 1));
    // (the plane models go up from a pinned buffer: a copy out of pageable memory is staged by the runtime)
    HIPC(ctx, ctx->f_models_host.ensure(kF360MaxSlots));
    float4* models = ctx->f_models_host;
    for (int s2 = 0; s2 < nslots; ++s2) models[s2] = make_float4(NAN, 0.f, 0.f, 0.f);
    for (size_t k = 0; k < planes.size(); ++k)
        models[plane_slot[k]] = make_float4(planes[k].normal[0], planes[k].normal[1], planes[k].normal[2], planes[k].d);
    HIPC(ctx, hipMemcpyAsync(ctx->f_models, models, (size_t)nslots * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    // work labels (plane slot / -1 invalid / -2 free): the two halves of f_count (its counts are spent once the slots are assigned) and
    // f_window (only live during the normal-map stage); tile flags: the first bytes of f_dist (normal-map stage only)
    int* w[3] = {reinterpret_cast<int*>(ctx->f_count.get()), reinterpret_cast<int*>(ctx->f_count.get()) + n, ctx->f_window};
    const int tiles_y = (rows + kRefTH - 1) / kRefTH, tiles_x = (cols + 63) / 64;
    unsigned char* tile_free = reinterpret_cast<unsigned char*>(ctx->f_dist.get());
    HIPC(ctx, hipMemsetAsync(tile_free, 0, (size_t)tiles_x * tiles_y, ctx->stream));
    // X (w[1]) starts as the pass labels (written by the same launch) and is relaxed in place; pass 2 starts from a copy of pass 1's result (w[2])
    hipLaunchKernelGGL(k_f360_refine_init, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->f_label, ctx->f_slot_of_root, ctx->f_models, n, cols, tiles_x,
                       w[0], w[1], tile_free, d_changed);
    const dim3 g(tiles_x, (tiles_y + kRefWaves - 1) / kRefWaves), b(64 * kRefWaves);
    const int n_lds = nslots <= 2048 ? nslots : 0;         // plane models staged in LDS when they fit 32 KB
    const size_t lds_bytes = (size_t)n_lds * sizeof(float4);
    int sweeps = 0;
    for (int pass = 1; pass <= 2; ++pass) {
        const int* W0 = pass == 1 ? w[0] : w[2];
        if (pass == 2) HIPC(ctx, hipMemcpyAsync(w[2], w[1], (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        bool converged = false;
        // A launch relaxes until the growth chains stop moving (its waves poll their rings, k_f360_refine_tile); the host looks at the
        // "something changed" flag of every second launch (a check costs a stream synchronisation): the run ends with a launch that
        // changed nothing.
        constexpr int kPerCheck = 2;
        static const int kPolls = [] { const char* e = knobs::debug("RGBD360_REFINE_POLLS"); return e ? atoi(e) : 4096; }();      // (512 until round 4: a launch whose growth chains were still moving gave up after 0.34 ms and cost a second round of launches + a host synchronisation)
        static const int kQuiet = [] { const char* e = knobs::debug("RGBD360_REFINE_QUIET"); return e ? atoi(e) : 32; }();
        const int max_rounds = tiles_x + tiles_y + 8;      // a tile is final once its predecessor tiles are: one launch per tile at worst
        for (int round = 0; round < max_rounds && !converged; ++round) {
            volatile int* flags = ctx->f_flags_host;
            for (int k = 0; k < kPerCheck; ++k) flags[k] = 0;
            for (int k = 0; k < kPerCheck; ++k) {
                with_choice<1, 2>(pass == 2, [&](auto P) {
                    with_choice<0, 1>(n_lds > 0, [&](auto L) {
                        hipLaunchKernelGGL((k_f360_refine_tile<P, decltype(L)::value != 0>), g, b, lds_bytes, ctx->stream, ctx->f_xyz, W0, w[1], ctx->f_models, ctx->f_refine_dist,
                                           rows, cols, tiles_y, tile_free, ctx->f_flags_host + k, d_activity, kPolls, kQuiet, n_lds);
                    });
                });
                ++sweeps;
            }
            HIPC(ctx, hipGetLastError());
            HIPC(ctx, hostwait::tag_and_wait(ctx->tag, ctx->stream));      // (a tag kernel + host spin: ~10 us less than hipStreamSynchronize, host_wait.h)
            converged = flags[kPerCheck - 1] == 0;      // a launch that changes nothing is a fixed point: every later one repeats it
        }
        if (!converged) return fail(ctx, -7, "plane refinement did not converge");
        if (knobs::debug("RGBD360_REFINE_DEBUG")) {
            int act = 0;
            hipMemcpy(&act, d_activity, sizeof(int), hipMemcpyDeviceToHost);
            int nfree = 0;
            std::vector<unsigned char> tf((size_t)tiles_x * tiles_y);
            hipMemcpy(tf.data(), tile_free, tf.size(), hipMemcpyDeviceToHost);
            for (unsigned char v : tf) nfree += v ? 1 : 0;
            for (int ty = 0; ty < tiles_y; ++ty) {
                std::string line;
                for (int tx = 0; tx < tiles_x; ++tx) { const int v = tf[(size_t)ty * tiles_x + tx]; line += v == 0 ? '.' : (v == 1 ? 'o' : (v < 11 ? char('0' + v - 1) : '#')); }
                fprintf(stderr, "%s\n", line.c_str());
            }
            fprintf(stderr, "[refine dbg] pass %d: activity (steps that changed a label, cumulative) %d, free tiles %d of %d, sweeps %d\n", pass, act, nfree, tiles_x * tiles_y, sweeps);
        }
    }
    const int* W0 = w[1];
    hipLaunchKernelGGL(k_f360_refine_commit, dim3((n + kCommitThreads * kCommitPerThread - 1) / (kCommitThreads * kCommitPerThread)), dim3(kCommitThreads), 0, ctx->stream, ctx->f_xyz, ctx->f_label, w[0], W0, ctx->f_root_of_slot, n,
                       ctx->f_count_of_slot, ctx->f_mom, kF360MaxSlots, d_changed);
    hipLaunchKernelGGL(k_f360_mom_reduce, dim3((kF360MaxSlots * 9 + 255) / 256), dim3(256), 0, ctx->stream, ctx->f_mom, ctx->f_nslots, kF360MaxSlots,
                       ctx->f_root_of_slot, ctx->f_count_of_slot, ctx->f_pack_host, (const int*)d_changed, ctx->f_flags_host + kFlags);
    // the contour PCL hands to calcConvexHull is that of the REFINED region, projected with the plane `segment` fitted: extremes of the
    // committed labels against the frames k_f360_slot_frames left before the refinement
    if (const int rc_h = launch_hull(ctx, rows, cols, /*clear_first=*/true)) return rc_h;
    launch_colour(ctx, rows, cols);          // the colour of the REFINED inlier sets (Frame360.h:1045-1046 run on the refined regions); a no-op without a colour image
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hostwait::tag_and_wait(ctx->tag, ctx->stream));      // (a tag kernel + host spin: ~10 us less than hipStreamSynchronize, host_wait.h)
    ctx->f_refine_changed = ctx->f_flags_host[kFlags];
    ctx->f_refine_sweeps = sweeps;
    // count and the extent descriptors of the grown inlier sets (Frame360.h:1010-1037 derives them from the refined inlier cloud);
    // centroid / normal / d / curvature stay those of `segment`, as PCL's PlanarRegion keeps them
    const F360SlotRecord* recs = slot_records(ctx);
    for (size_t k = 0; k < planes.size(); ++k)          // the grown inlier sets against the same a-priori bound as the segment's
        if (!f360_mom_in_range(recs[plane_slot[k]].count, recs[plane_slot[k]].max_abs))
            return fail(ctx, -8, "region moments out of range (N max(|x|,|y|,|z|)^2 >= 3.4e10 m^2, or a point beyond 2896 m)");
    for (size_t k = 0; k < planes.size(); ++k) {
        const F360SlotRecord& R = recs[plane_slot[k]];
        rgbd360_plane& P = planes[k];
        apply_extent(P, region_fit(R), R.count);
        apply_hull(P, hull_records(ctx)[plane_slot[k]]);
        apply_colour(ctx, P, plane_slot[k]);
    }
    return 0;
}

int f360_planes_dev(F360State* ctx, int rows, int cols, int min_inliers, float angular_threshold, float distance_threshold,
                    float max_curvature, int depth_mode, rgbd360_plane* planes, int max_planes, int* n_planes) {
    using namespace f360;
    const int n = rows * cols;
    uint8_t* flags = ctx->f_change;
    hipLaunchKernelGGL(k_f360_link_flags, dim3((cols + kLinkTW - 1) / kLinkTW, (rows + kLinkTH - 1) / kLinkTH), dim3(kLinkTW), 0, ctx->stream,
                       ctx->f_xyz, ctx->f_normals, rows, cols, cosf(angular_threshold), distance_threshold, depth_mode, flags);
    // run starts as compact per-row lists for the root pass and the slot assignment: in f_window (the normal-map stage's window plane,
    // spent by now; the refinement takes it over later) and, for the counts, in the tail of f_hd (the depth-change mask is spent once the distance map exists)
    int* run_starts = ctx->f_window;        // (no other use of this plane since round 6; f_slot_of_root stays free for k_f360_assign_list's writes)
    int* n_run_starts = reinterpret_cast<int*>(ctx->f_hd + (((size_t)n + 15) & ~(size_t)15));      // n + 4 rows <= 3 n + 64 bytes
    const bool seg_rows = cols % 4 == 0 && cols >= 1024 && cols <= kRunSegs * kRunSegSteps * 256;       // (flags and labels are hipMalloc'ed: rows of whole, aligned dwords)
    if (seg_rows)
        hipLaunchKernelGGL(k_f360_ccl_runs_seg, dim3(rows), dim3(64 * kRunSegs), 0, ctx->stream, flags, rows, cols, ctx->f_label, run_starts, n_run_starts);
    else
        hipLaunchKernelGGL(k_f360_ccl_runs, dim3((rows + kRunRowsPerBlock - 1) / kRunRowsPerBlock), dim3(64 * kRunRowsPerBlock), 0, ctx->stream,
                           flags, rows, cols, ctx->f_label, run_starts, n_run_starts);
    {
        const dim3 gb((cols + kBandCols - 1) / kBandCols, (rows + kBandRows - 1) / kBandRows);
        with_choice<kBandGroupsMax, kBandGroupsMax / 2>(kBandGroupsMax >= 16 && gb.x * gb.y >= 1536, [&](auto G) {
            hipLaunchKernelGGL((k_f360_ccl_merge_band<G>), gb, dim3(kBandCols * G), 0, ctx->stream, flags, rows, cols, ctx->f_label);
        });
    }
    constexpr int kTopLevel = kBandRows == 64 ? kBandLevels : kBandLevels + 2;      // 64-row bands: every 64th row in one launch behind them
    for (int level = kBandLevels; level <= kTopLevel && (1 << level) < rows; ++level) {
        const bool all_above = level == kTopLevel;
        const int n_rows = all_above ? (rows - 1) / (1 << level) : (rows - 1 - (1 << level)) / (2 << level) + 1;
        hipLaunchKernelGGL(k_f360_ccl_merge_level, dim3((cols + 255) / 256, n_rows), dim3(256), 0, ctx->stream, flags, rows, cols,
                           ctx->f_label, level, all_above ? 1 : 0);
    }
#ifdef F360_DEBUG_COUNTERS
    {
        unsigned long long h[8];
        hipStreamSynchronize(ctx->stream);
        hipMemcpyFromSymbol(h, HIP_SYMBOL(f360::g_dbg), sizeof(h));
        fprintf(stderr, "[f360 dbg] after merge: unions %llu find-hops %llu atomicMin %llu longest walk %llu\n", h[0], h[1], h[2], h[3]);
    }
#endif
    hipLaunchKernelGGL(k_f360_ccl_roots_list, dim3(rows), dim3(kRootsThreads), 0, ctx->stream, run_starts, n_run_starts, cols, ctx->f_label, ctx->f_count);
#ifdef F360_DEBUG_COUNTERS
    {
        unsigned long long h[8], z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        hipStreamSynchronize(ctx->stream);
        hipMemcpyFromSymbol(h, HIP_SYMBOL(f360::g_dbg), sizeof(h));
        fprintf(stderr, "[f360 dbg] after roots: find-hops %llu (cumulative) longest walk %llu\n", h[1], h[3]);
        hipMemcpyToSymbol(HIP_SYMBOL(f360::g_dbg), z, sizeof(z));
    }
#endif
    hipLaunchKernelGGL(k_f360_finish_count, dim3((n + kCntThreads * kCntPerThread - 1) / (kCntThreads * kCntPerThread)), dim3(kCntThreads), 0,
                       ctx->stream, flags, n, ctx->f_label, ctx->f_count, ctx->f_nslots);
    const dim3 bagg(kAggThreads);
    hipLaunchKernelGGL(k_f360_assign_list, dim3(rows), dim3(kAssignThreads), 0, ctx->stream, run_starts, n_run_starts, cols, ctx->f_label, ctx->f_count,
                       min_inliers, kF360MaxSlots, ctx->f_slot_of_root, ctx->f_root_of_slot, ctx->f_count_of_slot, ctx->f_nslots, ctx->f_mom,
                       f360::kMomReplicas);
    const dim3 gmom((n + kAggThreads * kMomPerThread - 1) / (kAggThreads * kMomPerThread));
    hipLaunchKernelGGL(k_f360_moments, gmom, bagg, 0, ctx->stream, ctx->f_xyz, ctx->f_label, ctx->f_slot_of_root, n, ctx->f_mom, kF360MaxSlots);
    // hull stage: per slot the in-plane frame (and an empty extremes row); the extremes themselves now, or -- with the refinement
    // switched on -- once the refined labels are committed (f360_refine_dev)
    // The header + records go straight into pinned host memory (a few KB over PCIe): no copy to enqueue, one wait.  (Four copies into
    // pageable vectors with two waits used to cost ~0.1 ms of the 0.45 ms call.)  The frame kernel packs them on its way (it sums the
    // moment replicas anyway); k_f360_mom_reduce only runs behind the refinement's commit, which changes the sums.
    hipLaunchKernelGGL(k_f360_slot_frames, dim3(256), dim3(64), 0, ctx->stream, ctx->f_mom, ctx->f_nslots, kF360MaxSlots,
                       ctx->f_count_of_slot, ctx->f_frames, ctx->f_ext, ctx->f_root_of_slot, ctx->f_pack_host);
    ctx->f_col_ran = false;
    if (!ctx->f_refine) {
        if (const int rc_h = launch_hull(ctx, rows, cols, /*clear_first=*/false)) return rc_h;
        launch_colour(ctx, rows, cols);       // (a no-op without a colour image of this geometry)
    }
    if (ctx->f_stage_timing) {
        hipEventRecord(ctx->f_stage_ev[3], ctx->stream);
        ctx->f_stage_valid = true;
    }
    HIPC(ctx, hipGetLastError());
    // one tag kernel behind the chain + a host spin (~10 us less than hipStreamSynchronize, host_wait.h).  Until round 5 the chain's last
    // kernel published the tag from its last block: 256 blocks x a system-scope fence cost 10-22 us more than this launch.
    HIPC(ctx, hostwait::tag_and_wait(ctx->tag, ctx->stream));
    const int nslots = *reinterpret_cast<const volatile int*>(ctx->f_pack_host.get());
    ctx->f_planes_ran = true;
    if (nslots > kF360MaxSlots) return fail(ctx, -7, "more than 4096 regions exceed min_inliers");
    const F360SlotRecord* recs = slot_records(ctx);
    // the fixed-point sums are exact only inside their range (frame360_kernels.h, kMomScale): refused a priori, from the
    // region's count and largest coordinate, before any sum is decoded -- a wrapped sum can look as plausible as a right one
    for (int s = 0; s < nslots; ++s)
        if (!f360_mom_in_range(recs[s].count, recs[s].max_abs))
            return fail(ctx, -8, "region moments out of range (N max(|x|,|y|,|z|)^2 >= 3.4e10 m^2, or a point beyond 2896 m)");
    std::vector<int> order(nslots);
    for (int s = 0; s < nslots; ++s) order[s] = s;
    std::sort(order.begin(), order.end(), [&](int a, int c) { return recs[a].root < recs[c].root; });   // PCL's order: by first pixel
    // Planes are built for every region first: when more than max_planes pass the curvature filter the LARGEST ones are kept
    // (still in PCL's order) instead of the first -- the regions lowest in the image (typically the floor) used to be the ones
    // cut -- and the total is remembered for rgbd360_planes_available so that an adapter can grow its buffer and call again.
    std::vector<rgbd360_plane> all;
    std::vector<int> all_slot;      // region slot of every plane (its sums live in row `slot` of the moment table)
    all.reserve(nslots);
    for (int oi = 0; oi < nslots; ++oi) {
        const int s = order[oi];
        RegionFit f = region_fit(recs[s]);
        const double cx = f.c[0], cy = f.c[1], cz = f.c[2];
        const double ev = f.evals[0];
        double* v = f.evecs[0];
        double d = -(v[0] * cx + v[1] * cy + v[2] * cz);
        if ((-cx) * v[0] + (-cy) * v[1] + (-cz) * v[2] < 0) {     // orient towards the viewpoint (origin)
            v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2];
            d = -(v[0] * cx + v[1] * cy + v[2] * cz);
        }
        const double tr = f.C[0][0] + f.C[1][1] + f.C[2][2];
        const double curvature = tr != 0 ? fabs(ev / tr) : 0;
        if (!(curvature < max_curvature)) continue;
        all.emplace_back();
        all_slot.push_back(s);
        rgbd360_plane& P = all.back();
        P.centroid[0] = (float)cx; P.centroid[1] = (float)cy; P.centroid[2] = (float)cz;
        P.normal[0] = (float)v[0]; P.normal[1] = (float)v[1]; P.normal[2] = (float)v[2];
        P.d = (float)d;
        P.curvature = (float)curvature;
        P.root = recs[s].root;
        apply_extent(P, f, recs[s].count);
        apply_colour(ctx, P, s);      // (with the refinement on: empty here, filled by f360_refine_dev below)
        if (!ctx->f_refine) apply_hull(P, hull_records(ctx)[s]);
        else {                   // filled by f360_refine_dev below
            P.area = P.area_moment;
            P.hull_points = 0;
            P.hull_n = 0;
            for (int k = 0; k < 3; ++k) P.center_hull[k] = P.centroid[k];
        }
    }
    ctx->f_refine_changed = ctx->f_refine_sweeps = 0;
    if (ctx->f_refine && !all.empty()) {
        const int rc = f360_refine_dev(ctx, rows, cols, nslots, all, all_slot);
        if (rc) return rc;
    }
    ctx->f_planes_available = (int)all.size();
    int np = 0;
    if ((int)all.size() <= max_planes) {
        for (const rgbd360_plane& P : all) planes[np++] = P;
    } else {
        std::vector<int> by_count(all.size());
        for (size_t k = 0; k < all.size(); ++k) by_count[k] = (int)k;
        std::stable_sort(by_count.begin(), by_count.end(), [&](int a, int c) { return all[a].count > all[c].count; });
        std::vector<char> keep(all.size(), 0);
        for (int k = 0; k < max_planes; ++k) keep[by_count[k]] = 1;
        for (size_t k = 0; k < all.size(); ++k)
            if (keep[k]) planes[np++] = all[k];
    }
    *n_planes = np;
    return 0;
}
// The angle tables of a rows x cols sphere image in `convention` (0 .. 2), resident in ctx->f_tab: sin / cos of the azimuth per column,
// then sin / cos of the polar angle per row.  They follow the reference's float expressions and are computed on the host (rows + cols
// values).  Shared by the sphere cloud and the voxel map's image insert (voxel_map.h).
int sphere_tables_dev(F360State* ctx, int rows, int cols, int convention) {
    if (!(ctx->f_tab && ctx->f_tab_rows == rows && ctx->f_tab_cols == cols && ctx->f_tab_conv == convention)) {      // else: the angle tables of this geometry are already on the device
        const size_t ntab = (size_t)2 * cols + 2 * rows;
        std::vector<float> tab(ntab);
        float *st = tab.data(), *ct = st + cols, *sp = ct + cols, *cp = sp + rows;
        if (convention == 0) {          // Frame360.h:562-585
            const float angle_pixel(cols / (2 * kPI));
            const float angle_pixel_inv(1 / angle_pixel);
            const float offset_phi = kPI * 31.5 / 180;
            for (int r = 0; r < rows; ++r) {
                float phi_i = offset_phi - r * angle_pixel_inv;
                sp[r] = sinf(phi_i);
                cp[r] = cosf(phi_i);
            }
            for (int c = 0; c < cols; ++c) {
                float theta_i = c * angle_pixel_inv;
                st[c] = sinf(theta_i);
                ct[c] = cosf(theta_i);
            }
        } else if (convention == 1) {   // Frame360_stereo.h:470-490
            const float step_theta = 2 * kPI / cols;
            const float step_phi = step_theta;
            const int start_phi = 166;
            for (int r = 0; r < rows; ++r) {
                float phi = (r + start_phi) * step_phi - kPI / 2;
                cp[r] = cosf(phi);
                sp[r] = sinf(phi);
            }
            for (int c = 0; c < cols; ++c) {
                float theta = c * step_theta - kPI;
                st[c] = sinf(theta);
                ct[c] = cosf(theta);
            }
        } else {                        // RPI.h:4556-4571
            const float angle_res = 2 * kPI / cols;
            const float half_nRows = 0.5 * rows - 0.5;
            for (int c = 0; c < cols; ++c) {
                float theta = c * angle_res;
                st[c] = sinf(theta);
                ct[c] = cosf(theta);
            }
            for (int r = 0; r < rows; ++r) {
                float phi = (half_nRows - r) * angle_res;
                sp[r] = sinf(phi);
                cp[r] = cosf(phi);
            }
        }
        HIPC(ctx, ctx->f_tab.ensure(ntab));
        ctx->f_tab_conv = -1;
        HIPC(ctx, hipMemcpyAsync(ctx->f_tab, tab.data(), ntab * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        HIPC(ctx, hipStreamSynchronize(ctx->stream));      // `tab` (pageable) must outlive the copy
        ctx->f_tab_rows = rows; ctx->f_tab_cols = cols; ctx->f_tab_conv = convention;
    }
    return 0;
}
// organised cloud of one spherical depth image -> ctx->f_xyz (device)
// defer_to_edge_kernel: tables and depth are put in place, the points themselves are left to k_f360_edge_bits<true> (the next stage
// of rgbd360_frame_planes), which forms them anyway
int sphere_cloud_dev(F360State* ctx, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                     bool depth_on_device = false, bool defer_to_edge_kernel = false) {
    if (convention < 0 || convention > 2 || (depth_type != 0 && depth_type != 1)) return fail(ctx, -1, "bad arguments");
    const size_t dpx = depth_type == 0 ? 2 : 4;
    if (const int rc = sphere_tables_dev(ctx, rows, cols, convention)) return rc;
    const void* d_depth = depth;
    size_t d_step = depth_step;
    if (!depth_on_device) {
        HIPC(ctx, hipMemcpy2DAsync(ctx->f_depth_raw, (size_t)cols * dpx, depth, depth_step, (size_t)cols * dpx, rows, hipMemcpyHostToDevice,
                                   ctx->stream));
        d_depth = ctx->f_depth_raw;
        d_step = (size_t)cols * dpx;
    }
    float* d_tab = ctx->f_tab;
    ctx->f_cloud_pending.depth = nullptr;
    if (defer_to_edge_kernel) {
        ctx->f_cloud_pending = {d_depth, d_step, depth_type, convention, d_tab, d_tab + cols, d_tab + 2 * cols, d_tab + 2 * cols + rows};
        if (!depth_on_device) HIPC(ctx, hipStreamSynchronize(ctx->stream));      // the caller may reuse its host image
        return 0;
    }
    // consecutive lanes = consecutive pixels, one 12-byte store per lane, four pixels (256 apart) per thread
    hipLaunchKernelGGL(k_sphere_cloud_s4, dim3((cols + 1023) / 1024, rows), dim3(256), 0, ctx->stream, d_depth, d_step, depth_type, rows, cols,
                       convention, d_tab, d_tab + cols, d_tab + 2 * cols, d_tab + 2 * cols + rows, ctx->f_xyz);
    HIPC(ctx, hipGetLastError());
    if (!depth_on_device) HIPC(ctx, hipStreamSynchronize(ctx->stream));      // the caller may reuse its host image
    return 0;
}

// How an entry point that works on a rows x cols frame begins: the size check (min_side: 1, or what the stage's neighbourhoods need),
// the context's device, the scratch of that many pixels and -- when the caller brings a cloud -- its upload into ctx->f_xyz
int f360_begin(F360State* ctx, int rows, int cols, int min_side, const float* xyz = nullptr) {
    if (rows < min_side || cols < min_side || (long long)rows * cols >= (1ll << 30)) return fail(ctx, -1, "bad image size");
    hipSetDevice(ctx->p.device);
    const size_t n = (size_t)rows * cols;
    if (const int rc = f360_ensure(ctx, n)) return rc;
    if (xyz) HIPC(ctx, hipMemcpyAsync(ctx->f_xyz, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return 0;
}
// ... and how it ends when the caller wants a map on the host: `count` floats, complete when the call returns
int f360_download(F360State* ctx, float* host, const float* dev, size_t count) {
    HIPC(ctx, hipMemcpyAsync(host, dev, count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
}  // namespace

extern "C" int rgbd360_sphere_cloud(rgbd360_ctx* ctx_, const void* depth, size_t depth_step, int depth_type, int rows, int cols,
                         int convention, float* host_out_xyz) {
    F360_ENTER(ctx_);
    if (!depth || !host_out_xyz) return -1;
    if (const int rc = f360_begin(ctx, rows, cols, 1)) return rc;
    if (const int rc = sphere_cloud_dev(ctx, depth, depth_step, depth_type, rows, cols, convention)) return rc;
    return f360_download(ctx, host_out_xyz, ctx->f_xyz, (size_t)rows * cols * 3);
}

extern "C" int rgbd360_normals(rgbd360_ctx* ctx_, const float* xyz, int rows, int cols, float max_depth_change_factor,
                               float normal_smoothing_size, int depth_mode, float* normals_out) {
    F360_ENTER(ctx_);
    if (!xyz || !normals_out) return -1;
    if (const int rc = f360_begin(ctx, rows, cols, 3, xyz)) return rc;
    if (const int rc = f360_normals_dev(ctx, rows, cols, max_depth_change_factor, normal_smoothing_size, depth_mode)) return rc;
    return f360_download(ctx, normals_out, ctx->f_normals, (size_t)rows * cols * 3);
}

extern "C" int rgbd360_bilateral_filter(rgbd360_ctx* ctx_, const float* xyz, int rows, int cols, float sigma_s, float sigma_r,
                                       float* xyz_out) {
    F360_ENTER(ctx_);
    if (!xyz || !xyz_out) return -1;
    if (const int rc = f360_begin(ctx, rows, cols, 1, xyz)) return rc;
    if (const int rc = f360_bilateral_dev(ctx, rows, cols, sigma_s, sigma_r)) return rc;
    return f360_download(ctx, xyz_out, ctx->f_xyz, (size_t)rows * cols * 3);
}

extern "C" int rgbd360_distance_map(rgbd360_ctx* ctx_, const float* xyz, int rows, int cols, float max_depth_change_factor,
                                    int depth_mode, float* dist_out) {
    F360_ENTER(ctx_);
    if (!xyz || !dist_out) return -1;
    if (const int rc = f360_begin(ctx, rows, cols, 3, xyz)) return rc;
    launch_distance_map(ctx, rows, cols, max_depth_change_factor, depth_mode);
    HIPC(ctx, hipGetLastError());
    return f360_download(ctx, dist_out, ctx->f_dist, (size_t)rows * cols);
}

// measurement: HIP events at the stage boundaries of the context's later frame_planes calls (rgbd360_hip_diag.h)
extern "C" int rgbd360_frame_planes_stage_timing(rgbd360_ctx* ctx_, int on) {
    F360_ENTER(ctx_);
    hipSetDevice(ctx->p.device);
    if (on)
        for (hipEvent_t& e : ctx->f_stage_ev)
            if (!e) HIPC(ctx, hipEventCreate(&e));
    ctx->f_stage_timing = on != 0;
    ctx->f_stage_valid = false;
    return 0;
}
extern "C" int rgbd360_frame_planes_stage_times(rgbd360_ctx* ctx_, float us[3]) {
    F360_ENTER(ctx_);
    if (!us) return -1;
    if (!ctx->f_stage_timing || !ctx->f_stage_valid) return fail(ctx, -1, "no timed frame_planes call (rgbd360_frame_planes_stage_timing(ctx, 1) first; the refinement must be off)");
    hipSetDevice(ctx->p.device);
    HIPC(ctx, hipEventSynchronize(ctx->f_stage_ev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        HIPC(ctx, hipEventElapsedTime(&ms, ctx->f_stage_ev[k], ctx->f_stage_ev[k + 1]));
        us[k] = ms * 1000.f;
    }
    return 0;
}

extern "C" int rgbd360_planes_available(rgbd360_ctx* ctx_) {
    F360_ENTER(ctx_);
    return ctx->f_planes_available;
}

extern "C" int rgbd360_set_plane_refinement(rgbd360_ctx* ctx_, int enabled, float distance_threshold) {
    F360_ENTER(ctx_);
    if (enabled && !(distance_threshold > 0.f)) return fail(ctx, -1, "the refinement distance threshold must be positive");
    ctx->f_refine = enabled ? 1 : 0;
    if (enabled) ctx->f_refine_dist = distance_threshold;
    return 0;
}
extern "C" int rgbd360_set_plane_color_image(rgbd360_ctx* ctx_, const uint8_t* rgb, size_t rgb_step, int rows, int cols, int step, int on_device) {
    F360_ENTER(ctx_);
    hipSetDevice(ctx->p.device);
    if (!rgb) {
        ctx->f_col_img = {nullptr, 0, 1};
        ctx->f_col_rows = ctx->f_col_cols = 0;
        return 0;
    }
    if (rows < 1 || cols < 1 || step < 1 || step > 16 || rgb_step < (size_t)cols * 3) return fail(ctx, -1, "bad colour image geometry");
    if (on_device) {
        ctx->f_col_img = {rgb, rgb_step, step};
    } else {
        const size_t bytes = (size_t)rows * cols * 3;
        HIPC(ctx, hipStreamSynchronize(ctx->stream));       // a plane call still reading the previous copy
        HIPC(ctx, ctx->f_col_owned.ensure(bytes));
        HIPC(ctx, hipMemcpy2D(ctx->f_col_owned, (size_t)cols * 3, rgb, rgb_step, (size_t)cols * 3, rows, hipMemcpyHostToDevice));
        ctx->f_col_img = {ctx->f_col_owned, (size_t)cols * 3, step};
    }
    ctx->f_col_rows = rows; ctx->f_col_cols = cols;
    return 0;
}
extern "C" int rgbd360_debug_plane_sums(rgbd360_ctx* ctx_, int max, int* n, int32_t* root, int32_t* count, int64_t* mom) {
    F360_ENTER(ctx_);
    if (!n || max < 0) return -1;
    *n = 0;
    if (!ctx->f_pack_host || !ctx->f_planes_ran) return 0;
    const int ns_all = *reinterpret_cast<const volatile int*>(ctx->f_pack_host.get());
    const int ns = ns_all < kF360MaxSlots ? ns_all : kF360MaxSlots;
    const f360::F360SlotRecord* recs = slot_records(ctx);
    for (int s = 0; s < ns && s < max; ++s) {
        if (root) root[s] = recs[s].root;
        if (count) count[s] = recs[s].count;
        if (mom)
            for (int q = 0; q < 9; ++q) mom[(size_t)s * 9 + q] = (int64_t)recs[s].mom[q];
    }
    *n = ns;
    return 0;
}
extern "C" int rgbd360_plane_refinement_stats(rgbd360_ctx* ctx_, int* pixels_relabelled, int* sweeps) {
    F360_ENTER(ctx_);
    if (pixels_relabelled) *pixels_relabelled = ctx->f_refine_changed;
    if (sweeps) *sweeps = ctx->f_refine_sweeps;
    return 0;
}

extern "C" int rgbd360_plane_fit(rgbd360_ctx* ctx_, const float* xyz, const float* normals, int rows, int cols, int min_inliers,
                                 float angular_threshold, float distance_threshold, float max_curvature, int depth_mode,
                                 int32_t* labels_out, rgbd360_plane* planes_out, int max_planes, int* n_planes_out) {
    F360_ENTER(ctx_);
    if (!xyz || !normals || !planes_out || !n_planes_out || max_planes < 1) return -1;
    int rc = f360_begin(ctx, rows, cols, 2, xyz);
    if (rc) return rc;
    const size_t n = (size_t)rows * cols;
    HIPC(ctx, hipMemcpyAsync(ctx->f_normals, normals, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    rc = f360_planes_dev(ctx, rows, cols, min_inliers, angular_threshold, distance_threshold, max_curvature, depth_mode, planes_out,
                         max_planes, n_planes_out);
    if (rc) return rc;
    if (labels_out) HIPC(ctx, hipMemcpy(labels_out, ctx->f_label, n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

static int frame_planes_impl(F360State* ctx, const void* depth, size_t depth_step, int depth_type, int rows, int cols,
                             int convention, float max_depth_change_factor, float normal_smoothing_size, int min_inliers,
                             float angular_threshold, float distance_threshold, float max_curvature, int depth_mode,
                             float* xyz_out, float* normals_out, int32_t* labels_out, rgbd360_plane* planes_out,
                             int max_planes, int* n_planes_out, bool depth_on_device) {
    if (!depth || !planes_out || !n_planes_out || max_planes < 1) return -1;
    int rc = f360_begin(ctx, rows, cols, 3);
    if (rc) return rc;
    const size_t n = (size_t)rows * cols;
    // the cloud stays on the device; a host copy is only made when asked for
    ctx->f_stage_valid = false;
    if (ctx->f_stage_timing) hipEventRecord(ctx->f_stage_ev[0], ctx->stream);
    rc = sphere_cloud_dev(ctx, depth, depth_step, depth_type, rows, cols, convention, depth_on_device, /*defer_to_edge_kernel=*/true);
    if (rc) return rc;
    rc = f360_normals_dev(ctx, rows, cols, max_depth_change_factor, normal_smoothing_size, depth_mode);
    if (rc) {
        ctx->f_cloud_pending.depth = nullptr;
        return rc;
    }
    if (xyz_out) HIPC(ctx, hipMemcpyAsync(xyz_out, ctx->f_xyz, n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    rc = f360_planes_dev(ctx, rows, cols, min_inliers, angular_threshold, distance_threshold, max_curvature, depth_mode, planes_out,
                         max_planes, n_planes_out);
    if (rc) return rc;
    if (normals_out) HIPC(ctx, hipMemcpy(normals_out, ctx->f_normals, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (labels_out) HIPC(ctx, hipMemcpy(labels_out, ctx->f_label, n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// one sensor's cloud (pinhole + median down-sampling) from a host depth image into ctx->f_xyz (device)
static int sensor_cloud_upload(F360State* ctx, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int step, float min_depth,
                               float max_depth) {
    const size_t dpx = depth_type == 0 ? 2 : 4;
    if (rows < 1 || cols < 1 || step < 1 || step > 4 || rows / step < 1 || cols / step < 1 || depth_step < (size_t)cols * dpx ||
        (depth_type != 0 && depth_type != 1) || (long long)rows * cols >= (1ll << 30))
        return fail(ctx, -1, "bad arguments");
    if (const int rc = f360_begin(ctx, rows, cols, 1)) return rc;
    HIPC(ctx, hipMemcpy2DAsync(ctx->f_depth_raw, (size_t)cols * dpx, depth, depth_step, (size_t)cols * dpx, rows, hipMemcpyHostToDevice, ctx->stream));
    f360::SensorCloudArgs a;
    a.rows = rows; a.cols = cols; a.step = step;
    a.depth_f32 = depth_type;
    const float res_factor_VGA = cols / 640.0;                       // CloudRGBD.h:118-123
    const float focal_length = 525 * res_factor_VGA;
    a.inv_fx = 1.f / focal_length; a.inv_fy = 1.f / focal_length;
    a.ox = cols / 2 - 0.5; a.oy = rows / 2 - 0.5;
    a.min_depth = min_depth; a.max_depth = max_depth;
    const int on = (rows / step) * (cols / step);
    hipLaunchKernelGGL(f360::k_sensor_cloud, dim3((on + 255) / 256), dim3(256), 0, ctx->stream, ctx->f_depth_raw, (size_t)cols * dpx, a, ctx->f_xyz);
    HIPC(ctx, hipGetLastError());
    return 0;
}

extern "C" int rgbd360_sensor_cloud_ex(rgbd360_ctx* ctx_, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int step,
                                      float min_depth, float max_depth, float* xyz_out) {
    F360_ENTER(ctx_);
    if (!depth || !xyz_out) return -1;
    if (const int rc = sensor_cloud_upload(ctx, depth, depth_step, depth_type, rows, cols, step, min_depth, max_depth)) return rc;
    return f360_download(ctx, xyz_out, ctx->f_xyz, (size_t)(rows / step) * (cols / step) * 3);
}
extern "C" int rgbd360_sensor_cloud(rgbd360_ctx* ctx_, const uint16_t* depth, size_t depth_step, int rows, int cols, int step, float min_depth,
                                   float max_depth, float* xyz_out) {
    return rgbd360_sensor_cloud_ex(ctx_, depth, depth_step, 0, rows, cols, step, min_depth, max_depth, xyz_out);
}

// the cloud in ctx->f_xyz -> (filter) -> normal map -> regions -> planes, moved by Rt
static int cloud_planes_tail(F360State* ctx, int rows, int cols, float sigma_s, float sigma_r, float max_depth_change_factor,
                             float normal_smoothing_size, int min_inliers, float angular_threshold, float distance_threshold,
                             float max_curvature, int depth_mode, const float Rt[16], rgbd360_plane* planes_out, int max_planes,
                             int* n_planes_out) {
    int rc = 0;
    if (sigma_s > 0.f) {                                             // Frame360.h:493-499
        rc = f360_bilateral_dev(ctx, rows, cols, sigma_s, sigma_r);
        if (rc) return rc;
    }
    rc = f360_normals_dev(ctx, rows, cols, max_depth_change_factor, normal_smoothing_size, depth_mode);      // Frame360.h:949-957
    if (rc) return rc;
    rc = f360_planes_dev(ctx, rows, cols, min_inliers, angular_threshold, distance_threshold, max_curvature, depth_mode, planes_out,
                         max_planes, n_planes_out);                                                         // Frame360.h:958-996
    if (rc) return rc;
    if (Rt) {                                                        // plane.transform(Rt), Frame360.h:1046: sensor -> rig frame
        for (int k = 0; k < *n_planes_out; ++k) {
            rgbd360_plane& P = planes_out[k];
            double nn[3], cc[3], pp[3], hh[3];
            for (int i = 0; i < 3; ++i) {
                nn[i] = cc[i] = pp[i] = hh[i] = 0;
                for (int j = 0; j < 3; ++j) {
                    nn[i] += (double)Rt[j * 4 + i] * P.normal[j];
                    cc[i] += (double)Rt[j * 4 + i] * P.centroid[j];
                    pp[i] += (double)Rt[j * 4 + i] * P.ppal_dir[j];
                    hh[i] += (double)Rt[j * 4 + i] * P.center_hull[j];
                }
                cc[i] += (double)Rt[12 + i];
                hh[i] += (double)Rt[12 + i];
            }
            double dd = -(nn[0] * cc[0] + nn[1] * cc[1] + nn[2] * cc[2]);
            bool flipped = false;
            if (dd < 0) {                                            // keep the normal towards the new origin (Frame360.h:989-993)
                for (int i = 0; i < 3; ++i) nn[i] = -nn[i];
                dd = -dd;
                flipped = true;
            }
            for (int i = 0; i < 3; ++i) {
                P.normal[i] = (float)nn[i];
                P.centroid[i] = (float)cc[i];
                P.ppal_dir[i] = (float)pp[i];
                P.center_hull[i] = (float)hh[i];
            }
            P.d = (float)dd;
            const int hn = std::min(P.hull_n, (int)RGBD360_HULL_MAX);
            for (int v = 0; v < hn; ++v) {                           // the polygon travels with the plane
                double q[3];
                for (int i = 0; i < 3; ++i) q[i] = (double)Rt[0 * 4 + i] * P.hull[v][0] + (double)Rt[1 * 4 + i] * P.hull[v][1] + (double)Rt[2 * 4 + i] * P.hull[v][2] + (double)Rt[12 + i];
                for (int i = 0; i < 3; ++i) P.hull[v][i] = (float)q[i];
            }
            // a rigid motion keeps the polygon's sense about the MOVED normal; where the normal was turned round (the plane lies between the
            // sensor's origin and the rig's) the header's promise -- counter-clockwise seen from the side the normal points to -- needs the
            // vertex order reversed
            if (flipped)
                for (int a = 0, b = hn - 1; a < b; ++a, --b)
                    for (int i = 0; i < 3; ++i) std::swap(P.hull[a][i], P.hull[b][i]);
        }
    }
    return 0;
}

extern "C" int rgbd360_sensor_planes_ex(rgbd360_ctx* ctx_, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int step,
                                       float min_depth, float max_depth, float sigma_s, float sigma_r, float max_depth_change_factor,
                                       float normal_smoothing_size, int min_inliers, float angular_threshold, float distance_threshold,
                                       float max_curvature, const float Rt[16], rgbd360_plane* planes_out, int max_planes, int* n_planes_out) {
    F360_ENTER(ctx_);
    if (!depth || !planes_out || !n_planes_out || max_planes < 1) return -1;
    if (step < 1 || rows / step < 3 || cols / step < 3) return fail(ctx, -1, "bad image size");
    const int rc = sensor_cloud_upload(ctx, depth, depth_step, depth_type, rows, cols, step, min_depth, max_depth);
    if (rc) return rc;
    return cloud_planes_tail(ctx, rows / step, cols / step, sigma_s, sigma_r, max_depth_change_factor, normal_smoothing_size, min_inliers,
                             angular_threshold, distance_threshold, max_curvature, /*depth_mode=*/0, Rt, planes_out, max_planes, n_planes_out);
}
extern "C" int rgbd360_sensor_planes(rgbd360_ctx* ctx_, const uint16_t* depth, size_t depth_step, int rows, int cols, int step, float min_depth,
                                    float max_depth, float sigma_s, float sigma_r, float max_depth_change_factor,
                                    float normal_smoothing_size, int min_inliers, float angular_threshold, float distance_threshold,
                                    float max_curvature, const float Rt[16], rgbd360_plane* planes_out, int max_planes, int* n_planes_out) {
    return rgbd360_sensor_planes_ex(ctx_, depth, depth_step, 0, rows, cols, step, min_depth, max_depth, sigma_s, sigma_r, max_depth_change_factor,
                                    normal_smoothing_size, min_inliers, angular_threshold, distance_threshold, max_curvature, Rt, planes_out, max_planes,
                                    n_planes_out);
}

extern "C" int rgbd360_cloud_planes(rgbd360_ctx* ctx_, const float* xyz, int rows, int cols, float sigma_s, float sigma_r,
                                   float max_depth_change_factor, float normal_smoothing_size, int min_inliers, float angular_threshold,
                                   float distance_threshold, float max_curvature, int depth_mode, const float Rt[16],
                                   rgbd360_plane* planes_out, int max_planes, int* n_planes_out) {
    F360_ENTER(ctx_);
    if (!xyz || !planes_out || !n_planes_out || max_planes < 1) return -1;
    if (const int rc = f360_begin(ctx, rows, cols, 3, xyz)) return rc;
    return cloud_planes_tail(ctx, rows, cols, sigma_s, sigma_r, max_depth_change_factor, normal_smoothing_size, min_inliers, angular_threshold,
                             distance_threshold, max_curvature, depth_mode, Rt, planes_out, max_planes, n_planes_out);
}

extern "C" int rgbd360_frame_planes(rgbd360_ctx* ctx_, const void* depth, size_t depth_step, int depth_type, int rows, int cols,
                                    int convention, float max_depth_change_factor, float normal_smoothing_size, int min_inliers,
                                    float angular_threshold, float distance_threshold, float max_curvature, int depth_mode,
                                    float* xyz_out, float* normals_out, int32_t* labels_out, rgbd360_plane* planes_out,
                                    int max_planes, int* n_planes_out) {
    F360_ENTER(ctx_);
    return frame_planes_impl(ctx, depth, depth_step, depth_type, rows, cols, convention, max_depth_change_factor, normal_smoothing_size,
                             min_inliers, angular_threshold, distance_threshold, max_curvature, depth_mode, xyz_out, normals_out,
                             labels_out, planes_out, max_planes, n_planes_out, false);
}

extern "C" int rgbd360_frame_planes_dev(rgbd360_ctx* ctx_, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols,
                                        int convention, float max_depth_change_factor, float normal_smoothing_size, int min_inliers,
                                        float angular_threshold, float distance_threshold, float max_curvature, int depth_mode,
                                        rgbd360_plane* planes_out, int max_planes, int* n_planes_out, const float** xyz_dev,
                                        const float** normals_dev, const int32_t** labels_dev) {
    F360_ENTER(ctx_);
    const int rc = frame_planes_impl(ctx, depth_dev, depth_step, depth_type, rows, cols, convention, max_depth_change_factor,
                                     normal_smoothing_size, min_inliers, angular_threshold, distance_threshold, max_curvature, depth_mode,
                                     nullptr, nullptr, nullptr, planes_out, max_planes, n_planes_out, true);
    if (rc) return rc;
    if (xyz_dev) *xyz_dev = ctx->f_xyz;
    if (normals_dev) *normals_dev = ctx->f_normals;
    if (labels_dev) *labels_dev = ctx->f_label;
    return 0;
}

extern "C" int rgbd360_stitch_sphere(rgbd360_ctx* ctx_, const uint8_t* rgb8, const uint16_t* depth8, int sensor_rows, int sensor_cols,
                                     const float Rt_inv[128], const float K[4], uint8_t* sphere_rgb_out, uint16_t* sphere_depth_out,
                                     int* out_rows, int* out_cols) {
    F360_ENTER(ctx_);
    if (!rgb8 || !depth8 || !Rt_inv || !K || !sphere_rgb_out || !sphere_depth_out) return -1;
    if (sensor_rows < 1 || sensor_cols < 1 || sensor_rows > 4096 || sensor_cols > 4096) return fail(ctx, -1, "bad sensor image size");
    hipSetDevice(ctx->p.device);
    f360::StitchArgs a;
    memcpy(a.Rt_inv, Rt_inv, sizeof(a.Rt_inv));
    a.fx = K[0]; a.fy = K[1]; a.cx = K[2]; a.cy = K[3];
    a.sensor_rows = sensor_rows; a.sensor_cols = sensor_cols;
    a.W = sensor_rows * 8;                               // Frame360.h:391
    a.H = (int)(a.W * 0.5 * 60.0 / 180);                 // Frame360.h:392
    if (out_rows) *out_rows = a.H;
    if (out_cols) *out_cols = a.W;
    const float offsetPhi = a.H / 2 - 0.5;               // Frame360.h:1104-1106
    const float offsetTheta = -sensor_rows * 15 / 2 + 0.5;
    const float angle_pixel = 2 * kPI / a.W;
    std::vector<float> tab((size_t)2 * a.H + 2 * a.W);
    for (int r = 0; r < a.H; ++r) {
        const float phi_i = (offsetPhi - r) * angle_pixel;
        tab[r] = sinf(phi_i);
        tab[a.H + r] = cosf(phi_i);
    }
    for (int c = 0; c < a.W; ++c) {
        const float theta_i = (c + offsetTheta) * angle_pixel;
        tab[2 * a.H + c] = sinf(theta_i);
        tab[2 * a.H + a.W + c] = cosf(theta_i);
    }
    const size_t n_in = (size_t)8 * sensor_rows * sensor_cols, n_out = (size_t)a.H * a.W;
    // (a failed step returns at once: the temporaries' destructors free them, which waits for whatever the stream still holds -- and
    // `tab`, declared before them, outlives that wait)
    DevBuf<uint8_t> d_rgb, d_out_rgb;
    DevBuf<uint16_t> d_depth, d_out_depth;
    DevBuf<float> d_tab;
    HIPC(ctx, d_rgb.ensure(n_in * 3));
    HIPC(ctx, d_depth.ensure(n_in));
    HIPC(ctx, d_out_rgb.ensure(n_out * 3));
    HIPC(ctx, d_out_depth.ensure(n_out));
    HIPC(ctx, d_tab.ensure(tab.size()));
    HIPC(ctx, hipMemcpyAsync(d_rgb, rgb8, n_in * 3, hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(d_depth, depth8, n_in * 2, hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(f360::k_stitch_sphere, dim3((a.W + 255) / 256, a.H), dim3(256), 0, ctx->stream, a, d_rgb, d_depth, d_tab, d_tab + a.H,
                       d_tab + 2 * a.H, d_tab + 2 * a.H + a.W, d_out_rgb, d_out_depth);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipMemcpyAsync(sphere_rgb_out, d_out_rgb, n_out * 3, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(sphere_depth_out, d_out_depth, n_out * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// the resident voxel-grid global map (rgbd360_map_*)
// ---------------------------------------------------------------------------------------------------------
#include "voxel_map.h"
#include "map_edit.h"
#include "gn_math.h"
#include "map_align.h"
#include "map_align_plane.h"
#include "map_align_batch.h"
#include "rig_calib.h"
#include "map_pyramid.h"
#include "map_merge.h"
#include "map_normals.h"
#include "map_align_gicp.h"
#include "map_colour.h"
#include "map_align_colour.h"
#include "map_align_robust.h"
#include "map_raycast.h"
#include "map_carve.h"
#include "map_planes.h"
#include "depth_train.h"
#include "depth_apply.h"

#ifdef RGBD360_HULL_DBG
extern "C" int rgbd360_debug_hull_stats(unsigned long long* out /* [4096][8] */) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(f360::g_hull_dbg), sizeof(unsigned long long) * 4096 * 8) == hipSuccess ? 0 : -1;
}
#endif

