// rgbd360_api.hip -- host side of the C ABI declared in include/rgbd360_hip.h.
//
// Mirrors the call protocol of RegisterPhotoICP (RPI.h:201-288 setters, 480-516 frame setup, 4519-4784
// alignFrames360): frames are converted to device-resident pyramids once; an alignment is a sequence of
// {fused per-pixel pass, solve} launches per pyramid level on one HIP stream, with the Gauss-Newton state
// (poses, H, g, error, iteration counters) living in device memory.  The host only polls a "level done" flag.
// There is no CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>


#include <memory>
#include <new>

#include "../../include/rgbd360_hip.h"
#include "../../include/rgbd360_hip_diag.h"
#include "knobs.h"
#include "host_wait.h"
#include "dev_buf.h"
#include "dispatch.h"
#include "photo_icp_kernels.h"
#include "occlusion_kernels.h"
#include "pinhole_kernels.h"
#include "warp_images.h"
#include "f360_state.h"
#include "lm_host.h"

using namespace r360;

#include "level_geom.h"

namespace {

struct Level : LevelGeom {
    float *graySrc = nullptr, *depthSrc = nullptr, *grayTrg = nullptr, *depthTrg = nullptr;
    float4* srcRec = nullptr;
    DevBuf<float4> srcRecPin;        // pinhole LUT record of the source (built per alignment, RPI.h:4277-4300)
    F3 *trgP = nullptr, *trgD = nullptr;
    float *sinT = nullptr, *cosT = nullptr, *sinP = nullptr, *cosP = nullptr;
    float2 *tabT = nullptr, *tabP = nullptr;      // the same values interleaved {sin, cos}: one 8-byte load per pixel in the recompute form of the pass
    int libm = 0;                    // rgbd360_set_index_arithmetic: the warp in the reference's libm arithmetic
};

const float kIdentityPose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// contiguous, balanced spans of n_items over `world` ranks: the first n_items % world ranks get one more
void shard_range(int n_items, int rank, int world, int* lo, int* hi) {
    const int base = n_items / world, extra = n_items % world;
    *lo = rank * base + std::min(rank, extra);
    *hi = *lo + base + (rank < extra ? 1 : 0);
}

// job(0) .. job(n - 1) side by side: jobs 1 .. n-1 on a host thread each, job 0 -- and every job whose thread could not be started --
// on the caller's thread; returns when all have ended.  Never throws: no exception may cross the C boundary, so a job reports through
// what it captures (one return code per job; the callers take the first that is set).
template <class F>
void run_on_threads(int n, F job) {
    std::unique_ptr<std::thread[]> workers(n > 1 ? new (std::nothrow) std::thread[n - 1] : nullptr);
    for (int k = 1; k < n && workers; ++k) {
        try {
            workers[k - 1] = std::thread(job, k);
        } catch (const std::exception&) {      // left unstarted (not joinable)
        }
    }
    if (n > 0) job(0);
    for (int k = 1; k < n; ++k)
        if (!workers || !workers[k - 1].joinable()) job(k);
    for (int k = 1; k < n && workers; ++k)
        if (workers[k - 1].joinable()) workers[k - 1].join();
}

// one host frame (rows x cols, rgb8 + depth of depth_type) into packed device staging
hipError_t copy_frame_h2d(uint8_t* dst_rgb, void* dst_depth, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                          int depth_type, int rows, int cols, hipStream_t stream) {
    const size_t dpx = depth_type == 0 ? 2 : 4;
    const hipError_t e = hipMemcpy2DAsync(dst_rgb, (size_t)cols * 3, rgb, rgb_step, (size_t)cols * 3, rows, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    return hipMemcpy2DAsync(dst_depth, (size_t)cols * dpx, depth, depth_step, (size_t)cols * dpx, rows, hipMemcpyHostToDevice, stream);
}

// The upload ring of a frame sequence: host frames travel on a copy stream of their own through two staging slots, ahead of the
// alignment that converts them (up_ev[k]: slot k's upload has landed; conv_ev[k]: slot k has been consumed).  The one-pair context
// holds one (a frame per slot; slot 0 also serves the single-frame entries, which copy on the context's own stream and never open
// the ring) and so does the lock-step engine (a round of P frames per slot).  The slots grow only.
struct UploadRing {
    hipStream_t stream = nullptr;
    hipEvent_t up_ev[2] = {nullptr, nullptr}, conv_ev[2] = {nullptr, nullptr};
    DevBuf<uint8_t> rgb[2], depth[2];
    hipError_t open() {      // the copy stream and the four events, on first use
        if (stream) return hipSuccess;
        hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        for (int k = 0; k < 2 && e == hipSuccess; ++k) {
            e = hipEventCreateWithFlags(&up_ev[k], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&conv_ev[k], hipEventDisableTiming);
        }
        return e;
    }
    bool holds(size_t bytes_rgb, size_t bytes_depth, int slot) const { return rgb[slot].capacity() >= bytes_rgb && depth[slot].capacity() >= bytes_depth; }
    hipError_t ensure(size_t bytes_rgb, size_t bytes_depth, int slot) {
        const hipError_t e = rgb[slot].ensure(bytes_rgb);
        return e != hipSuccess ? e : depth[slot].ensure(bytes_depth);
    }
};
// drains and destroys the ring's stream and events; the staging goes with the ring's owner
void upload_ring_destroy(UploadRing& U) {
    if (U.stream) hipStreamSynchronize(U.stream);
    for (int k = 0; k < 2; ++k) {
        if (U.up_ev[k]) hipEventDestroy(U.up_ev[k]);
        if (U.conv_ev[k]) hipEventDestroy(U.conv_ev[k]);
    }
    if (U.stream) hipStreamDestroy(U.stream);
}

struct SeqEngine;      // sequence_engine.h

}  // namespace

struct rgbd360_ctx {
    rgbd360_params p;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<Level> levels;
    int rows = 0, cols = 0;
    bool have_src = false, have_trg = false;
    DevBuf<GNState> d_state;          // the CURRENT state buffer: every launch of the stream reads / updates this one ...
    DevBuf<GNState> d_state_alt;      // ... except the fused pass (k_eval_fs), which reads d_state, writes d_state_alt, after which the two swap
    PinnedBuf<GNState> h_state{hostwait::kPublishedFlags};
    hostwait::SpinTag tag;        // pinned sequence number the stream's last kernel stores (host_wait.h)
    int pend_rows_hint = r360::kPendingRows;      // upper bound of the partial rows the next fused launch finds pending (stage_pending)
    DevBuf<double> d_partials;        // partial rows of the last pass enqueued (current) ...
    DevBuf<double> d_partials_alt;    // ... and where a fused pass puts its rows while its blocks still read the previous table
    int max_blocks = 0;               // rows of a partial table = blocks of the largest level
    bool fused_occ = true;            // the occlusion-aware alignments on the fused schedule too (rgbd360_debug_set_schedule: {build, pass, k_solve} triples)
    bool seq_route_contexts = false;  // rgbd360_debug_set_sequence_route: every sequence over the per-context route (the occlusion-aware ones always are)
    int seq_route_cap = 0;            // ... with this many contexts at most (0: ctx_route_cap())
    bool fused_solve = true;          // single-pair schedule: solve in the prologue of the next pass (rgbd360_debug_set_schedule: {k_eval, k_solve} pairs)
    DevBuf<GnIO> d_gnio;
    // upload staging: slot 0 serves the single-frame entries (copies on `stream`); the sequence entry alternates both slots,
    // copying on the ring's stream one frame ahead of the alignment
    UploadRing ring;
    int poll_chunk = 3;           // {pass, solve} pairs per level enqueued ahead of the device
    int first_chunk_top = 8;      // ... and for the first visit of the coarsest level (cheap passes, most iterations)
    int chunk_level0 = 3;         // ... and for the finest level (most expensive passes; a second chunk costs a host round trip)
    bool adaptive_chunks = true;  // RGBD360_ADAPTIVE_CHUNKS=0: fixed chunks only (A/B)
    int hist_iters[8] = {-1, -1, -1, -1, -1, -1, -1, -1};      // accepted iterations per level of the previous alignment: sizes the first chunks of the next
    F360State* f360 = nullptr;        // the Frame360 stages' state (rgbd360_frame360.hip; created on the first Frame360 call, f360_state.h)
    float al_guess[16] = {0};     // alignment in flight (rgbd360_align360_begin / _finish)
    int al_method = 0;
    bool al_active = false;
    std::vector<rgbd360_ctx*> siblings;                // extra contexts of rgbd360_align360_batch's per-context route (owned)
    std::vector<SeqEngine*> engines;                   // lock-step sequence engines of rgbd360_align360_batch (owned)
    int al_occ = 0;
    float cam[4] = {0.f, 0.f, 0.f, 0.f};               // cameraMatrix(0,0), (1,1), (0,2), (1,2)   RPI.h:89, 254-257
    bool have_cam = false;
    float sal_thr = -1.f;                               // useSaliency(true): thresSaliency (RPI.h:217, 266); < 0 = off
    // pinhole occlusion passes: (target index, source index) pairs before / after the sort, the sort's scratch, one partial row per walk block
    DevBuf<unsigned> pin_keys, pin_vals;               // the pinhole occlusion passes: per source pixel its target + pass flags,
    DevBuf<int> pin_cnt;                               // per target pixel its arrivals (PinOccLists, pinhole_kernels.h: filled from these
    DevBuf<int4> pin_box;                              // three at launch)
    DevBuf<unsigned> pin_slots;
    DevBuf<double> pin_partials;
    DevBuf<int> occ_head;                              // occlusion modes: per-target lists of candidate runs (generation-tagged heads)
    DevBuf<int4> occ_nodes;                            // ... run nodes, indexed by the run's last source pixel
    DevBuf<unsigned char> occ_runinfo;                 // ... per source pixel: candidate / prefix maximum within its run / offset to the run's first pixel
    int occ_gen = 0;                                   // generation tag of the head entries (no memset between passes)
    // rgbd360_warp_images*: the winner plane and the four float planes the host entries stage their outputs in, sized for the finest level on
    // first use (wi_winner.capacity() pixels per plane) and freed with the levels
    DevBuf<int32_t> wi_winner;
    DevBuf<float> wi_stage;
    int max_eval_blocks = 256;    // grid cap of the fused pass (debug knob RGBD360_EVAL_BLOCKS, csrc/knobs.h)
    int index_libm = 0;           // rgbd360_set_index_arithmetic: 1 = the spherical warp in the reference's libm arithmetic
    DevBuf<unsigned char> arena;      // ONE allocation behind every per-level buffer of the context (planes, records, angle tables)
    std::string err;
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

int fail(rgbd360_ctx* ctx, int code, const char* msg) {
    ctx->err = msg;
    return code;
}

// what a change of the frame size frees (the occlusion set of the spherical path, the staging and the states stay, and grow only)
void free_levels(rgbd360_ctx* ctx) {
    ctx->pin_keys.release(); ctx->pin_vals.release(); ctx->pin_partials.release();
    ctx->pin_cnt.release(); ctx->pin_box.release(); ctx->pin_slots.release();
    ctx->wi_winner.release(); ctx->wi_stage.release();
    ctx->d_partials.release(); ctx->d_partials_alt.release();
    ctx->arena.release();
    ctx->levels.clear();      // (and every level's srcRecPin)
    ctx->rows = ctx->cols = 0;
    ctx->have_src = ctx->have_trg = false;
}

int ensure_levels(rgbd360_ctx* ctx, int rows, int cols) {
    if (ctx->rows == rows && ctx->cols == cols && !ctx->levels.empty()) return 0;
    if (const char* why = check_image_size(ctx->p, rows, cols)) return fail(ctx, -1, why);
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    free_levels(ctx);
    ctx->levels.resize(ctx->p.n_pyr);
    size_t arena_off = 0;
    {
        size_t total = 0;
        for (int l = 0, rr = rows, cc = cols; l < ctx->p.n_pyr; ++l, rr /= 2, cc /= 2) {
            const size_t n = (size_t)rr * cc;
            total += 4 * ((n * 4 + 255) & ~(size_t)255) + ((n * 16 + 255) & ~(size_t)255) + 2 * ((n * 12 + 255) & ~(size_t)255) +
                     2 * (((size_t)cc * 4 + 255) & ~(size_t)255) + 2 * (((size_t)rr * 4 + 255) & ~(size_t)255) +
                     (((size_t)cc * 8 + 255) & ~(size_t)255) + (((size_t)rr * 8 + 255) & ~(size_t)255);
        }
        HIPC(ctx, ctx->arena.ensure(total));
    }
    int r = rows, c = cols;
    int max_blocks = 0;
    for (int l = 0; l < ctx->p.n_pyr; ++l) {
        Level& L = ctx->levels[l];
        static_cast<LevelGeom&>(L) = level_geom(r, c, ctx->max_eval_blocks);
        // every buffer of every level out of ONE allocation (sized below on the first level's visit): a context is ~110 MB at
        // 2048 x 1024, and one large range keeps its pages' translations together (fewer, larger fragments) instead of scattering
        // ~45 small allocations over the address space
        auto take = [&](size_t bytes) -> void* {
            void* q = ctx->arena + arena_off;
            arena_off += (bytes + 255) & ~(size_t)255;
            return q;
        };
        const size_t nb = (size_t)L.n * sizeof(float);
        L.graySrc = (float*)take(nb); L.depthSrc = (float*)take(nb); L.grayTrg = (float*)take(nb); L.depthTrg = (float*)take(nb);
        L.srcRec = (float4*)take((size_t)L.n * sizeof(float4));
        L.trgP = (F3*)take((size_t)L.n * sizeof(F3));
        L.trgD = (F3*)take((size_t)L.n * sizeof(F3));
        L.sinT = (float*)take(c * sizeof(float)); L.cosT = (float*)take(c * sizeof(float));
        L.sinP = (float*)take(r * sizeof(float)); L.cosP = (float*)take(r * sizeof(float));
        L.tabT = (float2*)take(c * sizeof(float2)); L.tabP = (float2*)take(r * sizeof(float2));
        if (!L.tabT || !L.tabP) return fail(ctx, -103, "cannot allocate the pyramid levels");
        if (!L.graySrc || !L.depthSrc || !L.grayTrg || !L.depthTrg || !L.srcRec || !L.trgP || !L.trgD || !L.sinT || !L.cosT || !L.sinP || !L.cosP)
            return fail(ctx, -103, "cannot allocate the pyramid levels");
        HIPC(ctx, upload_angle_tables(angle_tables(L), L.sinT, L.cosT, L.sinP, L.cosP, L.tabT, L.tabP));
        L.libm = ctx->index_libm;
        if (L.nblocks > max_blocks) max_blocks = L.nblocks;
        r /= 2; c /= 2;
    }
    // at least the kPendingRows rows stage_pending always loads, + diagnostic rows; both tables are new here (free_levels released them)
    const size_t part_n = (size_t)(std::max((max_blocks + 31) / 32 * 32, kPendingRows) + 32 + max_blocks / 2 + 2) * kNumPartials;      // + the diagnostic rows of the stamp builds
    HIPC(ctx, ctx->d_partials.ensure(part_n));
    HIPC(ctx, ctx->d_partials_alt.ensure(part_n));
    HIPC(ctx, hipMemset(ctx->d_partials, 0, part_n * sizeof(double)));          // the fused pass loads max_blocks rows whatever the pending count
    HIPC(ctx, hipMemset(ctx->d_partials_alt, 0, part_n * sizeof(double)));
    ctx->max_blocks = max_blocks;
    ctx->rows = rows; ctx->cols = cols;
    return 0;
}

LevelDev level_dev(const Level& L) {
    LevelDev d;
    fill_level_dev(d, L);
    d.src = L.srcRec; d.trgP = L.trgP; d.trgD = L.trgD;
    d.depth_src = L.depthSrc; d.gray_src = L.graySrc; d.tabT = L.tabT; d.tabP = L.tabP;
    d.libm = L.libm;
    return d;
}
// Levels of this many pixels and more run the per-pixel pass in its recompute form (SRC 1, photo_icp_kernels.h: 8 B per source pixel less;
// a gain wherever the level is fed from HBM, a small loss on the latency-bound small levels).  Default: levels whose photo + depth
// working set (40 B/px) does not fit the 256 MiB Infinity Cache next to anything else, i.e. 4096 x 2048 and up; RGBD360_RECOMPUTE_MIN_PX
// moves the bound (0 = every level, for A/B runs and tests).
int recompute_min_px() {
    static const int v = [] { const char* e = knobs::product("RGBD360_RECOMPUTE_MIN_PX"); return e ? atoi(e) : 4 * 1024 * 1024; }();
    return v;
}

EvalConsts eval_consts(const rgbd360_params& p) {
    EvalConsts e;
    e.sigma_photo = p.sigma_photo; e.sigma_depth = p.sigma_depth;
    e.thr_photo = p.thres_sal_photo; e.thr_depth = p.thres_sal_depth;
    e.sigma_photo_inv_f = 1. / p.sigma_photo;
    e.sigma_photo_inv_d = 1. / p.sigma_photo;
    return e;
}

dim3 grid2d(int rows, int cols, int bx = 256) { return dim3((cols + bx - 1) / bx, rows, 1); }

int occ_ensure(rgbd360_ctx* ctx) {
    const size_t n = ctx->levels.empty() ? 0 : (size_t)ctx->levels[0].n;
    if (n > 0 && ctx->occ_head.capacity() >= n && ctx->occ_nodes.capacity() >= n && ctx->occ_runinfo.capacity() >= n) return 0;
    // the three grow together (and survive a smaller frame size); the heads of a set that grew start empty
    HIPC(ctx, ctx->occ_head.ensure(n));
    HIPC(ctx, ctx->occ_nodes.ensure(n));
    HIPC(ctx, ctx->occ_runinfo.ensure(n));
    HIPC(ctx, hipMemsetAsync(ctx->occ_head, 0, ctx->occ_head.capacity() * sizeof(int), ctx->stream));      // generation 0 = empty; the passes count from 1
    ctx->occ_gen = 0;
    return 0;
}

// The head entries of the occlusion lists carry their pass's generation (1..kOccGenMax) in their top byte: one memset per kOccGenMax
// passes instead of one per pass.  Returns the generation of the pass about to be enqueued.
int occ_next_gen(rgbd360_ctx* ctx) {
    if (++ctx->occ_gen > kOccGenMax) {
        hipMemsetAsync(ctx->occ_head, 0, ctx->occ_head.capacity() * sizeof(int), ctx->stream);
        ctx->occ_gen = 1;
    }
    return ctx->occ_gen;
}

FsInit fs_init(const float* init_pose) {
    FsInit init;
    init.on = init_pose ? 1 : 0;
    if (init_pose) memcpy(init.pose.v, init_pose, sizeof(init.pose.v));
    else memset(init.pose.v, 0, sizeof(init.pose.v));
    return init;
}

// the occlusion-aware pass over the run lists of generation `gen`, gate and pose from `st`
void launch_eval_occ(rgbd360_ctx* ctx, int level, int method, int occ, const LevelDev& lv, const EvalConsts& ec, const GNState* st,
                     double* partials, int gen) {
    const Level& L = ctx->levels[level];
    const dim3 g(L.nblocks), b(kEvalThreads);
    with_choice<1, 2>(occ != 1, [&](auto O) {
        with_method(method, [&](auto M) {
            hipLaunchKernelGGL((k_eval_occ<M, O>), g, b, 0, ctx->stream, lv, ec, st, partials, L.chunk, level, gen, ctx->occ_head,
                               (const int4*)ctx->occ_nodes, (const unsigned char*)ctx->occ_runinfo);
        });
    });
}

void launch_eval(rgbd360_ctx* ctx, int level, int method, bool hg, int occ = 0) {
    const Level& L = ctx->levels[level];
    LevelDev lv = level_dev(L);
    lv.min_depth = ctx->p.min_depth; lv.max_depth = ctx->p.max_depth;
    const EvalConsts ec = eval_consts(ctx->p);
    dim3 g(L.nblocks), b(kEvalThreads);
    if (occ != 0) {
        // per-target lists of candidate RUNS at the pose under evaluation, then the occlusion-aware fused pass, which decides per pixel
        const int gen = occ_next_gen(ctx);
        const dim3 gb((L.n + 255) / 256), bb(256);
        with_choice<1, 2>(occ != 1, [&](auto O) {
            hipLaunchKernelGGL((k_occ_build<O>), gb, bb, 0, ctx->stream, lv, ctx->d_state, level, gen, ctx->occ_head, ctx->occ_nodes, ctx->occ_runinfo);
        });
        launch_eval_occ(ctx, level, method, occ, lv, ec, ctx->d_state, ctx->d_partials, gen);
        return;
    }
    auto launch = [&](auto M, auto HG, auto S) {
        hipLaunchKernelGGL((k_eval<M, HG, S>), g, b, 0, ctx->stream, ctx->d_state, lv.src, lv.n, L.chunk, level, L.nblocks, ctx->d_partials, lv, ec);
    };
    // (the error-only pass exists in the record form alone)
    if (!hg) with_method(method, [&](auto M) { launch(M, std::false_type{}, std::integral_constant<int, 0>{}); });
    else with_choice<0, 1>(L.n >= recompute_min_px(), [&](auto S) { with_method(method, [&](auto M) { launch(M, std::true_type{}, S); }); });
}

// publish: the solve also writes the state into ctx->h_state and bumps the context's host tag (hostwait::wait picks it up)
// cfg_in (may be NULL): termination settings and error form of the solve instead of the context's (rgbd360_debug_solve_state)
void launch_solve(rgbd360_ctx* ctx, int level, int mode, int forced, int occ = 0, bool publish = false, const SolveCfg* cfg_in = nullptr) {
    const Level& L = ctx->levels[level];
    SolveCfg cfg;
    if (cfg_in) cfg = *cfg_in;
    cfg.level = level; cfg.mode = mode; cfg.n_pixels = L.n;
    if (!cfg_in) {
        cfg.forced = forced; cfg.max_iters = ctx->p.max_iters; cfg.occ = occ;
        cfg.tol_residual = ctx->p.tol_residual; cfg.tol_update = ctx->p.tol_update;
    }
    if (publish) {
        cfg.host_state = ctx->h_state;
        cfg.host_tag = ctx->tag.h;
        cfg.host_seq = ++ctx->tag.seq;
    }
    hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, ctx->stream, ctx->d_state, ctx->d_partials, L.nblocks, cfg);
}

// Fused-solve schedule (k_eval_fs, photo_icp_kernels.h): the launch solves the pass the previous launch left pending and runs the
// next pass; state and partial table ping-pong, the host's "current" pointers follow the stream order.
bool fused_ok(const rgbd360_ctx* ctx, int occ) {
    return ctx->fused_solve && (occ == 0 || ctx->fused_occ) && ctx->max_blocks <= kMaxPendingRows;
}
SolveCfg fused_cfg(const rgbd360_ctx* ctx, int forced, int occ = 0) {
    SolveCfg cfg;
    cfg.level = -1; cfg.n_pixels = 0;       // taken from the state (level_active / pend_npix of the pending pass)
    cfg.mode = 0; cfg.forced = forced; cfg.max_iters = ctx->p.max_iters; cfg.occ = occ;
    cfg.tol_residual = ctx->p.tol_residual; cfg.tol_update = ctx->p.tol_update;
    return cfg;
}
// init_pose != nullptr: the launch starts the schedule itself at that pose (no k_level_init in front of it); cfg_in (may be NULL):
// the solve's settings instead of fused_cfg(ctx, forced) (rgbd360_debug_solve_state)
void launch_eval_fused(rgbd360_ctx* ctx, int level, int method, int forced, const float* init_pose = nullptr, const SolveCfg* cfg_in = nullptr) {
    const FsInit init = fs_init(init_pose);
    const Level& L = ctx->levels[level];
    LevelDev lv = level_dev(L);
    lv.min_depth = ctx->p.min_depth; lv.max_depth = ctx->p.max_depth;
    const EvalConsts ec = eval_consts(ctx->p);
    const SolveCfg cfg = cfg_in ? *cfg_in : fused_cfg(ctx, forced);
    dim3 g(L.nblocks), b(kEvalThreads);
    with_choice<0, 1>(L.n >= recompute_min_px(), [&](auto S) {
        with_method(method, [&](auto M) {
            hipLaunchKernelGGL((k_eval_fs<M, S>), g, b, 0, ctx->stream, (const GNState*)ctx->d_state, ctx->d_state_alt, (const double*)ctx->d_partials,
                               ctx->d_partials_alt, lv.src, lv.n, L.chunk, level, L.nblocks, ctx->pend_rows_hint, lv, ec, cfg, init);
        });
    });
    ctx->pend_rows_hint = L.nblocks;             // what this launch can leave pending bounds what the next one has to load
    std::swap(ctx->d_state, ctx->d_state_alt);
    std::swap(ctx->d_partials, ctx->d_partials_alt);
}
// The occlusion-aware iteration of the fused schedule: k_occ_build_fs (solve of the pending pass + run lists at the new pose; writes
// the new state) and k_eval_occ (gate and pose from that state; leaves its rows pending) -- two launches instead of three.
void launch_occ_fused(rgbd360_ctx* ctx, int level, int method, int occ, int forced, const float* init_pose = nullptr) {
    const FsInit init = fs_init(init_pose);
    const Level& L = ctx->levels[level];
    LevelDev lv = level_dev(L);
    lv.min_depth = ctx->p.min_depth; lv.max_depth = ctx->p.max_depth;
    const EvalConsts ec = eval_consts(ctx->p);
    const SolveCfg cfg = fused_cfg(ctx, forced, occ);
    const int gen = occ_next_gen(ctx);
    dim3 g(L.nblocks), b(kEvalThreads);
    with_choice<1, 2>(occ != 1, [&](auto O) {
        hipLaunchKernelGGL((k_occ_build_fs<O>), g, b, 0, ctx->stream, (const GNState*)ctx->d_state, ctx->d_state_alt, (const double*)ctx->d_partials,
                           L.chunk, level, L.nblocks, ctx->pend_rows_hint, lv, cfg, init, gen, ctx->occ_head, ctx->occ_nodes, ctx->occ_runinfo);
    });
    launch_eval_occ(ctx, level, method, occ, lv, ec, ctx->d_state_alt, ctx->d_partials_alt, gen);
    ctx->pend_rows_hint = L.nblocks;
    std::swap(ctx->d_state, ctx->d_state_alt);
    std::swap(ctx->d_partials, ctx->d_partials_alt);
}
// the tail of a fused schedule: solves what the last pass left pending (nothing, if that launch was a no-op) and publishes
void launch_solve_pending(rgbd360_ctx* ctx, int forced, bool publish, int occ = 0) {
    SolveCfg cfg = fused_cfg(ctx, forced, occ);
    if (publish) {
        cfg.host_state = ctx->h_state;
        cfg.host_tag = ctx->tag.h;
        cfg.host_seq = ++ctx->tag.seq;
    }
    hipLaunchKernelGGL(k_solve_pending, dim3(1), dim3(kSolveThreads), 0, ctx->stream, ctx->d_state, (const double*)ctx->d_partials, ctx->pend_rows_hint, cfg);
}

void launch_level_init(rgbd360_ctx* ctx, int level, const float* pose, int reset_all) {
    Pose16 P;
    if (pose) memcpy(P.v, pose, sizeof(P.v));
    else memset(P.v, 0, sizeof(P.v));
    hipLaunchKernelGGL(k_level_init, dim3(1), dim3(64), 0, ctx->stream, ctx->d_state, P, pose ? 1 : 0, reset_all, level);
    ctx->pend_rows_hint = kPendingRows;
}

// the device state into ctx->h_state with memcpy + stream synchronise: for callers that read HIP events afterwards (an event the
// runtime has not yet seen complete costs hipEventElapsedTime a blocking wait of its own: +30 us per call measured)
int read_state_sync(rgbd360_ctx* ctx) {
    HIPC(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state, sizeof(GNState), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
// the device state into ctx->h_state, and wait for it: publishing kernel + host spin (host_wait.h), not memcpy + stream synchronise
int read_state(rgbd360_ctx* ctx) {
    static_assert(sizeof(GNState) % 4 == 0, "published word by word");
    HIPC(ctx, hostwait::publish_and_wait(ctx->tag, ctx->stream, ctx->d_state, ctx->h_state, sizeof(GNState)));
    return 0;
}

int check_args(rgbd360_ctx* ctx, int level, int method) {
    if (!ctx) return -1;
    if (!ctx->have_src || !ctx->have_trg) return fail(ctx, -2, "set_target and set_source must be called first");
    if (level < 0 || level >= (int)ctx->levels.size()) return fail(ctx, -3, "bad pyramid level");
    if (method < 0 || method > 2) return fail(ctx, -4, "bad method");
    return 0;
}

// every gradient record of the target frame (all levels x {intensity, depth}) in one launch
void launch_gradient_recs(rgbd360_ctx* ctx) {
    GradJobs jobs;
    int nb = 0, n = 0;
    for (int l = 0; l < ctx->p.n_pyr; ++l) {
        const Level& L = ctx->levels[l];
        const int seam = ctx->p.mask_seams ? L.cols / 8 : 0;
        for (int k = 0; k < 2; ++k) {
            jobs.src[n] = k == 0 ? L.grayTrg : L.depthTrg;
            jobs.rec[n] = k == 0 ? L.trgP : L.trgD;
            jobs.rows[n] = L.rows; jobs.cols[n] = L.cols; jobs.seam[n] = seam;
            jobs.first_block[n] = nb;
            nb += (L.n + 255) / 256;
            ++n;
        }
    }
    jobs.first_block[n] = nb;
    jobs.n = n;
    hipLaunchKernelGGL(k_gradient_rec_multi, dim3(nb), dim3(256), 0, ctx->stream, jobs);
}

// every source record (LUT point + intensity) of the source frame in one launch
void launch_src_recs(rgbd360_ctx* ctx) {
    SrcJobs jobs;
    int nb = 0, n = 0;
    for (int l = 0; l < ctx->p.n_pyr; ++l) {
        const Level& L = ctx->levels[l];
        jobs.depth[n] = L.depthSrc; jobs.gray[n] = L.graySrc;
        jobs.sin_theta[n] = L.sinT; jobs.cos_theta[n] = L.cosT; jobs.sin_phi[n] = L.sinP; jobs.cos_phi[n] = L.cosP;
        jobs.rec[n] = L.srcRec;
        jobs.rows[n] = L.rows; jobs.cols[n] = L.cols;
        jobs.first_block[n] = nb;
        nb += (L.n + 255) / 256;
        ++n;
    }
    jobs.first_block[n] = nb;
    jobs.n = n;
    jobs.min_depth = ctx->p.min_depth; jobs.max_depth = ctx->p.max_depth;
    hipLaunchKernelGGL(k_src_rec_multi, dim3(nb), dim3(256), 0, ctx->stream, jobs);
}

// Sequence path: copy one host frame into staging slot `slot` on the context's upload stream, ahead of its use.
static int upload_stage(rgbd360_ctx* ctx, int slot, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t d_step,
                        int depth_type, int rows, int cols) {
    const size_t dpx = depth_type == 0 ? 2 : 4;
    UploadRing& U = ctx->ring;
    HIPC(ctx, U.open());
    HIPC(ctx, U.ensure((size_t)rows * cols * 3, (size_t)rows * cols * dpx, slot));
    HIPC(ctx, hipStreamWaitEvent(U.stream, U.conv_ev[slot], 0));      // the slot's previous frame has been converted
    HIPC(ctx, copy_frame_h2d(U.rgb[slot], U.depth[slot], rgb, rgb_step, depth, d_step, depth_type, rows, cols, U.stream));
    HIPC(ctx, hipEventRecord(U.up_ev[slot], U.stream));
    return 0;
}

// staged_slot >= 0: the frame was put into that staging slot by upload_stage (rgb / depth are then unused).
int set_frame(rgbd360_ctx* ctx, bool target, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t d_step,
              int depth_type, int rows, int cols, bool on_device, bool wait_for_upload = true, int staged_slot = -1) {
    if (!ctx) return -1;
    if (staged_slot < 0 && (!rgb || !depth)) return fail(ctx, -1, "null image pointer");
    if (depth_type != 0 && depth_type != 1) return fail(ctx, -1, "depth_type must be 0 (u16 mm) or 1 (f32 m)");
    if (ctx->levels.size() && (rows != ctx->rows || cols != ctx->cols) && (target ? ctx->have_src : ctx->have_trg)) {
        // the other frame has different dimensions: both must be set again (the reference would read out of bounds)
        if (target) ctx->have_src = false; else ctx->have_trg = false;
    }
    int rc = ensure_levels(ctx, rows, cols);
    if (rc) return rc;
    const size_t dpx = depth_type == 0 ? 2 : 4;
    const uint8_t* d_rgb = rgb;
    const void* d_depth = depth;
    size_t s_rgb = rgb_step, s_depth = d_step;
    if (staged_slot >= 0) {
        HIPC(ctx, hipStreamWaitEvent(ctx->stream, ctx->ring.up_ev[staged_slot], 0));
        d_rgb = ctx->ring.rgb[staged_slot]; d_depth = ctx->ring.depth[staged_slot];
        s_rgb = (size_t)cols * 3; s_depth = (size_t)cols * dpx;
    } else if (!on_device) {
        HIPC(ctx, ctx->ring.ensure((size_t)rows * cols * 3, (size_t)rows * cols * dpx, 0));
        HIPC(ctx, copy_frame_h2d(ctx->ring.rgb[0], ctx->ring.depth[0], rgb, rgb_step, depth, d_step, depth_type, rows, cols, ctx->stream));
        d_rgb = ctx->ring.rgb[0]; d_depth = ctx->ring.depth[0];
        s_rgb = (size_t)cols * 3; s_depth = (size_t)cols * dpx;
    }
    Level& L0 = ctx->levels[0];
    float* gray0 = target ? L0.grayTrg : L0.graySrc;
    float* dep0 = target ? L0.depthTrg : L0.depthSrc;
    {
        dim3 g = grid2d(rows, (cols + 3) / 4);
        g.z = 2;                                        // colour -> intensity and depth -> metres in one launch
        hipLaunchKernelGGL(k_convert_pair, g, dim3(256), 0, ctx->stream, d_rgb, s_rgb, d_depth, s_depth, depth_type, rows, cols, gray0, dep0);
        if (staged_slot >= 0) HIPC(ctx, hipEventRecord(ctx->ring.conv_ev[staged_slot], ctx->stream));
    }
    for (int l = 1; l < ctx->p.n_pyr; ++l) {
        Level &P = ctx->levels[l - 1], &C = ctx->levels[l];
        dim3 g = grid2d(C.rows, C.cols);
        g.z = 2;                                        // intensity and depth step in one launch
        hipLaunchKernelGGL(k_pyrdown_pair, g, dim3(256), 0, ctx->stream, target ? P.grayTrg : P.graySrc,
                           target ? P.depthTrg : P.depthSrc, P.rows, P.cols, target ? C.grayTrg : C.graySrc,
                           target ? C.depthTrg : C.depthSrc, C.rows, C.cols, ctx->p.min_depth, ctx->p.max_depth);
    }
    if (target) launch_gradient_recs(ctx);
    else launch_src_recs(ctx);
    HIPC(ctx, hipGetLastError());
    // host buffers may be reused by the caller once a set_* call returns; the sequence entry owns them until it returns
    if (!on_device && staged_slot < 0 && wait_for_upload) HIPC(ctx, hipStreamSynchronize(ctx->stream));
    if (target) ctx->have_trg = true; else ctx->have_src = true;
    return 0;
}

}  // namespace

#include "sequence_engine.h"
#include "rig_dense.h"

extern "C" {

void rgbd360_default_params(rgbd360_params* p) {
    p->n_pyr = 4;
    p->min_depth = 0.3f;
    p->max_depth = 6.0f;
    p->sigma_photo = (float)(6. / 255);
    p->sigma_depth = (float)0.2;
    p->thres_sal_photo = 0.01f;
    p->thres_sal_depth = 0.01f;
    p->max_iters = 10;
    p->tol_residual = 1e-3f;
    p->tol_update = 1e-4f;
    p->mask_seams = 1;
    p->device = 0;
}

int rgbd360_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rgbd360_create(const rgbd360_params* p, rgbd360_ctx** out) {
    if (!p || !out) return -1;
    *out = nullptr;
    if (p->n_pyr < 1 || p->n_pyr > 8) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -100;   // no HIP device: no fallback
    if (p->device < 0 || p->device >= ndev) return -101;
    if (hipSetDevice(p->device) != hipSuccess) return -102;
    rgbd360_ctx* ctx = new rgbd360_ctx();
    ctx->p = *p;
    if (const char* e = knobs::debug("RGBD360_EVAL_BLOCKS")) {
        const int v = atoi(e);
        if (v >= 8 && v <= 8192) ctx->max_eval_blocks = v;
    }
    if (const char* e = knobs::debug("RGBD360_POLL_CHUNK")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 16) ctx->poll_chunk = v;
    }
    if (const char* e = knobs::debug("RGBD360_FIRST_CHUNK")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 16) ctx->first_chunk_top = v;
    }
    if (const char* e = knobs::debug("RGBD360_L0_CHUNK")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 16) ctx->chunk_level0 = v;
    }
    if (const char* e = knobs::debug("RGBD360_ADAPTIVE_CHUNKS")) {
        ctx->adaptive_chunks = atoi(e) != 0;
    }
    if (const char* e = knobs::debug("RGBD360_FUSED_SOLVE")) {
        ctx->fused_solve = atoi(e) != 0;
    }
    if (const char* e = knobs::debug("RGBD360_FUSED_OCC")) {
        ctx->fused_occ = atoi(e) != 0;
    }
    bool ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&ctx->ev0) == hipSuccess && hipEventCreate(&ctx->ev1) == hipSuccess &&
              ctx->d_state.ensure(1) == hipSuccess &&
              hipMemset(ctx->d_state, 0, sizeof(GNState)) == hipSuccess &&
              ctx->d_state_alt.ensure(1) == hipSuccess &&
              hipMemset(ctx->d_state_alt, 0, sizeof(GNState)) == hipSuccess &&
              ctx->d_gnio.ensure(1) == hipSuccess &&
              ctx->h_state.ensure(1) == hipSuccess &&
              hostwait::spin_tag_init(&ctx->tag) == hipSuccess;
    if (!ok) {
        rgbd360_destroy(ctx);
        return -103;
    }
    *out = ctx;
    return 0;
}

void rgbd360_destroy(rgbd360_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->p.device);
    for (rgbd360_ctx* sib : ctx->siblings) rgbd360_destroy(sib);
    ctx->siblings.clear();
    for (SeqEngine* e : ctx->engines) seq_free(e);
    ctx->engines.clear();
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    upload_ring_destroy(ctx->ring);
    if (ctx->f360) f360_state_destroy(ctx->f360);
    hostwait::spin_tag_free(&ctx->tag);
    if (ctx->ev0) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) hipEventDestroy(ctx->ev1);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;      // every buffer the context owns, with its device current and nothing of its streams left
}

const char* rgbd360_last_error(rgbd360_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
void* rgbd360_stream(rgbd360_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
int rgbd360_sync(rgbd360_ctx* ctx) {
    if (!ctx) return -1;
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int rgbd360_set_target(rgbd360_ctx* ctx, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                       int depth_type, int rows, int cols) {
    if (ctx) hipSetDevice(ctx->p.device);
    return set_frame(ctx, true, rgb, rgb_step, depth, depth_step, depth_type, rows, cols, false);
}
int rgbd360_set_source(rgbd360_ctx* ctx, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                       int depth_type, int rows, int cols) {
    if (ctx) hipSetDevice(ctx->p.device);
    return set_frame(ctx, false, rgb, rgb_step, depth, depth_step, depth_type, rows, cols, false);
}
int rgbd360_set_target_dev(rgbd360_ctx* ctx, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                           int depth_type, int rows, int cols) {
    if (ctx) hipSetDevice(ctx->p.device);
    return set_frame(ctx, true, rgb, rgb_step, depth, depth_step, depth_type, rows, cols, true);
}
int rgbd360_set_source_dev(rgbd360_ctx* ctx, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                           int depth_type, int rows, int cols) {
    if (ctx) hipSetDevice(ctx->p.device);
    return set_frame(ctx, false, rgb, rgb_step, depth, depth_step, depth_type, rows, cols, true);
}

int rgbd360_promote_source_to_target(rgbd360_ctx* ctx) {
    if (!ctx) return -1;
    if (!ctx->have_src) return fail(ctx, -2, "no source frame to promote");
    hipSetDevice(ctx->p.device);
    for (Level& L : ctx->levels) {
        std::swap(L.graySrc, L.grayTrg);
        std::swap(L.depthSrc, L.depthTrg);
    }
    launch_gradient_recs(ctx);
    HIPC(ctx, hipGetLastError());
    ctx->have_trg = true;
    ctx->have_src = false;
    return 0;
}

// The whole coarse-to-fine schedule is enqueued ahead of the device: every launch carries its level and turns into a
// no-op unless that level is the active, unfinished one (k_level_init of level l only fires once level l+1 has
// finished).  In the common case -- each level converges within its first chunk -- the host synchronises ONCE per
// alignment; a level that needs more passes gets another chunk, followed again by the finer levels.
// The last solve launch of the schedule publishes the state to the host (SolveCfg::host_state): no copy launch behind it.
static void enqueue_schedule(rgbd360_ctx* ctx, int pending, bool pending_started) {
    const int top = ctx->p.n_pyr - 1;
    for (int level = pending; level >= 0; --level) {
        const bool fused = fused_ok(ctx, ctx->al_occ);
        const bool start = level == top && !pending_started;      // the finer levels are entered by the solve itself when a level finishes
        if (start && !fused) launch_level_init(ctx, level, ctx->al_guess, 1);      // (the fused schedule's first launch initialises the state itself)
        int n_pairs = (level == top && !pending_started) ? ctx->first_chunk_top : (level == 0 ? ctx->chunk_level0 : ctx->poll_chunk);
        // Consecutive alignments of a sequence take much the same number of iterations per level: the first visit of a level is
        // given what the previous alignment needed there (its accepted iterations + the first pass + the pass that ends the level: one
        // launch fewer costs a host round trip per level, 173 -> 293 us measured)
        // instead of the fixed chunk -- fewer no-op launches on the coarse levels (~3 us each), no second round trip on level 0.
        if (ctx->adaptive_chunks && !(level == pending && pending_started) && ctx->hist_iters[level & 7] >= 0)
            n_pairs = std::min(std::max(ctx->hist_iters[level & 7] + 2, 2), 12);
        if (fused) {
            // one launch per iteration: n_pairs passes, each carrying the solve of the one before it; the solve of the chunk's last
            // pass rides in the next level's first launch, the schedule's very last one in a one-block launch that publishes
            for (int k = 0; k < n_pairs; ++k) {
                const float* init_pose = start && k == 0 ? ctx->al_guess : nullptr;
                if (ctx->al_occ) launch_occ_fused(ctx, level, ctx->al_method, ctx->al_occ, 0, init_pose);
                else launch_eval_fused(ctx, level, ctx->al_method, 0, init_pose);
            }
            if (level == 0) launch_solve_pending(ctx, 0, /*publish=*/true, ctx->al_occ);
            continue;
        }
        for (int k = 0; k < n_pairs; ++k) {
            launch_eval(ctx, level, ctx->al_method, true, ctx->al_occ);
            launch_solve(ctx, level, 0, 0, ctx->al_occ, /*publish=*/level == 0 && k == n_pairs - 1);
        }
    }
}

int rgbd360_align360_begin(rgbd360_ctx* ctx, const float guess[16], int method, int occlusion) {
    int rc = check_args(ctx, 0, method);
    if (rc) return rc;
    if (occlusion < 0 || occlusion > 2) return fail(ctx, -5, "occlusion must be 0, 1 or 2");
    if (!guess) return fail(ctx, -1, "null pose pointer");
    hipSetDevice(ctx->p.device);
    if (occlusion != 0 && (rc = occ_ensure(ctx)) != 0) return rc;
    ctx->al_occ = occlusion;
    memcpy(ctx->al_guess, guess, sizeof(ctx->al_guess));
    ctx->al_method = method;
    ctx->al_active = true;
    enqueue_schedule(ctx, ctx->p.n_pyr - 1, false);      // (its last solve publishes the state and bumps the tag)
    HIPC(ctx, hipGetLastError());
    return 0;
}

int rgbd360_align360_finish(rgbd360_ctx* ctx, float pose_out[16], rgbd360_result* res) {
    if (!ctx || !pose_out) return -1;
    if (!ctx->al_active) return fail(ctx, -2, "rgbd360_align360_begin was not called");
    hipSetDevice(ctx->p.device);
    ctx->al_active = false;
    for (int round = 0;; ++round) {
        HIPC(ctx, hostwait::wait(ctx->tag, ctx->stream));      // the state published by begin / the previous round has landed
        const GNState& S = *ctx->h_state;
        if (S.status != 0) break;
        if (S.level_active == 0 && S.done) break;
        if (S.done) return fail(ctx, -6, "alignment schedule stalled between levels");
        if (round > (ctx->p.max_iters + 4) * ctx->p.n_pyr) return fail(ctx, -6, "alignment loop did not terminate");
        enqueue_schedule(ctx, S.level_active, true);         // the stalled level gets another chunk, then the finer ones
        HIPC(ctx, hipGetLastError());
    }
    rgbd360_result R;
    result_from_state(*ctx->h_state, ctx->p.n_pyr, ctx->al_occ, pose_out, &R);
    for (int l = 0; l < 8; ++l) ctx->hist_iters[l] = (R.status == 0 && l < ctx->p.n_pyr) ? ctx->h_state[0].iters[l] : -1;
    if (res) *res = R;
    return R.status;
}

int rgbd360_align360(rgbd360_ctx* ctx, const float guess[16], int method, int occlusion, float pose_out[16],
                     rgbd360_result* res) {
    if (!pose_out) return ctx ? fail(ctx, -1, "null pose pointer") : -1;
    const int rc = rgbd360_align360_begin(ctx, guess, method, occlusion);
    if (rc) return rc;
    return rgbd360_align360_finish(ctx, pose_out, res);
}

// ---------------------------------------------------------------------------------------------------------
// A sequence of consecutive pairs on one GPU (SURVEY.md 8b rgbd360_align360_batch, 8e): pair j = (frame j, frame j+1),
// frame j = target, frame j+1 = source, as OdometryRGBD360.cpp:141-297 walks a sequence.  The pairs are cut into
// n_inflight contiguous sub-chunks, one context (own HIP stream) each; inside a sub-chunk frame j+1 is uploaded once and
// promoted from source to target; in every step all live contexts are enqueued before any is waited for.
// ---------------------------------------------------------------------------------------------------------
static int align360_batch_threads(rgbd360_ctx* ctx, int n_frames, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                               size_t depth_step, int depth_type, int rows, int cols, const float guess[16], int method,
                               int occlusion, int n_inflight, float* poses_out, rgbd360_result* results_out, bool on_device) {
    if (!ctx) return -1;
    if (!rgb || !depth || !poses_out) return fail(ctx, -1, "null pointer");
    if (n_frames < 1) return fail(ctx, -1, "n_frames must be >= 1");
    if (n_inflight < 1 || n_inflight > 16) return fail(ctx, -1, "n_inflight must be in 1..16");
    if (method < 0 || method > 2) return fail(ctx, -4, "bad method");
    if (occlusion < 0 || occlusion > 2) return fail(ctx, -5, "occlusion must be 0, 1 or 2");
    const int n = n_frames - 1;
    if (n == 0) return 0;
    for (int k = 0; k < n_frames; ++k)
        if (!rgb[k] || !depth[k]) return fail(ctx, -1, "null frame pointer");
    const float* g = guess ? guess : kIdentityPose;
    const int k_ctx = std::min(n_inflight, n);
    while ((int)ctx->siblings.size() < k_ctx - 1) {
        rgbd360_ctx* sib = nullptr;
        const int rc = rgbd360_create(&ctx->p, &sib);
        if (rc) return fail(ctx, rc, "cannot create a sibling context");
        ctx->siblings.push_back(sib);
    }
    std::vector<rgbd360_ctx*> cs(k_ctx);
    cs[0] = ctx;
    for (int c = 1; c < k_ctx; ++c) {
        cs[c] = ctx->siblings[c - 1];
        if (cs[c]->index_libm != ctx->index_libm) rgbd360_set_index_arithmetic(cs[c], ctx->index_libm);      // the siblings follow the context's warp arithmetic
    }
    // contiguous balanced spans [a, b) of pairs per context
    std::vector<int> a(k_ctx), b(k_ctx);
    for (int c = 0; c < k_ctx; ++c) shard_range(n, c, k_ctx, &a[c], &b[c]);
    // One host thread per sub-chunk: a 4-level alignment is ~65 dependent launches, so a single enqueueing thread (≈2.7 us
    // per launch) caps a GPU at ≈5.7 k alignments/s however many contexts are in flight.  The sub-chunks share nothing
    // (own context, stream, buffers, error string; disjoint output slots), so each walks its pairs on its own thread:
    // upload (asynchronous, waited for only by the pair's own finish) -> frame set-up -> schedule -> finish -> promote.
    std::vector<int> rcs(k_ctx, 0);
    auto run_chunk = [&](int c) {
        rgbd360_ctx* cc = cs[c];
        hipSetDevice(cc->p.device);
        int rc = 0;
        if (on_device) {
            rc = set_frame(cc, true, rgb[a[c]], rgb_step, depth[a[c]], depth_step, depth_type, rows, cols, true);
        } else {        // frame f of this sub-chunk travels through staging slot (f - a) & 1, one frame ahead of the alignment
            rc = upload_stage(cc, 0, rgb[a[c]], rgb_step, depth[a[c]], depth_step, depth_type, rows, cols);
            if (!rc) rc = upload_stage(cc, 1, rgb[a[c] + 1], rgb_step, depth[a[c] + 1], depth_step, depth_type, rows, cols);
            if (!rc) rc = set_frame(cc, true, nullptr, 0, nullptr, 0, depth_type, rows, cols, false, false, 0);
        }
        for (int j = a[c]; !rc && j < b[c]; ++j) {
            if (on_device) {
                rc = set_frame(cc, false, rgb[j + 1], rgb_step, depth[j + 1], depth_step, depth_type, rows, cols, true);
            } else {
                rc = set_frame(cc, false, nullptr, 0, nullptr, 0, depth_type, rows, cols, false, false, (j + 1 - a[c]) & 1);
                if (!rc && j + 2 <= b[c])       // the next source frame is copied while this pair is being aligned
                    rc = upload_stage(cc, (j + 2 - a[c]) & 1, rgb[j + 2], rgb_step, depth[j + 2], depth_step, depth_type, rows, cols);
            }
            if (!rc) rc = rgbd360_align360_begin(cc, g, method, occlusion);
            if (rc) break;
            rgbd360_result R;
            rc = rgbd360_align360_finish(cc, poses_out + (size_t)16 * j, &R);      // >= 0: the pair's outcome, kept in R.status
            if (results_out) results_out[j] = R;
            if (rc >= 0) rc = j + 1 < b[c] ? std::min(0, rgbd360_promote_source_to_target(cc)) : 0;
        }
        if (cc->ring.stream) hipStreamSynchronize(cc->ring.stream);      // no upload may outlive the caller's buffers
        if (rc) hipStreamSynchronize(cc->stream);
        rcs[c] = rc;
    };
    run_on_threads(k_ctx, run_chunk);
    for (int c = 0; c < k_ctx; ++c)
        if (rcs[c]) return cs[c] == ctx ? rcs[c] : fail(ctx, rcs[c], cs[c]->err.c_str());
    return 0;
}

// The lock-step route (sequence_engine.h): n_inflight = pairs in flight = slots, spread over one or two engines (own stream and host
// thread each: while one engine waits for its round's states or enqueues, the other's kernels fill the device).
// Contexts of the per-context route.  The device runs four hardware queues side by side; a fifth busy queue makes the command
// processor time-slice them, and throughput collapses (64 pairs at 1024 x 512, host frames: 6.8 k alignments/s with 3 contexts,
// 2.2 k with 4, when GPU_MAX_HW_QUEUES=8 gives every stream a queue of its own).  With the runtime's default of 4 queues the streams
// share queues instead and 6 contexts are the optimum (7.6 k; 3: 6.5 k; 16: 6.6 k) -- tools/ctx_threads_perf.py.
// RGBD360_CTX_ROUTE_CAP overrides (measurements).
static int ctx_route_cap() {
    static const int v = [] {
        const char* q = knobs::product("GPU_MAX_HW_QUEUES");
        const int dflt = (q && atoi(q) > 4) ? 3 : 6;
        const char* e = knobs::debug("RGBD360_CTX_ROUTE_CAP");
        const int c = e ? atoi(e) : dflt;
        return c >= 1 && c <= 16 ? c : dflt;
    }();
    return v;
}

static int align360_batch_lockstep(rgbd360_ctx* ctx, int n_frames, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                                   size_t depth_step, int depth_type, int rows, int cols, const float* g, int method, int n_inflight,
                                   float* poses_out, rgbd360_result* results_out, bool on_device) {
    const int n = n_frames - 1;
    // host frames: the call is PCIe-bound and a round's frames travel while the previous round is aligned -- more than 16 slots only
    // lengthen the first (unoverlapped) upload and the staging buffers (4.37 k alignments/s with 16 slots, 4.12 k with 32)
    const int S = std::min(on_device ? n_inflight : std::min(n_inflight, 16), n);
    int n_eng = S >= 4 ? 2 : 1;
    if (const char* e = knobs::product("RGBD360_SEQ_ENGINES")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 4) n_eng = std::min(v, S);
    }
    while ((S + n_eng - 1) / n_eng > kMaxSlots) ++n_eng;
    std::vector<int> cnt(n_eng), off(n_eng);
    for (int e = 0, o = 0; e < n_eng; ++e) {
        cnt[e] = S / n_eng + (e < S % n_eng ? 1 : 0);
        off[e] = o;
        o += cnt[e];
    }
    hipSetDevice(ctx->p.device);
    // engines are kept between calls; geometry or slot count changes rebuild them
    bool rebuild = (int)ctx->engines.size() != n_eng;
    for (int e = 0; !rebuild && e < n_eng; ++e)
        rebuild = ctx->engines[e]->rows != rows || ctx->engines[e]->cols != cols || ctx->engines[e]->P != cnt[0];
    if (rebuild) {
        for (SeqEngine* e : ctx->engines) seq_free(e);
        ctx->engines.clear();
        for (int e = 0; e < n_eng; ++e) {
            SeqEngine* E = nullptr;
            std::string err;
            const int rc = seq_create(ctx->p, cnt[0], rows, cols, ctx->max_eval_blocks, &E, &err);
            if (rc == 0) E->libm = ctx->index_libm;
            if (rc) return fail(ctx, rc, err.c_str());
            ctx->engines.push_back(E);
        }
    }
    std::vector<int> a(S), b(S);      // contiguous balanced spans [a, b) of pairs per slot
    for (int c = 0; c < S; ++c) shard_range(n, c, S, &a[c], &b[c]);
    std::vector<int> rcs(n_eng, 0);
    auto run_engine = [&](int e) {
        rcs[e] = seq_run(ctx->engines[e], cnt[e], a.data() + off[e], b.data() + off[e], rgb, rgb_step, depth, depth_step, depth_type, g, method,
                         on_device, poses_out, results_out);
        if (rcs[e]) hipStreamSynchronize(ctx->engines[e]->stream);
    };
    run_on_threads(n_eng, run_engine);
    for (int e = 0; e < n_eng; ++e)
        if (rcs[e]) return fail(ctx, rcs[e], ctx->engines[e]->err.c_str());
    return 0;
}

static int align360_batch_impl(rgbd360_ctx* ctx, int n_frames, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                               size_t depth_step, int depth_type, int rows, int cols, const float guess[16], int method,
                               int occlusion, int n_inflight, float* poses_out, rgbd360_result* results_out, bool on_device) {
    if (!ctx) return -1;
    if (!rgb || !depth || !poses_out) return fail(ctx, -1, "null pointer");
    if (n_frames < 1) return fail(ctx, -1, "n_frames must be >= 1");
    if (n_inflight < 1 || n_inflight > 64) return fail(ctx, -1, "n_inflight must be in 1..64");
    if (method < 0 || method > 2) return fail(ctx, -4, "bad method");
    if (occlusion < 0 || occlusion > 2) return fail(ctx, -5, "occlusion must be 0, 1 or 2");
    if (depth_type != 0 && depth_type != 1) return fail(ctx, -1, "depth_type must be 0 (u16 mm) or 1 (f32 m)");
    if (n_frames == 1) return 0;
    for (int k = 0; k < n_frames; ++k)
        if (!rgb[k] || !depth[k]) return fail(ctx, -1, "null frame pointer");
    const char* route = knobs::debug("RGBD360_SEQ_ROUTE");          // "contexts": the per-context route for every sequence (A/B measurements)
    // the occlusion-aware passes have no slot dimension: those sequences run one context per sub-chunk
    if (occlusion != 0 || ctx->seq_route_contexts || (route && strcmp(route, "contexts") == 0))
        // (capped: more busy streams than hardware queues run side by side costs a factor of three, see ctx_route_cap)
        return align360_batch_threads(ctx, n_frames, rgb, rgb_step, depth, depth_step, depth_type, rows, cols, guess, method, occlusion,
                                      std::min(n_inflight, ctx->seq_route_cap > 0 ? ctx->seq_route_cap : ctx_route_cap()), poses_out, results_out, on_device);
    return align360_batch_lockstep(ctx, n_frames, rgb, rgb_step, depth, depth_step, depth_type, rows, cols, guess ? guess : kIdentityPose, method,
                                   n_inflight, poses_out, results_out, on_device);
}

int rgbd360_align360_batch(rgbd360_ctx* ctx, int n_frames, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                           size_t depth_step, int depth_type, int rows, int cols, const float guess[16], int method,
                           int occlusion, int n_inflight, float* poses_out, rgbd360_result* results_out) {
    return align360_batch_impl(ctx, n_frames, rgb, rgb_step, depth, depth_step, depth_type, rows, cols, guess, method, occlusion,
                               n_inflight, poses_out, results_out, false);
}
int rgbd360_align360_batch_dev(rgbd360_ctx* ctx, int n_frames, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth,
                               size_t depth_step, int depth_type, int rows, int cols, const float guess[16], int method,
                               int occlusion, int n_inflight, float* poses_out, rgbd360_result* results_out) {
    return align360_batch_impl(ctx, n_frames, rgb, rgb_step, depth, depth_step, depth_type, rows, cols, guess, method, occlusion,
                               n_inflight, poses_out, results_out, true);
}

int rgbd360_level_dims(rgbd360_ctx* ctx, int level, int* rows, int* cols) {
    if (!ctx || level < 0 || level >= (int)ctx->levels.size()) return -3;
    *rows = ctx->levels[level].rows;
    *cols = ctx->levels[level].cols;
    return 0;
}

int rgbd360_get_plane(rgbd360_ctx* ctx, int which, int level, float* host_out) {
    if (!ctx || !host_out) return -1;
    if (level < 0 || level >= (int)ctx->levels.size()) return fail(ctx, -3, "bad pyramid level");
    hipSetDevice(ctx->p.device);
    const Level& L = ctx->levels[level];
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    if (which >= 0 && which <= 3) {
        const float* src = which == 0 ? L.graySrc : which == 1 ? L.grayTrg : which == 2 ? L.depthSrc : L.depthTrg;
        HIPC(ctx, hipMemcpy(host_out, src, (size_t)L.n * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    if (which >= 4 && which <= 7) {
        std::vector<F3> tmp(L.n);
        HIPC(ctx, hipMemcpy(tmp.data(), which < 6 ? L.trgP : L.trgD, (size_t)L.n * sizeof(F3), hipMemcpyDeviceToHost));
        const bool x = (which == 4 || which == 6);
        for (int i = 0; i < L.n; ++i) host_out[i] = x ? tmp[i].b : tmp[i].c;
        return 0;
    }
    return fail(ctx, -4, "bad plane id");
}

int rgbd360_get_lut(rgbd360_ctx* ctx, int level, float* host_out_xyz) {
    if (!ctx || !host_out_xyz) return -1;
    if (level < 0 || level >= (int)ctx->levels.size()) return fail(ctx, -3, "bad pyramid level");
    if (!ctx->have_src) return fail(ctx, -2, "no source frame");
    hipSetDevice(ctx->p.device);
    const Level& L = ctx->levels[level];
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float4> tmp(L.n);
    HIPC(ctx, hipMemcpy(tmp.data(), L.srcRec, (size_t)L.n * sizeof(float4), hipMemcpyDeviceToHost));
    for (int i = 0; i < L.n; ++i) {
        host_out_xyz[3 * i] = tmp[i].x;
        host_out_xyz[3 * i + 1] = tmp[i].y;
        host_out_xyz[3 * i + 2] = tmp[i].z;
    }
    return 0;
}

int rgbd360_eval(rgbd360_ctx* ctx, int level, const float pose[16], int method, double* err2, long long* n_valid,
                 double err2_split[2], long long n_split[2], float H[36], float g[6], double H64[36], double g64[6],
                 long long* n_visible) {
    return rgbd360_eval_occ(ctx, level, pose, method, 0, err2, n_valid, err2_split, n_split, H, g, H64, g64, n_visible);
}

int rgbd360_eval_occ(rgbd360_ctx* ctx, int level, const float pose[16], int method, int occlusion, double* err2,
                     long long* n_valid, double err2_split[2], long long n_split[2], float H[36], float g[6], double H64[36],
                     double g64[6], long long* n_visible) {
    int rc = check_args(ctx, level, method);
    if (rc) return rc;
    if (!pose) return fail(ctx, -1, "null pose pointer");
    if (occlusion < 0 || occlusion > 2) return fail(ctx, -5, "occlusion must be 0, 1 or 2");
    hipSetDevice(ctx->p.device);
    if (occlusion != 0 && (rc = occ_ensure(ctx)) != 0) return rc;
    launch_level_init(ctx, level, pose, 1);
    launch_eval(ctx, level, method, true, occlusion);
    launch_solve(ctx, level, 1, 0, occlusion);
    HIPC(ctx, hipGetLastError());
    rc = read_state(ctx);
    if (rc) return rc;
    const GNState& S = *ctx->h_state;
    if (err2) *err2 = S.tot[P_E2P] + S.tot[P_E2D];
    if (n_valid) *n_valid = (long long)(S.tot[P_NP] + S.tot[P_ND]);
    lm::Sums T;
    T.add_row(S.tot);
    T.write(err2_split, n_split, nullptr, nullptr, H64, g64, n_visible);
    if (H) memcpy(H, S.H, sizeof(float) * 36);      // the device solve's own float H, g
    if (g) memcpy(g, S.g, sizeof(float) * 6);
    return 0;
}

int rgbd360_warp_indices(rgbd360_ctx* ctx, int level, const float pose[16], int32_t* host_out_rc) {
    if (!ctx || !pose || !host_out_rc) return -1;
    if (level < 0 || level >= (int)ctx->levels.size()) return fail(ctx, -3, "bad pyramid level");
    if (!ctx->have_src) return fail(ctx, -2, "no source frame");
    hipSetDevice(ctx->p.device);
    const Level& L = ctx->levels[level];
    DevBuf<int32_t> d_out;
    HIPC(ctx, d_out.ensure((size_t)L.n * 2));
    Pose16 P;
    memcpy(P.v, pose, sizeof(P.v));
    hipLaunchKernelGGL(k_warp_indices, dim3((L.n + 255) / 256), dim3(256), 0, ctx->stream, level_dev(L), P, d_out.get());
    HIPC(ctx, hipMemcpyAsync(host_out_rc, d_out, (size_t)L.n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int rgbd360_gn_step(rgbd360_ctx* ctx, const float H[36], const float g[6], float lambda, const float pose[16],
                    float pose_tmp[16], float update[6]) {
    if (!ctx || !H || !g || !pose) return -1;
    hipSetDevice(ctx->p.device);
    GnIO io;
    memcpy(io.H, H, sizeof(io.H));
    memcpy(io.g, g, sizeof(io.g));
    memcpy(io.pose, pose, sizeof(io.pose));
    io.lambda = lambda;
    io.status = -1;
    HIPC(ctx, hipMemcpyAsync(ctx->d_gnio, &io, sizeof(io), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_gn_step, dim3(1), dim3(64), 0, ctx->stream, ctx->d_gnio);
    HIPC(ctx, hipMemcpyAsync(&io, ctx->d_gnio, sizeof(io), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    if (pose_tmp) memcpy(pose_tmp, io.pose_tmp, sizeof(io.pose_tmp));
    if (update) memcpy(update, io.update, sizeof(io.update));
    return io.status;
}

int rgbd360_forced_iters(rgbd360_ctx* ctx, int level, const float pose0[16], int method, int n_iters, float pose_out[16],
                         double* last_rms, float* elapsed_ms) {
    int rc = check_args(ctx, level, method);
    if (rc) return rc;
    if (!pose0 || n_iters < 1) return fail(ctx, -1, "bad arguments");
    hipSetDevice(ctx->p.device);
    const bool fold_init = fused_ok(ctx, 0) && !elapsed_ms;      // the first fused launch initialises the state itself (timed calls keep
    if (!fold_init) launch_level_init(ctx, level, pose0, 1);      // the initialisation outside the events)
    if (elapsed_ms) HIPC(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (fused_ok(ctx, 0)) {       // n_iters launches {solve of the previous pass, pass} + the last solve
        for (int k = 0; k < n_iters; ++k) launch_eval_fused(ctx, level, method, 1, fold_init && k == 0 ? pose0 : nullptr);
        launch_solve_pending(ctx, 1, /*publish=*/!elapsed_ms);
    } else {
        for (int k = 0; k < n_iters; ++k) {
            launch_eval(ctx, level, method, true);
            launch_solve(ctx, level, 0, 1, 0, /*publish=*/!elapsed_ms && k == n_iters - 1);
        }
    }
    if (elapsed_ms) HIPC(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPC(ctx, hipGetLastError());
    // events want the synchronise; without them the last solve has published the state and the host spins on its tag (host_wait.h)
    if (elapsed_ms) rc = read_state_sync(ctx);
    else HIPC(ctx, hostwait::wait(ctx->tag, ctx->stream));
    if (rc) return rc;
    if (elapsed_ms) HIPC(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
    const GNState& S = *ctx->h_state;
    if (pose_out) memcpy(pose_out, S.pose, sizeof(float) * 16);
    if (last_rms) *last_rms = S.error;
    return S.status;
}

// One solve on a hand-made partial table (row 0 = `row`, every other row zero) at the identity pose, through the two-launch form
// (k_solve) or through the fused form (the prologue of k_eval_fs; the state is read as that launch leaves it): the state-machine paths real images hardly
// ever reach (ILL-POSED by the rank test alone, by a zero pivot, ...) can be driven from a test.  Needs both frames set (the fused
// form runs a pass afterwards when the step is accepted).  out_i: {status, done, level_active, it, n_evals, pend_nb}.
int rgbd360_debug_solve_partials(rgbd360_ctx* ctx, int level, const double row[32], int method, int fused, int out_i[6], float cand_out[16],
                                 float update_out[6]) {
    int rc = check_args(ctx, level, method);
    if (rc) return rc;
    if (!row || !out_i) return fail(ctx, -1, "bad arguments");
    if (fused && !fused_ok(ctx, 0)) return fail(ctx, -1, "the fused-solve schedule is switched off");
    hipSetDevice(ctx->p.device);
    const Level& L = ctx->levels[level];
    float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    launch_level_init(ctx, level, I, 1);
    const size_t rows = (size_t)std::max((ctx->max_blocks + 31) / 32 * 32, kPendingRows);
    HIPC(ctx, hipMemsetAsync(ctx->d_partials, 0, rows * kNumPartials * sizeof(double), ctx->stream));
    // fused == 2: the row sits beyond the first batch of rows and the launch is given too small a bound -- stage_pending has to notice
    // that the state holds more rows than the host said and fetch them (the bound is checked on the device, not trusted)
    const int row_at = fused == 2 ? 40 : 0;
    if (row_at >= L.nblocks) return fail(ctx, -1, "the level has too few block rows for the late-row form");
    HIPC(ctx, hipMemcpyAsync(ctx->d_partials + (size_t)row_at * kNumPartials, row, kNumPartials * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (fused) {
        const int pend[2] = {L.nblocks, L.n};       // as if a pass of this level had just written the table
        HIPC(ctx, hipMemcpyAsync(&ctx->d_state[0].pend_nb, pend, sizeof(pend), hipMemcpyHostToDevice, ctx->stream));
        ctx->pend_rows_hint = fused == 2 ? 1 : kPendingRows;      // a hand-made pending pass: no bound known
        launch_eval_fused(ctx, level, method, 0);      // the state is read as this launch leaves it: its own pass (if it ran one) stays pending
    } else {
        launch_solve(ctx, level, 0, 0);
    }
    HIPC(ctx, hipGetLastError());
    rc = read_state_sync(ctx);
    if (rc) return rc;
    const GNState& S = *ctx->h_state;
    out_i[0] = S.status; out_i[1] = S.done; out_i[2] = S.level_active; out_i[3] = S.it; out_i[4] = S.n_evals; out_i[5] = S.pend_nb;
    if (cand_out) memcpy(cand_out, S.cand, sizeof(float) * 16);
    if (update_out) memcpy(update_out, S.update, sizeof(float) * 6);
    return 0;
}

// One pending solve on a hand-made partial TABLE (rgbd360_hip_diag.h): rows 0 ... n_rows - 1 = `rows`, every other row zero, pend_nb = n_rows,
// through k_solve (route 0), the prologue of k_eval_fs (1) or k_solve_pending (2); the fused routes are told to expect rows_hint rows.
// What a single row cannot show -- which row group a row is summed in, and in which order -- shows in tot.
int rgbd360_debug_solve_table(rgbd360_ctx* ctx, int level, const double* rows, int n_rows, int rows_hint, int method, int route,
                              double tot_out[32], int out_i[6], float cand_out[16]) {
    int rc = check_args(ctx, level, method);
    if (rc) return rc;
    if (!rows || !tot_out || !out_i || n_rows < 1 || n_rows > kPendingRows || rows_hint < 1 || rows_hint > kPendingRows || route < 0 || route > 2)
        return fail(ctx, -1, "bad arguments");
    if (route && !fused_ok(ctx, 0)) return fail(ctx, -1, "the fused-solve schedule is switched off");
    hipSetDevice(ctx->p.device);
    const Level& L = ctx->levels[level];
    float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    launch_level_init(ctx, level, I, 1);
    const size_t table_rows = (size_t)std::max((ctx->max_blocks + 31) / 32 * 32, kPendingRows);
    HIPC(ctx, hipMemsetAsync(ctx->d_partials, 0, table_rows * kNumPartials * sizeof(double), ctx->stream));
    HIPC(ctx, hipMemcpyAsync(ctx->d_partials, rows, (size_t)n_rows * kNumPartials * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (route == 0) {
        SolveCfg cfg;
        cfg.level = level; cfg.mode = 0; cfg.n_pixels = L.n;
        cfg.forced = 0; cfg.max_iters = ctx->p.max_iters; cfg.occ = 0;
        cfg.tol_residual = ctx->p.tol_residual; cfg.tol_update = ctx->p.tol_update;
        hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, ctx->stream, ctx->d_state, ctx->d_partials, n_rows, cfg);
    } else {
        const int pend[2] = {n_rows, L.n};          // as if a pass of this level had just written n_rows rows
        HIPC(ctx, hipMemcpyAsync(&ctx->d_state[0].pend_nb, pend, sizeof(pend), hipMemcpyHostToDevice, ctx->stream));
        ctx->pend_rows_hint = rows_hint;
        if (route == 1) launch_eval_fused(ctx, level, method, 0);      // the state is read as this launch leaves it
        else launch_solve_pending(ctx, 0, false);
    }
    HIPC(ctx, hipGetLastError());
    rc = read_state_sync(ctx);
    ctx->pend_rows_hint = kPendingRows;             // whatever follows knows no bound
    if (rc) return rc;
    const GNState& S = *ctx->h_state;
    memcpy(tot_out, S.tot, sizeof(double) * kNumPartials);
    out_i[0] = S.status; out_i[1] = S.done; out_i[2] = S.level_active; out_i[3] = S.it; out_i[4] = S.n_evals; out_i[5] = S.pend_nb;
    if (cand_out) memcpy(cand_out, S.cand, sizeof(float) * 16);
    return 0;
}

// One solve from a chosen state (rgbd360_hip_diag.h): the state is initialised at in->pose like a level entry, the rest of the
// chosen state is written over it field by field, and the row is placed as in rgbd360_debug_solve_partials.
int rgbd360_debug_solve_state(rgbd360_ctx* ctx, int level, const double row[32], const rgbd360_solve_state_in* in, int method,
                              int occlusion, int route, rgbd360_solve_state_out* out) {
    int rc = check_args(ctx, level, method);
    if (rc) return rc;
    if (!row || !in || !out || route < 0 || route > 2 || occlusion < 0 || occlusion > 2) return fail(ctx, -1, "bad arguments");
    if (route && !fused_ok(ctx, 0)) return fail(ctx, -1, "the fused-solve schedule is switched off");
    hipSetDevice(ctx->p.device);
    const Level& L = ctx->levels[level];
    const int row_at = route == 2 ? 40 : 0;
    if (row_at >= L.nblocks) return fail(ctx, -1, "the level has too few block rows for the late-row form");
    launch_level_init(ctx, level, in->pose, 1);
    GNState* d = ctx->d_state;
    HIPC(ctx, hipMemcpyAsync(d->update, in->update, sizeof(float) * 6, hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(&d->lambda, &in->lambda, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(&d->error, &in->error, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(&d->first, &in->first, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(&d->it, &in->it, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const size_t rows = (size_t)std::max((ctx->max_blocks + 31) / 32 * 32, kPendingRows);
    HIPC(ctx, hipMemsetAsync(ctx->d_partials, 0, rows * kNumPartials * sizeof(double), ctx->stream));
    HIPC(ctx, hipMemcpyAsync(ctx->d_partials + (size_t)row_at * kNumPartials, row, kNumPartials * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SolveCfg cfg = fused_cfg(ctx, in->forced, occlusion);
    cfg.max_iters = in->max_iters;
    cfg.tol_residual = in->tol_residual;
    cfg.tol_update = in->tol_update;
    if (route) {
        const int pend[2] = {L.nblocks, L.n};       // as if a pass of this level had just written the table
        HIPC(ctx, hipMemcpyAsync(&d->pend_nb, pend, sizeof(pend), hipMemcpyHostToDevice, ctx->stream));
        ctx->pend_rows_hint = route == 2 ? 1 : kPendingRows;
        launch_eval_fused(ctx, level, method, in->forced, nullptr, &cfg);
    } else {
        launch_solve(ctx, level, 0, in->forced, occlusion, false, &cfg);
    }
    HIPC(ctx, hipGetLastError());
    rc = read_state_sync(ctx);
    if (rc) return rc;
    const GNState& S = *ctx->h_state;
    out->status = S.status; out->done = S.done; out->level_active = S.level_active; out->it = S.it; out->n_evals = S.n_evals;
    out->pend_nb = S.pend_nb; out->iters_level = S.iters[level & 7];
    memcpy(out->cand, S.cand, sizeof(out->cand));
    memcpy(out->pose, S.pose, sizeof(out->pose));
    memcpy(out->update, S.update, sizeof(out->update));
    out->lambda = S.lambda; out->error = S.error; out->new_error = S.new_error; out->diff_error = S.diff_error;
    return 0;
}

int rgbd360_time_eval_kernel(rgbd360_ctx* ctx, int level, const float pose[16], int method, int want_hg, int reps,
                             float* avg_us) {
    int rc = check_args(ctx, level, method);
    if (rc) return rc;
    if (!pose || reps < 1 || !avg_us) return fail(ctx, -1, "bad arguments");
    hipSetDevice(ctx->p.device);
    launch_level_init(ctx, level, pose, 1);
    const bool fused = want_hg == 2;      // the product's single-pair launch: solve of the previous pass + pass (forced schedule)
    if (fused && !fused_ok(ctx, 0)) return fail(ctx, -1, "the fused-solve schedule is switched off");
    auto one = [&]() {
        if (fused) launch_eval_fused(ctx, level, method, 1);
        else launch_eval(ctx, level, method, want_hg != 0);
    };
    one();   // warm-up
    HIPC(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (int k = 0; k < reps; ++k) one();
    HIPC(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    if (fused) launch_solve_pending(ctx, 1, false);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPC(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *avg_us = ms * 1000.f / reps;
    return 0;
}

// The same timer with the launches ROTATING over n_ctx contexts (all on ctxs[0]'s device, each holding its own copy of a frame
// pair) on ctxs[0]'s stream: with n_ctx x working set > 256 MiB every launch finds its records evicted from the Infinity Cache,
// so the average is an HBM-fed launch -- the back-to-back timer above re-reads an Infinity-Cache-resident set at 2048x1024.
int rgbd360_time_eval_kernel_rotating(rgbd360_ctx* const* ctxs, int n_ctx, int level, const float pose[16], int method, int want_hg,
                                      int reps, float* avg_us) {
    if (!ctxs || n_ctx < 1 || !ctxs[0]) return -1;
    rgbd360_ctx* c0 = ctxs[0];
    if (!pose || reps < 1 || !avg_us) return fail(c0, -1, "bad arguments");
    for (int k = 0; k < n_ctx; ++k) {
        if (!ctxs[k]) return fail(c0, -1, "null context");
        const int rc = check_args(ctxs[k], level, method);
        if (rc) return k == 0 ? rc : fail(c0, rc, ctxs[k]->err.c_str());
        if (ctxs[k]->p.device != c0->p.device) return fail(c0, -1, "all contexts must live on one device");
        if (want_hg == 2 && !fused_ok(ctxs[k], 0)) return fail(c0, -1, "the fused-solve schedule is switched off");
    }
    hipSetDevice(c0->p.device);
    // every context's kernels go to c0's stream for the duration of the measurement: all contexts are synchronised first (the
    // only step that can fail), then the streams are swapped in a loop that cannot, and swapped back on every way out
    for (int k = 0; k < n_ctx; ++k) HIPC(c0, hipStreamSynchronize(ctxs[k]->stream));
    std::vector<hipStream_t> own(n_ctx);
    for (int k = 0; k < n_ctx; ++k) {
        own[k] = ctxs[k]->stream;
        ctxs[k]->stream = c0->stream;
    }
    const bool fused = want_hg == 2;      // k_eval_fs, forced schedule (every context iterates on its own pair)
    auto one = [&](rgbd360_ctx* c) {
        if (fused) launch_eval_fused(c, level, method, 1);
        else launch_eval(c, level, method, want_hg != 0);
    };
    for (int k = 0; k < n_ctx; ++k) {
        launch_level_init(ctxs[k], level, pose, 1);
        one(ctxs[k]);      // warm-up
    }
    hipError_t e = hipEventRecord(c0->ev0, c0->stream);
    for (int r = 0; r < reps && e == hipSuccess; ++r) one(ctxs[r % n_ctx]);
    if (e == hipSuccess) e = hipEventRecord(c0->ev1, c0->stream);
    if (fused) for (int k = 0; k < n_ctx; ++k) launch_solve_pending(ctxs[k], 1, false);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c0->stream);
    for (int k = 0; k < n_ctx; ++k) ctxs[k]->stream = own[k];
    HIPC(c0, e);
    float ms = 0.f;
    HIPC(c0, hipEventElapsedTime(&ms, c0->ev0, c0->ev1));
    *avg_us = ms * 1000.f / reps;
    return 0;
}

// The forced schedule of rgbd360_forced_iters in the lock-step engine's regime: n_pairs copies of ONE pair iterate side by side, every
// {pass, solve} launch serving all of them (k_eval_b / k_solve_b), n_iters Gauss-Newton iterations each on `level`.  What a GN
// iteration costs when the solve launch and the launch boundaries are shared by the pairs in flight -- the product's sequence path.
int rgbd360_forced_iters_batch(rgbd360_ctx* ctx, int n_pairs, const uint8_t* rgb_trg, const void* depth_trg, const uint8_t* rgb_src,
                               const void* depth_src, size_t rgb_step, size_t depth_step, int depth_type, int rows, int cols, int level,
                               const float pose0[16], int method, int n_iters, float* poses_out, float* elapsed_ms, float* pass_avg_us) {
    if (!ctx) return -1;
    if (!rgb_trg || !depth_trg || !rgb_src || !depth_src || !pose0 || n_iters < 1 || n_pairs < 1 || n_pairs > kMaxSlots)
        return fail(ctx, -1, "bad arguments");
    if (method < 0 || method > 2) return fail(ctx, -4, "bad method");
    if (level < 0 || level >= ctx->p.n_pyr) return fail(ctx, -3, "bad pyramid level");
    if (depth_type != 0 && depth_type != 1) return fail(ctx, -1, "depth_type must be 0 (u16 mm) or 1 (f32 m)");
    hipSetDevice(ctx->p.device);
    SeqEngine* E = nullptr;
    std::string err;
    int rc = seq_create(ctx->p, n_pairs, rows, cols, ctx->max_eval_blocks, &E, &err);
    if (rc == 0) E->libm = ctx->index_libm;
    if (rc) return fail(ctx, rc, err.c_str());
    const size_t dpx = depth_type == 0 ? 2 : 4;
    const size_t fr = (size_t)rows * cols * 3, fd = (size_t)rows * cols * dpx;
    const std::unique_ptr<SeqEngine, void (*)(SeqEngine*)> engine(E, seq_free);      // drained and freed on every way out
    DevBuf<uint8_t> d_rgb[2], d_dep[2];
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = d_rgb[k].ensure(fr);
        if (e == hipSuccess) e = d_dep[k].ensure(fd);
        if (e == hipSuccess) e = hipMemcpy2D(d_rgb[k], (size_t)cols * 3, k == 0 ? rgb_trg : rgb_src, rgb_step, (size_t)cols * 3, rows, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy2D(d_dep[k], (size_t)cols * dpx, k == 0 ? depth_trg : depth_src, depth_step, (size_t)cols * dpx, rows, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return fail(ctx, -(int)e - 1000, hipGetErrorString(e));
    const unsigned long long live = n_pairs >= 64 ? ~0ull : ((1ull << n_pairs) - 1ull);
    FramePtrs fp;
    memset(&fp, 0, sizeof(fp));
    for (int s = 0; s < n_pairs; ++s) { fp.rgb[s] = d_rgb[0]; fp.depth[s] = d_dep[0]; }
    seq_frame_setup(E, fp, (size_t)cols * 3, (size_t)cols * dpx, depth_type, live, 0ull, live, E->tb);            // targets
    for (int s = 0; s < n_pairs; ++s) { fp.rgb[s] = d_rgb[1]; fp.depth[s] = d_dep[1]; }
    seq_frame_setup(E, fp, (size_t)cols * 3, (size_t)cols * dpx, depth_type, live, live, 0ull, E->tb ^ 1);         // sources
    Pose16 Pz;
    memcpy(Pz.v, pose0, sizeof(Pz.v));
    hipLaunchKernelGGL(k_level_init_b, dim3(n_pairs), dim3(64), 0, E->stream, E->d_states, Pz, 1, 1, level, live);
    for (int k = 0; k < 3; ++k) {        // warm
        seq_launch_eval(E, level, method);
        seq_launch_solve(E, level, 1);
    }
    hipLaunchKernelGGL(k_level_init_b, dim3(n_pairs), dim3(64), 0, E->stream, E->d_states, Pz, 1, 1, level, live);
    e = hipEventRecord(ctx->ev0, E->stream);
    for (int k = 0; k < n_iters; ++k) {
        seq_launch_eval(E, level, method);
        seq_launch_solve(E, level, 1);
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->ev1, E->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(E->h_states, E->d_states, (size_t)n_pairs * sizeof(GNState), hipMemcpyDeviceToHost, E->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(E->stream);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (e == hipSuccess && pass_avg_us) {      // the batch pass alone: back-to-back launches at the poses the iterations reached
        constexpr int kReps = 10;
        e = hipEventRecord(ctx->ev0, E->stream);
        for (int k = 0; k < kReps; ++k) seq_launch_eval(E, level, method);
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, E->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(E->stream);
        float pms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&pms, ctx->ev0, ctx->ev1);
        if (e == hipSuccess) *pass_avg_us = pms * 1e3f / kReps;
    }
    int status = 0;
    if (e == hipSuccess) {
        if (elapsed_ms) *elapsed_ms = ms;
        for (int s = 0; s < n_pairs; ++s) {
            if (poses_out) memcpy(poses_out + 16 * s, E->h_states[s].pose, sizeof(float) * 16);
            if (E->h_states[s].status != 0) status = E->h_states[s].status;
        }
    }
    if (e != hipSuccess) return fail(ctx, -(int)e - 1000, hipGetErrorString(e));
    return status;
}

int rgbd360_time_solve_kernel(rgbd360_ctx* ctx, int level, int mode, int reps, float* avg_us) {
    int rc = check_args(ctx, level, 0);
    if (rc) return rc;
    if (reps < 1 || !avg_us) return fail(ctx, -1, "bad arguments");
    hipSetDevice(ctx->p.device);
    launch_solve(ctx, level, mode, 1);   // warm-up (partials of the last pass)
    HIPC(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (int k = 0; k < reps; ++k) launch_solve(ctx, level, mode, 1);
    HIPC(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPC(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *avg_us = ms * 1000.f / reps;
    return 0;
}

int rgbd360_debug_eval_stamps(rgbd360_ctx* ctx, int level, double out[16]) {      // blocks 0 and nb - 1, 8 values each
    if (!ctx || !out || level < 0 || level >= (int)ctx->levels.size()) return -1;
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    const int nb = ctx->levels[level].nblocks;
    HIPC(ctx, hipMemcpy(out, ctx->d_partials + (size_t)nb * kNumPartials, 8 * sizeof(double), hipMemcpyDeviceToHost));
    HIPC(ctx, hipMemcpy(out + 8, ctx->d_partials + (size_t)(nb + 1) * kNumPartials, 8 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int rgbd360_debug_eval_blocks(rgbd360_ctx* ctx, int level, double* out /*2*nblocks*/) {
    if (!ctx || !out || level < 0 || level >= (int)ctx->levels.size()) return -1;
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    const int nb = ctx->levels[level].nblocks;
    HIPC(ctx, hipMemcpy(out, ctx->d_partials + (size_t)(nb + 8) * kNumPartials, 2 * nb * sizeof(double), hipMemcpyDeviceToHost));
    return nb;
}

int rgbd360_debug_eval_waves(rgbd360_ctx* ctx, int level, double* out /*16*nblocks*/) {      // per wave: "loop done", 100 MHz ticks from its block's start
    if (!ctx || !out || level < 0 || level >= (int)ctx->levels.size()) return -1;
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    const int nb = ctx->levels[level].nblocks;
    HIPC(ctx, hipMemcpy(out, ctx->d_partials + (size_t)(nb + 32) * kNumPartials, 16 * nb * sizeof(double), hipMemcpyDeviceToHost));
    return nb;
}

int rgbd360_debug_eval_history(rgbd360_ctx* ctx, int level, int reset, double out[120]) {
    if (!ctx || level < 0 || level >= (int)ctx->levels.size()) return -1;
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    const int nb = ctx->levels[level].nblocks;
    if (reset) HIPC(ctx, hipMemset(ctx->d_partials + (size_t)(nb + 2) * kNumPartials, 0, 5 * kNumPartials * sizeof(double)));
    if (out) HIPC(ctx, hipMemcpy(out, ctx->d_partials + (size_t)(nb + 3) * kNumPartials, 120 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int rgbd360_debug_solve_stamps(rgbd360_ctx* ctx, unsigned long long out[8]) {
    if (!ctx || !out) return -1;
    int rc = read_state(ctx);
    if (rc) return rc;
    memcpy(out, ctx->h_state[0].stamps, sizeof(unsigned long long) * 8);
    return 0;
}

int rgbd360_selftest_math(rgbd360_ctx* ctx, uint32_t first_bits, uint32_t count, unsigned long long mismatches[3]) {
    if (!ctx || !mismatches) return -1;
    hipSetDevice(ctx->p.device);
    DevBuf<unsigned long long> d;
    HIPC(ctx, d.ensure(3));
    HIPC(ctx, hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_selftest_math, dim3(2048), dim3(256), 0, ctx->stream, first_bits, count, d.get());
    HIPC(ctx, hipMemcpyAsync(mismatches, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// libm_f32.h as the DEVICE compiles it against the C library this process links (the reference's asinf / atanf / roundf / atan2f): the floats
// first_bits .. first_bits + count - 1 through the three one-argument functions, `count` drawn pairs through atan2f.  mismatches[4].
int rgbd360_selftest_libm(rgbd360_ctx* ctx, uint32_t first_bits, uint32_t count, unsigned long long mismatches[4]) {
    if (!ctx || !mismatches) return -1;
    hipSetDevice(ctx->p.device);
    for (int k = 0; k < 4; ++k) mismatches[k] = 0;
    constexpr uint32_t kChunk = 1u << 22;
    DevBuf<float> d;
    HIPC(ctx, d.ensure(4 * (size_t)kChunk));
    std::vector<float> h(4 * (size_t)kChunk);
    auto differ = [](float a, float b) {
        uint32_t x, y;
        memcpy(&x, &a, 4); memcpy(&y, &b, 4);
        return x != y && !((x & 0x7fffffffu) > 0x7f800000u && (y & 0x7fffffffu) > 0x7f800000u);      // (any NaN equals any NaN)
    };
    hipError_t e = hipSuccess;
    int shown = 0;
    for (uint64_t done = 0; done < count && e == hipSuccess; done += kChunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(kChunk, count - done), first = first_bits + (uint32_t)done;
        hipLaunchKernelGGL(k_selftest_libm, dim3(2048), dim3(256), 0, ctx->stream, first, n, d.get());
        e = hipMemcpyAsync(h.data(), d, 4 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) break;
        for (uint32_t k = 0; k < n; ++k) {
            float v;
            const uint32_t u = first + k;
            memcpy(&v, &u, 4);
            if ((u & 0x7fffffffu) <= 0x3fc00000u) {
                const bool bad = differ(h[k], asinf(v));
                mismatches[0] += bad;
                if (bad && shown < 6 && knobs::debug("RGBD360_SELFTEST_VERBOSE")) {      // (debug builds: the first mismatches on stderr)
                    ++shown;
                    fprintf(stderr, "[selftest_libm] asinf(%.9g = 0x%08x): device %.9g, library %.9g\n", (double)v, u, (double)h[k], (double)asinf(v));
                }
            }
            mismatches[1] += differ(h[(size_t)n + k], atanf(v));
            mismatches[2] += differ(h[2 * (size_t)n + k], roundf(v));
            float y, x;
            selftest_libm_pair(u, y, x);
            mismatches[3] += differ(h[3 * (size_t)n + k], atan2f(y, x));
        }
    }
    HIPC(ctx, e);
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// Pinhole single-sensor alignment: RegisterPhotoICP::alignFrames, RPI.h:4254-4512.
// Per-pixel passes on the device (pinhole_kernels.h), Levenberg-Marquardt driver on the host.
// ---------------------------------------------------------------------------------------------------------
namespace {

int pin_check(rgbd360_ctx* ctx, int level, int method) {
    int rc = check_args(ctx, level, method);
    if (rc) return rc;
    if (!ctx->have_cam) return fail(ctx, -2, "rgbd360_set_camera was not called");
    if (ctx->p.mask_seams) return fail(ctx, -5, "pinhole alignment needs params.mask_seams = 0 (the seam mask belongs to the spherical panorama)");
    return 0;
}

int pin_prepare_level(rgbd360_ctx* ctx, int level) {
    Level& L = ctx->levels[level];
    HIPC(ctx, L.srcRecPin.ensure((size_t)L.n));
    const PinK K = level_K(ctx->cam, level);
    const float inv_fx = 1. / K.fx, inv_fy = 1. / K.fy;
    hipLaunchKernelGGL(k_src_rec_pinhole, grid2d(L.rows, L.cols), dim3(256), 0, ctx->stream, L.depthSrc, L.graySrc, L.rows, L.cols, K,
                       inv_fx, inv_fy, ctx->p.min_depth, ctx->p.max_depth, L.srcRecPin.get());
    HIPC(ctx, hipGetLastError());
    return 0;
}

LevelDev pin_level_dev(const Level& L) {
    LevelDev d = level_dev(L);
    d.src = L.srcRecPin;
    return d;
}

// one fused pass at `pose`; the reduced sums land in ctx->h_state->tot
int pin_eval(rgbd360_ctx* ctx, int level, const float* pose, int method) {
    const Level& L = ctx->levels[level];
    const LevelDev lv = pin_level_dev(L);
    const PinK K = level_K(ctx->cam, level);
    const EvalConsts ec = eval_consts(ctx->p);
    // two launches per evaluation: the pass (pose by kernel argument) and the reduce-only solve, which publishes the sums to the
    // host itself (was: state initialisation + pass + solve + copy, 21 us per round trip)
    Pose16 P;
    memcpy(P.v, pose, sizeof(P.v));
    const dim3 g(L.nblocks), b(kEvalThreads);
    with_method(method, [&](auto M) {
        hipLaunchKernelGGL((k_eval_pinhole<M>), g, b, 0, ctx->stream, lv, K, ec, P, ctx->d_partials, L.chunk, level, ctx->sal_thr);
    });
    launch_solve(ctx, level, 1, 0, 0, /*publish=*/true);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hostwait::wait(ctx->tag, ctx->stream));
    return 0;
}

// The occlusion-aware evaluation (pinhole_kernels.h, second half): per-target arrival lists, one walk per target pixel in source-index
// order; the reduce-only solve publishes the sums like pin_eval's.
int pin_occ_ensure(rgbd360_ctx* ctx, size_t n) {
    // the set is complete once its last member is there (pin_partials: allocated behind the arming launch)
    if (ctx->pin_partials.capacity() > 0 && ctx->pin_keys.capacity() >= n) return 0;
    HIPC(ctx, ctx->pin_keys.ensure(n));
    HIPC(ctx, ctx->pin_vals.ensure(n));
    HIPC(ctx, ctx->pin_cnt.ensure(n));
    HIPC(ctx, ctx->pin_box.ensure(n));
    HIPC(ctx, ctx->pin_slots.ensure(n * kPinShort));
    // armed once; every walk re-arms the words of the target pixels it visited
    hipLaunchKernelGGL(k_pin_occ_arm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->pin_cnt.get(), ctx->pin_box.get(), (int)n);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, ctx->pin_partials.ensure(((n + kPinWalkThreads - 1) / kPinWalkThreads) * kNumPartials));
    return 0;
}
PinOccLists pin_lists(const rgbd360_ctx* ctx) { return PinOccLists{ctx->pin_cnt, ctx->pin_box, ctx->pin_slots}; }

int pin_eval_occ(rgbd360_ctx* ctx, int level, const float* pose, int method, int occ) {
    const Level& L = ctx->levels[level];
    int rc = pin_occ_ensure(ctx, (size_t)ctx->levels[0].n);
    if (rc) return rc;
    const LevelDev lv = pin_level_dev(L);
    const PinK K = level_K(ctx->cam, level);
    const EvalConsts ec = eval_consts(ctx->p);
    Pose16 P;
    memcpy(P.v, pose, sizeof(P.v));
    const dim3 gk((L.n + 255) / 256), bk(256);
    with_choice<1, 2>(occ != 1, [&](auto O) {
        hipLaunchKernelGGL((k_pin_occ_keys<O>), gk, bk, 0, ctx->stream, lv, K, P, ctx->pin_keys.get(), ctx->pin_vals.get(), pin_lists(ctx));
    });
    const int nblk = (L.n + kPinWalkThreads - 1) / kPinWalkThreads;
    const dim3 gw(nblk), bw(kPinWalkThreads);
    with_method(method, [&](auto M) {
        hipLaunchKernelGGL((k_pin_occ_walk<M>), gw, bw, 0, ctx->stream, lv, K, ec, P, ctx->pin_keys.get(), ctx->pin_vals.get(), pin_lists(ctx), ctx->pin_partials.get());
    });
    SolveCfg cfg;
    cfg.level = level; cfg.mode = 1; cfg.forced = 0; cfg.max_iters = ctx->p.max_iters; cfg.n_pixels = L.n;
    cfg.occ = 0;
    cfg.tol_residual = ctx->p.tol_residual; cfg.tol_update = ctx->p.tol_update;
    cfg.host_state = ctx->h_state;
    cfg.host_tag = ctx->tag.h;
    cfg.host_seq = ++ctx->tag.seq;
    hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, ctx->stream, ctx->d_state, (const double*)ctx->pin_partials, nblk, cfg);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hostwait::wait(ctx->tag, ctx->stream));
    return 0;
}

}  // namespace

extern "C" int rgbd360_set_camera(rgbd360_ctx* ctx, float fx, float fy, float ox, float oy) {
    if (!ctx) return -1;
    if (!(fx > 0.f) || !(fy > 0.f)) return fail(ctx, -1, "focal lengths must be positive");
    ctx->cam[0] = fx; ctx->cam[1] = fy; ctx->cam[2] = ox; ctx->cam[3] = oy;
    ctx->have_cam = true;
    return 0;
}

extern "C" int rgbd360_set_index_arithmetic(rgbd360_ctx* ctx, int mode) {
    if (!ctx) return -1;
    if (mode != 0 && mode != 1) return fail(ctx, -1, "index arithmetic: 0 (device definition) or 1 (the reference's libm)");
    if (ctx->al_active) return fail(ctx, -6, "an alignment is in flight");
    ctx->index_libm = mode;
    for (Level& L : ctx->levels) L.libm = mode;
    for (SeqEngine* E : ctx->engines) E->libm = mode;
    for (rgbd360_ctx* sib : ctx->siblings) rgbd360_set_index_arithmetic(sib, mode);
    return 0;
}
extern "C" int rgbd360_get_index_arithmetic(rgbd360_ctx* ctx) { return ctx ? ctx->index_libm : -1; }

extern "C" int rgbd360_use_saliency(rgbd360_ctx* ctx, int on, float thres_saliency) {
    if (!ctx) return -1;
    if (on && !(thres_saliency >= 0.f)) return fail(ctx, -1, "thres_saliency must be >= 0");
    ctx->sal_thr = on ? thres_saliency : -1.f;
    return 0;
}

static int pin_eval_any(rgbd360_ctx* ctx, int level, const float* pose, int method, int occlusion) {
    return occlusion == 0 ? pin_eval(ctx, level, pose, method) : pin_eval_occ(ctx, level, pose, method, occlusion);
}

extern "C" int rgbd360_eval_pinhole_occ(rgbd360_ctx* ctx, int level, const float pose[16], int method, int occlusion, double err2_split[2],
                                        long long n_split[2], float H[36], float g[6], double H64[36], double g64[6], long long* n_rows) {
    int rc = pin_check(ctx, level, method);
    if (rc) return rc;
    if (!pose) return fail(ctx, -1, "null pose pointer");
    if (occlusion < 0 || occlusion > 2) return fail(ctx, -5, "occlusion must be 0, 1 or 2");
    hipSetDevice(ctx->p.device);
    if ((rc = pin_prepare_level(ctx, level)) != 0) return rc;
    if ((rc = pin_eval_any(ctx, level, pose, method, occlusion)) != 0) return rc;
    lm::Sums S;
    S.add_row(ctx->h_state.get()->tot);
    S.write(err2_split, n_split, H, g, H64, g64, n_rows);
    return 0;
}

extern "C" int rgbd360_eval_pinhole(rgbd360_ctx* ctx, int level, const float pose[16], int method, double err2_split[2],
                                    long long n_split[2], float H[36], float g[6], double H64[36], double g64[6], long long* n_rows) {
    return rgbd360_eval_pinhole_occ(ctx, level, pose, method, 0, err2_split, n_split, H, g, H64, g64, n_rows);
}

extern "C" int rgbd360_warp_indices_pinhole(rgbd360_ctx* ctx, int level, const float pose[16], int32_t* host_out_rc) {
    int rc = pin_check(ctx, level, 0);
    if (rc) return rc;
    if (!pose || !host_out_rc) return fail(ctx, -1, "null pointer");
    hipSetDevice(ctx->p.device);
    if ((rc = pin_prepare_level(ctx, level)) != 0) return rc;
    const Level& L = ctx->levels[level];
    DevBuf<int32_t> d_out;
    HIPC(ctx, d_out.ensure((size_t)L.n * 2));
    Pose16 P;
    memcpy(P.v, pose, sizeof(P.v));
    hipLaunchKernelGGL(k_warp_indices_pinhole, dim3((L.n + 255) / 256), dim3(256), 0, ctx->stream, pin_level_dev(L), level_K(ctx->cam, level),
                       P, d_out.get());
    HIPC(ctx, hipMemcpyAsync(host_out_rc, d_out, (size_t)L.n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// The source frame warped into the target frame at one pose, and the difference images (warp_images.h).
// ---------------------------------------------------------------------------------------------------------
namespace {
int wi_check(rgbd360_ctx* ctx, int level, const float* pose, int method, bool pinhole) {
    const int rc = pinhole ? pin_check(ctx, level, method) : check_args(ctx, level, method);
    if (rc) return rc;
    if (!pose) return fail(ctx, -1, "null pose pointer");
    if (ctx->al_active) return fail(ctx, -6, "an alignment is in flight");
    return 0;
}

int wi_ensure(rgbd360_ctx* ctx) {
    const size_t n = (size_t)ctx->levels[0].n;
    HIPC(ctx, ctx->wi_winner.ensure(n));
    HIPC(ctx, ctx->wi_stage.ensure(4 * n));
    return 0;
}

// both passes on the context's stream; `winner` is the plane the first pass fills (the caller's or the context's)
template <bool PINHOLE>
int wi_launch(rgbd360_ctx* ctx, int level, const float* pose, int method, int32_t* winner, const WarpImagesOut& out) {
    const Level& L = ctx->levels[level];
    const LevelDev lv = PINHOLE ? pin_level_dev(L) : level_dev(L);
    const PinK K = PINHOLE ? level_K(ctx->cam, level) : PinK{0.f, 0.f, 0.f, 0.f};
    Pose16 P;
    memcpy(P.v, pose, sizeof(P.v));
    const dim3 grid = level_pixel_grid(L, kPixelThreads);
    HIPC(ctx, hipMemsetAsync(winner, 0xff, (size_t)L.n * sizeof(int32_t), ctx->stream));      // -1: nothing landed
    hipLaunchKernelGGL(k_warp_winner<PINHOLE>, grid, dim3(kPixelThreads), 0, ctx->stream, lv, K, P, winner);
    hipLaunchKernelGGL(k_warp_resolve<PINHOLE>, grid, dim3(kPixelThreads), 0, ctx->stream, lv, K, P, method, ctx->p.thres_sal_photo,
                       (const int32_t*)winner, out);
    HIPC(ctx, hipGetLastError());
    return 0;
}

template <bool PINHOLE>
int wi_host(rgbd360_ctx* ctx, int level, const float* pose, int method, float* warped_gray, float* warped_depth, float* diff_gray,
            float* diff_depth, int32_t* winner) {
    int rc = wi_check(ctx, level, pose, method, PINHOLE);
    if (rc) return rc;
    hipSetDevice(ctx->p.device);
    if (PINHOLE && (rc = pin_prepare_level(ctx, level)) != 0) return rc;
    if ((rc = wi_ensure(ctx)) != 0) return rc;
    const size_t n = (size_t)ctx->levels[level].n;
    float* const host[4] = {warped_gray, warped_depth, diff_gray, diff_depth};
    float* dev[4];
    for (int k = 0; k < 4; ++k) dev[k] = host[k] ? ctx->wi_stage + k * ctx->wi_winner.capacity() : nullptr;
    if ((rc = wi_launch<PINHOLE>(ctx, level, pose, method, ctx->wi_winner, WarpImagesOut{dev[0], dev[1], dev[2], dev[3]})) != 0) return rc;
    for (int k = 0; k < 4; ++k)
        if (host[k]) HIPC(ctx, hipMemcpyAsync(host[k], dev[k], n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (winner) HIPC(ctx, hipMemcpyAsync(winner, ctx->wi_winner, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
}  // namespace

extern "C" int rgbd360_warp_images(rgbd360_ctx* ctx, int level, const float pose[16], int method, float* warped_gray, float* warped_depth,
                                   float* diff_gray, float* diff_depth, int32_t* winner) {
    return wi_host<false>(ctx, level, pose, method, warped_gray, warped_depth, diff_gray, diff_depth, winner);
}

extern "C" int rgbd360_warp_images_pinhole(rgbd360_ctx* ctx, int level, const float pose[16], int method, float* warped_gray,
                                           float* warped_depth, float* diff_gray, float* diff_depth, int32_t* winner) {
    return wi_host<true>(ctx, level, pose, method, warped_gray, warped_depth, diff_gray, diff_depth, winner);
}

extern "C" int rgbd360_warp_images_dev(rgbd360_ctx* ctx, int level, const float pose[16], int method, float* warped_gray_dev,
                                       float* warped_depth_dev, float* diff_gray_dev, float* diff_depth_dev, int32_t* winner_dev) {
    int rc = wi_check(ctx, level, pose, method, false);
    if (rc) return rc;
    hipSetDevice(ctx->p.device);
    if (!winner_dev && (rc = wi_ensure(ctx)) != 0) return rc;
    return wi_launch<false>(ctx, level, pose, method, winner_dev ? winner_dev : ctx->wi_winner,
                            WarpImagesOut{warped_gray_dev, warped_depth_dev, diff_gray_dev, diff_depth_dev});
}

// rgbd360_hip_diag.h: HIP-event averages over `reps` back-to-back launches of {the winner pass, the resolve pass, the whole
// rgbd360_warp_images_dev sequence (clear + both passes), one k_warp_indices launch} on this level, outputs into the context's staging.
extern "C" int rgbd360_time_warp_images(rgbd360_ctx* ctx, int level, const float pose[16], int method, int reps, float avg_us[4]) {
    int rc = wi_check(ctx, level, pose, method, false);
    if (rc) return rc;
    if (reps < 1 || !avg_us) return fail(ctx, -1, "bad arguments");
    hipSetDevice(ctx->p.device);
    if ((rc = wi_ensure(ctx)) != 0) return rc;
    const Level& L = ctx->levels[level];
    const LevelDev lv = level_dev(L);
    const PinK K = {0.f, 0.f, 0.f, 0.f};
    Pose16 P;
    memcpy(P.v, pose, sizeof(P.v));
    const dim3 grid = level_pixel_grid(L, kPixelThreads);
    const size_t wi_n = ctx->wi_winner.capacity();
    const WarpImagesOut out = {ctx->wi_stage, ctx->wi_stage + wi_n, ctx->wi_stage + 2 * wi_n, ctx->wi_stage + 3 * wi_n};
    int32_t* const winner = ctx->wi_winner;
    for (int what = 0; what < 4; ++what) {
        auto one = [&]() {
            if (what == 0) hipLaunchKernelGGL(k_warp_winner<false>, grid, dim3(kPixelThreads), 0, ctx->stream, lv, K, P, winner);
            if (what == 1) hipLaunchKernelGGL(k_warp_resolve<false>, grid, dim3(kPixelThreads), 0, ctx->stream, lv, K, P, method, ctx->p.thres_sal_photo, (const int32_t*)winner, out);
            if (what == 2) (void)wi_launch<false>(ctx, level, pose, method, winner, out);
            if (what == 3) hipLaunchKernelGGL(k_warp_indices, grid, dim3(kPixelThreads), 0, ctx->stream, lv, P, (int32_t*)ctx->wi_stage.get());      // 8 of the staging's 16 B/px
        };
        if (what == 0) HIPC(ctx, hipMemsetAsync(winner, 0xff, (size_t)L.n * sizeof(int32_t), ctx->stream));
        one();      // warm-up
        HIPC(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        for (int k = 0; k < reps; ++k) one();
        HIPC(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        HIPC(ctx, hipGetLastError());
        HIPC(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        HIPC(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        avg_us[what] = ms * 1000.f / reps;
    }
    return 0;
}

extern "C" int rgbd360_align_pinhole(rgbd360_ctx* ctx, const float guess[16], int method, int occlusion, float pose_out[16],
                                     rgbd360_result* res) {
    int rc = pin_check(ctx, 0, method);
    if (rc) return rc;
    if (!guess || !pose_out) return fail(ctx, -1, "null pose pointer");
    if (occlusion < 0 || occlusion > 2) return fail(ctx, -5, "occlusion must be 0, 1 or 2");
    hipSetDevice(ctx->p.device);
    // avResidual and its two parts: of the latest evaluation, of the one before it, and what the latest trip started from
    struct Residuals { double eval = 0, photo = 0, depth = 0; } last, before, temp;
    float sso = 0.f;
    // RPI.h:742-744: both averages / nValidDepthPts; the _Occ passes divide the photometric sum by its own count (RPI.h:1314-1317, 1765-1768)
    auto residuals = [&](const lm::Sums& S) {
        Residuals r;
        r.photo = sqrt(S.e2p / (occlusion ? S.np : S.nd));
        r.depth = sqrt(S.e2d / S.nd);
        r.eval = r.photo + r.depth;
        return r;
    };
    auto eval = [&](int level, const float* pose, lm::Sums& S) -> int {
        const int e = pin_eval_any(ctx, level, pose, method, occlusion);
        if (e) return e;
        S.add_row(ctx->h_state.get()->tot);
        before = last;
        last = residuals(S);
        return 0;
    };
    const bool pin_trace = knobs::debug("RGBD360_PIN_TRACE") != nullptr;      // debug builds: every trip's error, update, g and diag(H) on stderr
    auto on_trip = [&](const lm::Trip& t) {
        temp = before;      // avResidual_temp: a trip's candidate is its first evaluation, so `before` is what the trip started from
        if (occlusion == 2) sso = (float)(t.at_pose->rows / (double)ctx->levels[t.level].n);      // calcHessGrad_Occ2 sets SSO (RPI.h:2016)
        if (!pin_trace) return;
        fprintf(stderr, "[pin trace] level %d it %d lambda %g: error %.10f -> %.10f, update", t.level, t.it, (double)t.lambda, t.error, t.new_error);
        for (int k = 0; k < 6; ++k) fprintf(stderr, " %.9g", (double)t.update[k]);
        fprintf(stderr, "; g");
        for (int k = 0; k < 6; ++k) fprintf(stderr, " %.9g", (double)t.g[k]);
        fprintf(stderr, "; diag H");
        for (int k = 0; k < 6; ++k) fprintf(stderr, " %.9g", (double)t.H[k * 6 + k]);
        fprintf(stderr, "\n");
    };
    lm::Outcome O;
    rc = lm::align(lm::pinhole_schedule(), ctx->p.n_pyr, guess, [&](int level) { return pin_prepare_level(ctx, level); }, eval,
                   [&](const lm::Sums& S) { return residuals(S).eval; }, on_trip, &O);
    if (rc) return rc;
    memcpy(pose_out, O.pose, sizeof(O.pose));
    if (O.status == 0 && O.final_error != O.final_error) O.status = 2;      // NaN: no depth-valid pixel (or PHOTO only: x / nValidDepthPts)
    rgbd360_result R;
    memset(&R, 0, sizeof(R));
    R.status = O.status;
    // avResidual = avResidual_temp (RPI.h:4507-4509); an ILL-POSED trip evaluates nothing, so what it started from is `last`
    const Residuals& av = O.any_trip && O.status != 1 ? temp : last;
    R.err_final = O.status == 1 ? 0.0 : av.eval;
    R.rms_photo = av.photo;
    R.rms_depth = av.depth;
    R.sso = O.status == 1 ? 0.f : sso;
    memcpy(R.iters, O.iters, sizeof(O.iters));
    memcpy(R.hessian, O.H, sizeof(O.H));
    memcpy(R.gradient, O.g, sizeof(O.g));
    if (res) *res = R;
    return O.status;
}

// test hooks (rgbd360_hip_diag.h): the schedules the parity tests compare with the default ones
extern "C" int rgbd360_debug_set_schedule(rgbd360_ctx* ctx, int fused_solve, int fused_occ) {
    if (!ctx) return -1;
    if (ctx->al_active) return fail(ctx, -6, "an alignment is in flight");
    ctx->fused_solve = fused_solve != 0;
    ctx->fused_occ = fused_occ != 0;
    return 0;
}
extern "C" int rgbd360_debug_set_sequence_route(rgbd360_ctx* ctx, int route, int max_contexts) {
    if (!ctx || route < 0 || route > 1 || max_contexts < 0 || max_contexts > 16) return -1;
    ctx->seq_route_contexts = route == 1;
    ctx->seq_route_cap = max_contexts;
    return 0;
}
extern "C" int rgbd360_debug_knobs_enabled(void) { return knobs::debug_build() ? 1 : 0; }

// the Frame360 translation unit's view of a context (f360_state.h)
F360State* rgbd360_ctx_f360(rgbd360_ctx* ctx) {
    if (!ctx->f360) ctx->f360 = f360_state_create(ctx->p.device, ctx->stream);
    return ctx->f360;
}
void rgbd360_ctx_set_error(rgbd360_ctx* ctx, const char* msg) { ctx->err = msg ? msg : ""; }

#include "map_render.h"
#include "frame_store.h"
#include "store_overlap.h"
#include "pose_graph.h"
#include "pose_graph_cov.h"
#include "multi_gpu.h"

