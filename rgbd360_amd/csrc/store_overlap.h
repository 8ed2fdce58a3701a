// store_overlap.h -- sensed-space overlap of stored frames (rgbd360_store_overlap*, include/rgbd360_overlap.h): for a list of (target
// entry, source entry, pose) triples, or for all ordered pairs of a set of entries at their world poses, how much of what the source
// frame senses the target frame senses too.  Included by rgbd360_api.hip behind frame_store.h.
//
// The reference scores a pair by its SSO = visible pixels / image size, a by-product of a finished alignment (RegisterPhotoICP.h:3226;
// used for keyframe selection KFsphere_SLAM.cpp:402-478, for connection scores LoopClosure360.h:321, 360 and for the adjacency
// matrices of TopologicalMap360.h:65, 107-131).  On a 360-degree image nearly every point lands somewhere, so that ratio is close to
// 1 for any two frames of one building.  Here a warped source point only counts as shared space if the target frame sees a surface at
// the same range there.  Per source pixel i of level L, on its own (no z-buffer, no winner rule: the counts do not depend on the order
// of arrival):
//   1 point    the source point of the entry as the per-pixel pass loads it (SrcForm<0> on float4 records, SrcForm<2> / src_point on the
//              compact {depth, I} records); valid iff x != kInvalidPoint                                                    -> n_valid
//   2 warp     warp_images_point<false> (warp_images.h), in the context's index arithmetic: visibility, flat target index ti,
//              range = |R p + t|; valid and visible                                                                         -> n_visible
//   3 target   D = trgD[target entry][ti].a; visible and D finite (RPI.h:3064)                                              -> n_target
//   4 classes  float32, every operation rounded on its own:  diff = range - D,  tol = tol_abs + tol_rel * D
//              |diff| <= tol -> n_consistent;   diff > tol -> n_behind (hidden behind what the target sees);
//              -diff > tol -> n_in_front (the target sees past it)
// All counts are integers: ballots of the predicates, population counts in scalar registers, one integer atomicAdd per counter and
// block (through LDS).  No floating-point atomics, no per-lane atomics.
//
// The all-pairs entry builds its rows on the host (relative poses in float64, see rgbd360_store_overlap_all in
// include/rgbd360_overlap.h) and runs them through the list kernel, or, on levels of kOverlapStationaryMinPx pixels and more, through the
// source-stationary kernel: a block keeps its tile of source b in registers and walks b's targets.  Same per-point function, integer
// counts: a record of the matrix is the record of the list entry, byte for byte.  The stop rule of the design (the second kernel ships
// only where it is at least as fast as the first on the same pairs) and its measurement: profiles/store_overlap_perf.txt.
//
// Out of scope: normalised-cut partitioning of the matrix (TopologicalMap360::Partitioner, MRPT's spectral partition), PbMap guesses,
// occlusion-aware (z-buffered) overlap, distinct-target-pixel coverage, the pinhole and rig paths, several GPUs.
#pragma once

namespace r360 {

constexpr int kOverlapThreads = 256;        // source tile of the list kernel
constexpr int kOverlapCounters = 6;         // n_valid .. n_in_front, in the record's order
constexpr int kOverlapChunk = 32768;        // pairs per launch (grid.y < 65536)

struct OverlapPair {                        // one row of the device table: 80 bytes, read through block-uniform (scalar) loads
    int trg, src, slot, pad;                // slot: the record of the counter array this pair adds into
    float pose[16];
};
struct OverlapTol {
    float abs_, rel;
};

// The six predicates of one source point as wave masks, counted on the scalar unit.
struct OverlapCounts {
    int c[kOverlapCounters];
};
__device__ __forceinline__ void overlap_point(const LevelDev& lv, const PoseRT& T, const float4 s, const bool in_range, const F3* __restrict__ trgD,
                                              const OverlapTol tol, OverlapCounts& acc) {
    unsigned ti;
    float range;
    const PinK K = {0.f, 0.f, 0.f, 0.f};
    const bool seen = warp_images_point<false>(lv, K, T, s, ti, range);      // visible and valid
    const bool valid = in_range && s.x != kInvalidPoint;
    const bool visible = in_range && seen && ti < (unsigned)lv.n;            // (a visible index always lies inside the level)
    const float D = trgD[visible ? ti : 0u].a;                               // one 4-byte gather; lanes without a target read record 0
    const bool target = visible && isfinite(D);
    const float diff = __fsub_rn(range, D);
    const float tl = __fadd_rn(tol.abs_, __fmul_rn(tol.rel, D));
    acc.c[0] += ballot_count(valid);
    acc.c[1] += ballot_count(visible);
    acc.c[2] += ballot_count(target);
    acc.c[3] += ballot_count(target && fabsf(diff) <= tl);
    acc.c[4] += ballot_count(target && diff > tl);
    acc.c[5] += ballot_count(target && -diff > tl);
}

// The block's four waves leave their six counts in LDS; after the barrier lanes 0..5 of the block add the block's totals: one atomic
// instruction per block, one integer add per counter.  buf: which half of the LDS array (a loop alternates, so that one barrier per
// use is enough: a wave can only overwrite a half after the barrier of the use in between, which the reader passes after its reads).
__device__ __forceinline__ void overlap_flush(const OverlapCounts& acc, int32_t* __restrict__ rec, const int buf) {
    __shared__ int s_cnt[2][kOverlapThreads / 64][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int v = acc.c[0];
#pragma unroll
    for (int k = 1; k < kOverlapCounters; ++k) v = lane == k ? acc.c[k] : v;
    if (lane < kOverlapCounters) s_cnt[buf][wave][lane] = v;
    __syncthreads();
    if (threadIdx.x < kOverlapCounters) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < kOverlapThreads / 64; ++w) sum += s_cnt[buf][w][threadIdx.x];
        if (sum != 0) atomicAdd(&rec[1 + threadIdx.x], sum);      // rec[0] is `evaluated`
    }
}

// grid.x: source tiles of 256 pixels, grid.y: pairs of the chunk.  counts: [records][8] int32, cleared on the stream beforehand.
template <int SRC>
__global__ __launch_bounds__(kOverlapThreads) void k_store_overlap(LevelDev lv, const OverlapPair* __restrict__ pairs, OverlapTol tol,
                                                                   int32_t* __restrict__ counts) {
    const OverlapPair* __restrict__ P = pairs + blockIdx.y;                  // block-uniform: scalar loads
    const size_t to = (size_t)P->trg * (size_t)lv.n, so = (size_t)P->src * (size_t)lv.n;
    const int slot = P->slot;
    const PoseRT T = load_pose(P->pose);
    const int base = blockIdx.x * kOverlapThreads;
    const int i = base + (int)threadIdx.x;
    if (SRC == 2) lv.src2 += so;
    SrcCursor cur = {0, 0, 0, 0};
    SrcForm<SRC>::cursor_init(cur, lv, i, kOverlapThreads);
    const typename SrcForm<SRC>::T raw = SrcForm<SRC>::load(lv, SRC == 0 ? lv.src + so : lv.src, lv.n, base, (unsigned)threadIdx.x << 4, cur);
    const float4 s = SrcForm<SRC>::value(raw, lv);
    OverlapCounts acc = {{0, 0, 0, 0, 0, 0}};
    overlap_point(lv, T, s, i < lv.n, lv.trgD + to, tol, acc);
    overlap_flush(acc, counts + (size_t)slot * 8, 0);
}

// Source-stationary form for the all-pairs entry.  grid.x: source tiles, grid.y: segments = the sources that have targets.  A block loads
// its tile of the source ONCE into registers and walks the segment's rows (that source's evaluated targets, consecutive in the table):
// per target the pose and the entry come from scalar loads, then the warp, one 4-byte gather and the ballots.  Same per-point function,
// integer counts: the records are those of k_store_overlap.
struct OverlapSeg {
    int src, first, count, pad;
};
template <int SRC>
__global__ __launch_bounds__(kOverlapThreads) void k_store_overlap_all(LevelDev lv, const OverlapSeg* __restrict__ segs,
                                                                       const OverlapPair* __restrict__ pairs, OverlapTol tol,
                                                                       int32_t* __restrict__ counts) {
    const OverlapSeg* __restrict__ G = segs + blockIdx.y;
    const size_t so = (size_t)G->src * (size_t)lv.n;
    const int first = G->first, count = G->count;
    const int base = blockIdx.x * kOverlapThreads;
    const int i = base + (int)threadIdx.x;
    if (SRC == 2) lv.src2 += so;
    SrcCursor cur = {0, 0, 0, 0};
    SrcForm<SRC>::cursor_init(cur, lv, i, kOverlapThreads);
    const typename SrcForm<SRC>::T raw = SrcForm<SRC>::load(lv, SRC == 0 ? lv.src + so : lv.src, lv.n, base, (unsigned)threadIdx.x << 4, cur);
    const float4 s = SrcForm<SRC>::value(raw, lv);
    const bool in_range = i < lv.n;
    for (int j = 0; j < count; ++j) {
        const OverlapPair* __restrict__ P = pairs + first + j;
        const PoseRT T = load_pose(P->pose);
        OverlapCounts acc = {{0, 0, 0, 0, 0, 0}};
        overlap_point(lv, T, s, in_range, lv.trgD + (size_t)P->trg * (size_t)lv.n, tol, acc);
        overlap_flush(acc, counts + (size_t)P->slot * 8, j & 1);
    }
}

}  // namespace r360

namespace {

using r360::OverlapPair;

// rgbd360_store_overlap_all runs the source-stationary kernel on levels of at least this many pixels, the list kernel below.  Measured
// on 992 pairs (profiles/store_overlap_perf.txt): level with the list kernel at 32 768 pixels, 1.44 - 1.91 x faster from 131 072; the
// bound between the two measured sizes is a choice.
constexpr int kOverlapStationaryMinPx = 65536;

int overlap_check_params(rgbd360_store* st, const rgbd360_overlap_params* p) {
    if (!p) return store_fail(st, -1, "null overlap parameters");
    if (p->level < 0 || p->level >= st->p.n_pyr) return store_fail(st, -3, "bad pyramid level");
    if (!(p->tol_abs >= 0.f) || !(p->tol_rel >= 0.f) || !std::isfinite(p->tol_abs) || !std::isfinite(p->tol_rel))
        return store_fail(st, -1, "overlap tolerances must be finite and >= 0");
    return 0;
}

int overlap_check_entry(rgbd360_store* st, int k, const char* what, int e) {
    if (e < 0 || e >= st->capacity)
        return store_fail(st, -1, "pair " + std::to_string(k) + ": " + what + " entry " + std::to_string(e) + " is outside the store");
    if (!st->occupied[e]) return store_fail(st, -1, "pair " + std::to_string(k) + ": " + what + " entry " + std::to_string(e) + " is empty");
    return 0;
}

LevelDev overlap_level_dev(rgbd360_store* st, int level) {
    const SeqLevel& L = st->put_eng->levels[level];
    LevelDev lv = seq_level_dev(L, 0);
    const StoreLevelView& V = st->view.levels[level];
    lv.src = V.src; lv.src2 = reinterpret_cast<const float2*>(V.src); lv.trgP = V.trgP; lv.trgD = V.trgD;
    lv.min_depth = st->p.min_depth; lv.max_depth = st->p.max_depth;
    lv.libm = st->ctx->index_libm;
    return lv;
}

// n_segs > 0: the source-stationary kernel over the table's segments
void overlap_launch(rgbd360_store* st, int level, const r360::OverlapTol tol, int n_rows, int n_segs) {
    SeqEngine* E = st->put_eng;
    const SeqLevel& L = E->levels[level];
    const LevelDev lv = overlap_level_dev(st, level);
    const OverlapPair* table = reinterpret_cast<const OverlapPair*>(st->ov_table.get());
    if (n_segs > 0) {
        const r360::OverlapSeg* segs = reinterpret_cast<const r360::OverlapSeg*>(st->ov_segs.get());
        for (int k = 0; k < n_segs; k += r360::kOverlapChunk) {
            const dim3 g((L.n + r360::kOverlapThreads - 1) / r360::kOverlapThreads, std::min(r360::kOverlapChunk, n_segs - k));
            if (L.compact)
                hipLaunchKernelGGL((r360::k_store_overlap_all<2>), g, dim3(r360::kOverlapThreads), 0, E->stream, lv, segs + k, table, tol, st->ov_counts.get());
            else
                hipLaunchKernelGGL((r360::k_store_overlap_all<0>), g, dim3(r360::kOverlapThreads), 0, E->stream, lv, segs + k, table, tol, st->ov_counts.get());
        }
        return;
    }
    for (int k = 0; k < n_rows; k += r360::kOverlapChunk) {
        const dim3 g((L.n + r360::kOverlapThreads - 1) / r360::kOverlapThreads, std::min(r360::kOverlapChunk, n_rows - k));
        if (L.compact)
            hipLaunchKernelGGL((r360::k_store_overlap<2>), g, dim3(r360::kOverlapThreads), 0, E->stream, lv, table + k, tol, st->ov_counts.get());
        else
            hipLaunchKernelGGL((r360::k_store_overlap<0>), g, dim3(r360::kOverlapThreads), 0, E->stream, lv, table + k, tol, st->ov_counts.get());
    }
}

// rows: the pairs to evaluate, row.slot the record each adds into; n_records records come back (records no row names stay zero).
// reps / kernel_us: the measurement entry runs the launches `reps` times between events (counters cleared before each).
// stationary: rows are grouped by source; one segment per run of equal sources, walked by k_store_overlap_all.
int overlap_run(rgbd360_store* st, const std::vector<OverlapPair>& rows, int n_records, const rgbd360_overlap_params& p, rgbd360_overlap* out,
                int reps = 1, float* kernel_us = nullptr, bool stationary = false) {
    SeqEngine* E = st->put_eng;
    hipSetDevice(st->p.device);
    const int n_rows = (int)rows.size();
    const size_t count_bytes = (size_t)n_records * sizeof(rgbd360_overlap);
    static_assert(sizeof(rgbd360_overlap) == 8 * sizeof(int32_t), "the record is eight int32");
    if (n_rows) {
        SEQC(E, st->ov_table.ensure((size_t)n_rows * sizeof(OverlapPair)));
        SEQC(E, st->ov_counts.ensure((size_t)n_records * 8));
        SEQC(E, hipMemcpyAsync(st->ov_table.get(), rows.data(), (size_t)n_rows * sizeof(OverlapPair), hipMemcpyHostToDevice, E->stream));
        std::vector<r360::OverlapSeg> segs;
        if (stationary) {
            for (int k = 0; k < n_rows; ++k) {
                if (segs.empty() || segs.back().src != rows[k].src) segs.push_back(r360::OverlapSeg{rows[k].src, k, 0, 0});
                ++segs.back().count;
            }
            SEQC(E, st->ov_segs.ensure(segs.size() * sizeof(r360::OverlapSeg)));
            SEQC(E, hipMemcpyAsync(st->ov_segs.get(), segs.data(), segs.size() * sizeof(r360::OverlapSeg), hipMemcpyHostToDevice, E->stream));
        }
        const r360::OverlapTol tol = {p.tol_abs, p.tol_rel};
        hipEvent_t ev[2] = {nullptr, nullptr};
        if (kernel_us) { SEQC(E, hipEventCreate(&ev[0])); SEQC(E, hipEventCreate(&ev[1])); }
        for (int r = 0; r < reps; ++r) {
            SEQC(E, hipMemsetAsync(st->ov_counts.get(), 0, count_bytes, E->stream));
            if (kernel_us) SEQC(E, hipEventRecord(ev[0], E->stream));
            overlap_launch(st, p.level, tol, n_rows, (int)segs.size());
            SEQC(E, hipGetLastError());
            if (kernel_us) {
                SEQC(E, hipEventRecord(ev[1], E->stream));
                SEQC(E, hipEventSynchronize(ev[1]));
                float ms = 0.f;
                SEQC(E, hipEventElapsedTime(&ms, ev[0], ev[1]));
                kernel_us[r] = ms * 1000.f;
            }
        }
        if (kernel_us) { hipEventDestroy(ev[0]); hipEventDestroy(ev[1]); }
        SEQC(E, hipMemcpyAsync(out, st->ov_counts.get(), count_bytes, hipMemcpyDeviceToHost, E->stream));
        SEQC(E, hipStreamSynchronize(E->stream));
    } else {
        memset(out, 0, count_bytes);
    }
    for (const OverlapPair& r : rows) out[r.slot].evaluated = 1;
    return 0;
}

// T_ab = W_a^-1 W_b in float64 from the float32 inputs (the formula of the header, operation for operation); returns |t_ab|.
double overlap_rel_pose(const float* Wa, const float* Wb, float out[16]) {
    auto A = [&](int r, int c) { return (double)Wa[c * 4 + r]; };
    auto B = [&](int r, int c) { return (double)Wb[c * 4 + r]; };
    double t[3];
    for (int r = 0; r < 3; ++r) {
        const double it = -((A(0, r) * A(0, 3) + A(1, r) * A(1, 3)) + A(2, r) * A(2, 3));
        for (int c = 0; c < 3; ++c) out[c * 4 + r] = (float)((A(0, r) * B(0, c) + A(1, r) * B(1, c)) + A(2, r) * B(2, c));
        t[r] = ((A(0, r) * B(0, 3) + A(1, r) * B(1, 3)) + A(2, r) * B(2, 3)) + it;
        out[12 + r] = (float)t[r];
    }
    out[3] = out[7] = out[11] = 0.f;
    out[15] = 1.f;
    return std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
}

int overlap_list(rgbd360_store* st, int n_pairs, const int* trg, const int* src, const float* poses, const rgbd360_overlap_params* params,
                 rgbd360_overlap* out, int reps, float* kernel_us) {
    if (!st) return -1;
    if (n_pairs < 0) return store_fail(st, -1, "n_pairs must be >= 0");
    int rc = overlap_check_params(st, params);
    if (rc) return rc;
    if (n_pairs == 0) return 0;
    if (!trg || !src || !out) return store_fail(st, -1, "null pointer");
    for (int k = 0; k < n_pairs; ++k)      // all of them, before anything is launched
        if ((rc = overlap_check_entry(st, k, "target", trg[k])) != 0 || (rc = overlap_check_entry(st, k, "source", src[k])) != 0) return rc;
    std::vector<OverlapPair> rows(n_pairs);
    for (int k = 0; k < n_pairs; ++k) {
        rows[k].trg = trg[k]; rows[k].src = src[k]; rows[k].slot = k; rows[k].pad = 0;
        memcpy(rows[k].pose, poses ? poses + (size_t)16 * k : kIdentityPose, sizeof(rows[k].pose));
    }
    rc = overlap_run(st, rows, n_pairs, *params, out, reps, kernel_us);
    if (rc) { (void)hipStreamSynchronize(st->put_eng->stream); return store_fail(st, rc, st->put_eng->err); }
    return 0;
}

int overlap_all(rgbd360_store* st, int n, const int* entries, const float* world_poses, float max_translation, const rgbd360_overlap_params* params,
                rgbd360_overlap* out, float* rel_poses_out, int reps, float* kernel_us, int kernel /* 0 list, 1 source-stationary, -1 by size */) {
    if (!st) return -1;
    if (n < 0) return store_fail(st, -1, "n must be >= 0");
    int rc = overlap_check_params(st, params);
    if (rc) return rc;
    if (n == 0) return 0;
    if (n > 46340) return store_fail(st, -1, "too many entries for one matrix");
    if (!entries || !world_poses || !out) return store_fail(st, -1, "null pointer");
    {
        std::vector<char> seen(st->capacity, 0);
        for (int k = 0; k < n; ++k) {
            if ((rc = overlap_check_entry(st, k, "matrix", entries[k])) != 0) return rc;
            if (seen[entries[k]]) return store_fail(st, -1, "entry " + std::to_string(entries[k]) + " is named twice");
            seen[entries[k]] = 1;
        }
    }
    const bool all = !(max_translation > 0.f) || !std::isfinite(max_translation);
    const bool stationary = kernel < 0 ? st->put_eng->levels[params->level].n >= kOverlapStationaryMinPx : kernel == 1;
    std::vector<OverlapPair> rows;
    rows.reserve((size_t)n * (n - 1));
    for (int u = 0; u < n; ++u)
        for (int v = 0; v < n; ++v) {
            const int a = stationary ? v : u, b = stationary ? u : v;      // the stationary kernel wants a source's targets side by side
            OverlapPair r;
            r.trg = entries[a]; r.src = entries[b]; r.slot = a * n + b; r.pad = 0;
            const double dist = overlap_rel_pose(world_poses + (size_t)16 * a, world_poses + (size_t)16 * b, r.pose);
            if (rel_poses_out) memcpy(rel_poses_out + (size_t)16 * r.slot, r.pose, sizeof(r.pose));
            if (a != b && (all || dist <= (double)max_translation)) rows.push_back(r);
        }
    rc = overlap_run(st, rows, n * n, *params, out, reps, kernel_us, stationary);
    if (rc) { (void)hipStreamSynchronize(st->put_eng->stream); return store_fail(st, rc, st->put_eng->err); }
    return 0;
}

}  // namespace

extern "C" {

void rgbd360_store_overlap_default_params(const rgbd360_store* st, rgbd360_overlap_params* p) {
    if (!p) return;
    p->level = st ? st->p.n_pyr - 1 : 0;
    p->tol_abs = 0.05f;
    p->tol_rel = 0.02f;      // the project's max_depth_change_factor
}

int rgbd360_store_overlap(rgbd360_store* st, int n_pairs, const int* trg, const int* src, const float* poses, const rgbd360_overlap_params* params,
                          rgbd360_overlap* out) {
    return overlap_list(st, n_pairs, trg, src, poses, params, out, 1, nullptr);
}

int rgbd360_store_overlap_all(rgbd360_store* st, int n, const int* entries, const float* world_poses, float max_translation,
                              const rgbd360_overlap_params* params, rgbd360_overlap* out, float* rel_poses_out) {
    return overlap_all(st, n, entries, world_poses, max_translation, params, out, rel_poses_out, 1, nullptr, -1);
}

// rgbd360_hip_diag.h: the same two calls with the kernel launches of a call repeated `reps` times between HIP events
int rgbd360_store_time_overlap(rgbd360_store* st, int n_pairs, const int* trg, const int* src, const float* poses,
                               const rgbd360_overlap_params* params, int reps, float* kernel_us, rgbd360_overlap* out) {
    if (reps < 1 || !kernel_us) return -1;
    return overlap_list(st, n_pairs, trg, src, poses, params, out, reps, kernel_us);
}

int rgbd360_store_time_overlap_all(rgbd360_store* st, int n, const int* entries, const float* world_poses, float max_translation,
                                   const rgbd360_overlap_params* params, int kernel, int reps, float* kernel_us, rgbd360_overlap* out) {
    if (reps < 1 || !kernel_us || kernel < 0 || kernel > 1) return -1;
    return overlap_all(st, n, entries, world_poses, max_translation, params, out, nullptr, reps, kernel_us, kernel);
}

}  // extern "C"
