// map_align.h -- point-to-point ICP of a posed sphere frame, or of a cloud, against the resident voxel map (voxel_map.h): the
// cloud-to-cloud ICP the reference's registration programs put next to the dense alignment
//   filter.filterVoxel(cloud); icp.setInputSource(src); icp.setInputTarget(trg); icp.align(*aligned, guess);
// (RegisterPairRGBD360.cpp:111-118, MethodsRegisterRGBD360.cpp:294-320, OdometryRGBD360.cpp:98-114, 210-222,
// OdometryKeyFrame360.cpp:124-140) with the map as its target.  Part of the Frame360 translation unit, behind voxel_map.h and gn_math.h.
//
// Definition (include/rgbd360_hip.h, "point-to-point ICP of a frame against the map"; tests/map_align_reference.py
// restates it in numpy).  Per source point at the current pose: steps 1-5 of the map through vmap::classify; the 27 cells around the
// point's voxel, the centre first, then dz / dy / dx ascending; per cell found with count >= min_count the read-out's centroid, e = w - c
// and d2 in float32; the smallest d2 wins, a tie goes to the earlier cell; kept iff d2 <= max_dist^2; 17 float64 sums over the kept
// matches; H and g of J = [I | -[w]x] from the sums, gn::step, the stop tests.  max_dist lies in (0, leaf]: the 27 cells then hold every
// centroid closer than max_dist (up to rounding at cell faces -- a centroid may lie an ulp outside its cell), so the match is the true
// nearest centroid; a larger radius would need (2r + 1)^3 probes, callers who need a wider basin align against a coarser map first.
// No cell is pruned: all 27 are looked up whatever the point's place in its cell.
//
// This header also holds what every method of alignment against the map shares (map_align_plane.h is the second method,
// map_align_gicp.h the third, map_align_colour.h the fourth): the evaluation (eval_tile<M, SRC, OUT> and its two kernels, k_vmap_eval<M, SRC>
// here and k_vmap_eval_batch<M, SRC> in map_align_batch.h), the loop's state, init and solve (LoopState<WORDS>, icp_init_state,
// icp_solve_rows<M>, k_vmap_icp_init<WORDS>, k_vmap_icp_solve<M>) and the host driver (icp_prepare, icp_launch_eval<M>, icp_enqueue<M>,
// icp_align<M>, icp_eval<M>; the input of a call is voxel_map.h's MapInput).  A method is a row description with its Support, Args and
// Tail (PointMethod) and a host description (PointIcp).  eval_tile is built from three shared pieces: the source load
// (vmap::load_points, voxel_map.h, also k_vmap_insert's), the candidate search (vmap::search27 with the method's Support) and the block
// epilogue (vmap::block_row_sum); a method's own text is its per-point tail.  tests/test_map_align_bits_gpu.py pins the bytes of all four.
//
//   k_vmap_eval       the shape of k_vmap_insert: 256 threads, four points per thread 256 apart, all loads of a thread first
//                     (load_points).  Per point search27: the first probe of all 27 cells is loaded before any is looked at (27
//                     independent 8-byte loads in flight); a probe sequence goes on with plain loads.  The table is never written.
//                     block_row_sum: a wave's row (point-to-point: 22 doubles -- 17 sums, three counters, the probe and search counts)
//                     goes through a butterfly of lane exchanges, the four waves through LDS, and the workgroup writes one partial row.
//                     The pose comes from the loop's state in device memory; a launch of the loop returns at once when the state says
//                     the loop has ended.  (The measurement tools print it under the labels k_vmap_icp_eval, k_vmap_plane_eval,
//                     k_vmap_gicp_eval and k_vmap_colour_eval, one per method, as earlier profiles do.)
//   k_vmap_icp_solve  one workgroup: the rows added in ascending order (one lane per column), H and g, gn::step, status and the stop
//                     test, one trace record per applied step, the new pose and the state word.
//   host              max_iters x (eval, solve), the final eval and its solve, one copy of the state, ONE synchronisation; no host read
//                     between iterations.
// Cost: up to 27 dependent-free first probes of 8 bytes per point against random 64-byte slots, plus 32 bytes per occupied candidate;
// tools/map_align_perf.py measures it (profiles/map_align_perf.txt).
#pragma once
#include <chrono>

namespace vmap {

constexpr int kIcpSums = 17;
constexpr int kIcpWords = 22;        // a partial row: the 17 sums, n_valid, n_box_rejected, n_out_of_range, probes, points searched (all doubles: exact integers)
constexpr int kIcpMaxWords = 40;     // the widest row of any method (the robust rows of map_align_gicp.h and map_align_colour.h): the buffers of a map serve every method
constexpr int kIcpMaxIters = 1000;
constexpr int kNoKey = -2147483647 - 1;

// the loop's state in device memory, the trace behind it; WORDS: the method's row
template <int WORDS>
struct LoopState {
    float pose[16];
    int done, status, iterations, converged;
    double row[WORDS];               // the totals of the last evaluation that was summed
    float H[36], g[6];
};
struct IcpPose {
    float m[16];
};

// (the read-only lookup vmap::find: map_table.h)

// cell c of the 27 in the definition's order: 0 the centre, then dz, dy, dx ascending without the centre
__host__ __device__ inline void icp_cell(int c, int& dx, int& dy, int& dz) {
    int q = c == 0 ? 13 : c <= 13 ? c - 1 : c;      // position in the nested loops (13 = the centre)
    dx = q % 3 - 1;
    dy = q / 3 % 3 - 1;
    dz = q / 9 - 1;
}

// The candidate search of every method: the 27 cells around the voxel `key` of the posed point w, in icp_cell's order.  The first probe of
// all 27 is loaded before any is looked at (27 independent 8-byte loads in flight; a cell outside the 21-bit range has no key and costs
// no probe); then per cell vmap::find, count >= min_count, the read-out's centroid cf, e = w - cf and d2 in float32; the smallest d2 wins,
// a tie stays with the earlier cell.  A method's Support sees every candidate after that comparison: nothing for point-to-point, the
// nine support sums for point-to-plane (map_align_plane.h).  This one function is why both methods match the same key with the same d2.
struct NoSupport {
    __device__ __forceinline__ void add(const float*, const float*) {}
};
template <class Support>
struct Match {
    float best = __builtin_inff();           // d2 of the nearest candidate, its key (kEmpty: none), its slot and e = w - its centroid
    unsigned long long best_key = kEmpty;
    long long best_slot = -1;                // (read by map_align_gicp.h alone: the normal layer's record of the match)
    float be[3] = {0.f, 0.f, 0.f};
    Support support;
};
template <class Support>
__device__ __forceinline__ Match<Support> search27(const unsigned long long* __restrict__ table, unsigned long long mask, unsigned long long min_count,
                                                   unsigned long long key, const float w[3], unsigned& n_probes) {
#pragma clang fp contract(off)
    Match<Support> mt;
    const long long ib[3] = {(long long)(key & 0x1fffffull), (long long)((key >> 21) & 0x1fffffull), (long long)(key >> 42)};
    unsigned long long k0[27];
#pragma unroll
    for (int c = 0; c < 27; ++c) {
        int dx, dy, dz;
        icp_cell(c, dx, dy, dz);
        const long long nx = ib[0] + dx, ny = ib[1] + dy, nz = ib[2] + dz;
        const bool ok = nx >= 0 && nx < (1ll << 21) && ny >= 0 && ny < (1ll << 21) && nz >= 0 && nz < (1ll << 21);
        k0[c] = ok ? table[(mix64(pack_key(nx, ny, nz)) & mask) * kFields] : kEmpty;
        n_probes += ok ? 1u : 0u;
    }
#pragma unroll
    for (int c = 0; c < 27; ++c) {
        if (k0[c] == kEmpty) continue;       // an empty first slot, or no key at all: no candidate
        int dx, dy, dz;
        icp_cell(c, dx, dy, dz);
        const unsigned long long ck = pack_key(ib[0] + dx, ib[1] + dy, ib[2] + dz);
        const long long slot = find(table, mask, ck, mix64(ck) & mask, k0[c], n_probes);
        if (slot < 0) continue;
        const unsigned long long* rec = table + (unsigned long long)slot * kFields;
        const unsigned long long cnt = rec[1];
        if (cnt < min_count || cnt == 0) continue;
        float cf[3], e[3];
        centroid(rec, cnt, cf);
#pragma unroll
        for (int q = 0; q < 3; ++q) e[q] = w[q] - cf[q];
        const float d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        if (d2 < mt.best) {
            mt.best = d2;
            mt.best_key = ck;
            mt.best_slot = slot;
            mt.be[0] = e[0];
            mt.be[1] = e[1];
            mt.be[2] = e[2];
        }
        mt.support.add(w, cf);
    }
    return mt;
}

// The epilogue of an evaluation kernel: the thread's row summed over the wave (a butterfly, lane offsets 32 .. 1), the four waves
// through LDS in ascending order, one partial row per workgroup -- a fixed tree, the same sums from run to run.
template <int WORDS>
__device__ __forceinline__ void block_row_sum(double row[WORDS], double (*s_red)[WORDS], double* __restrict__ part_row) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < WORDS; ++q) {
#pragma unroll
        for (int off = 32; off; off >>= 1) row[q] += __shfl_xor(row[q], off);
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int q = 0; q < WORDS; ++q) s_red[t >> 6][q] = row[q];
    }
    __syncthreads();
    if (t < WORDS) {
        double s = s_red[0][t];
        for (int wv = 1; wv < kThreads / 64; ++wv) s += s_red[wv][t];
        part_row[t] = s;
    }
}
// the workgroup's partial row: a row per tile of an image row (SRC 0), per tile of the cloud (SRC 1)
template <int SRC>
__device__ __forceinline__ size_t block_row() {
    return SRC == 0 ? (size_t)blockIdx.y * gridDim.x + blockIdx.x : (size_t)blockIdx.x;
}
// the per-point key output: the matched voxel's indices, kNoKey x 3 without a kept match
__device__ __forceinline__ void store_key3(int32_t* __restrict__ key3, unsigned long long best_key, bool kept) {
    int32_t i3[3];
    unpack_key3(best_key, i3);
#pragma unroll
    for (int q = 0; q < 3; ++q) key3[q] = kept ? i3[q] : kNoKey;
}

// H (column-major) and g of J = [I | -[w]x] from the 17 sums
__host__ __device__ inline void icp_assemble(const double* s, float* H, float* g) {
    const double n = s[0], wx = s[1], wy = s[2], wz = s[3], xx = s[4], xy = s[5], xz = s[6], yy = s[7], yz = s[8], zz = s[9];
    const double Hd[6][6] = {{n, 0, 0, 0, wz, -wy},   {0, n, 0, -wz, 0, wx},    {0, 0, n, wy, -wx, 0},
                             {0, -wz, wy, yy + zz, -xy, -xz}, {wz, 0, -wx, -xy, xx + zz, -yz}, {-wy, wx, 0, -xz, -yz, xx + yy}};
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) H[c * 6 + r] = (float)Hd[r][c];
    for (int k = 0; k < 6; ++k) g[k] = (float)s[10 + k];
}

// What every evaluation takes besides its method's own arguments: the table, the match rule, the per-point outputs of every method
// (tests; either may be null): the matched voxel's indices and d2.
struct EvalCommon {
    const unsigned long long* table;
    unsigned long long mask, min_count;
    float max_dist2;
    int32_t* key3;
    float* d2_out;
};

// One workgroup's tile (bx, of image row by) of a source at the pose in P into one partial row: the evaluation of every method M, in the
// single kernel and in the batched one, so that a tile gives the same row in both.  M is a row description: its places (kWords,
// kCounters, kProbes, kSearched), the Support its search27 carries, its Args (a plain struct: its parameters and its extra per-point
// output pointers) and its Tail, the per-thread object that is the method's own text:
//   begin<SRC>(src, by)                    what it needs of the source beyond the points (coloured ICP: where the row's colours are)
//   add(index, pose, w, match, kept, a)    a point of the thread into its sums and own counters
//   store(index, a)                        that point's extra outputs
//   row(out)                               its sums and own counters into the row
// OUT: whether the per-point outputs exist at all (the batch has none: what only they need is then not kept).
template <class M, int SRC, bool OUT>
__device__ __forceinline__ void eval_tile(const Params& P, const Source& src, unsigned bx, unsigned by, const EvalCommon& c, const typename M::Args& a,
                                          double (*s_red)[M::kWords], double* __restrict__ part_row) {
#pragma clang fp contract(off)
    float x[kPerThread], y[kPerThread], z[kPerThread];
    bool in[kPerThread];
    long long index[kPerThread];
    load_points<SRC>(src, bx, by, x, y, z, in, index);
    typename M::Tail tail;
    tail.template begin<SRC>(src, by);

    unsigned n_probes = 0, n_valid = 0, n_box = 0, n_range = 0, n_searched = 0;      // (integers until the reduction)
    // one point after another through the one accumulator
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (!in[k]) continue;
        unsigned long long key = 0;
        long long f[3];
        float w[3];
        const int cls = classify(P, x[k], y[k], z[k], key, f, w);
        n_valid += cls >= 1 ? 1u : 0u;
        n_box += cls == 1 ? 1u : 0u;
        n_range += cls == 2 ? 1u : 0u;
        Match<typename M::Support> mt;
        if (cls == 3) {
            n_searched += 1u;
            mt = search27<typename M::Support>(c.table, c.mask, c.min_count, key, w, n_probes);
        }
        const bool kept = mt.best_key != kEmpty && mt.best <= c.max_dist2;
        if (OUT && c.key3) store_key3(c.key3 + 3 * index[k], mt.best_key, kept);
        if (OUT && c.d2_out) c.d2_out[index[k]] = mt.best;
        tail.add(index[k], P.pose, w, mt, kept, a);
        if (OUT) tail.store(index[k], a);
    }

    double row[M::kWords];
    tail.row(row);
    row[M::kCounters] = (double)n_valid;
    row[M::kCounters + 1] = (double)n_box;
    row[M::kCounters + 2] = (double)n_range;
    row[M::kProbes] = (double)n_probes;
    row[M::kSearched] = (double)n_searched;
    block_row_sum<M::kWords>(row, s_red, part_row);
}

// a tail that needs nothing of the source beyond the points
struct PointsOnly {
    template <int SRC>
    __device__ __forceinline__ void begin(const Source&, unsigned) {}
};

// The weight of a point in its method's sums: a tail is written once, over a weight policy.  A tail calls clear() per point, set(s, args)
// before its accumulation block with s the point's cost term AS A CALLABLE (one text: the expression the quadratic tail adds to its cost
// word), adds wt(t) for every term t in front of the cost word and rho(s) into the cost word, and hands store() and row() on.  UnitWeight
// is the quadratic cost: set() is nothing, wt(t) is t and rho(s) evaluates s where the tail always evaluated it, so the tail over it is
// the machine code it was before there were policies (tools/device_asm_diff.py).  RobustWeight evaluates s in set().  RobustWeight (include/rgbd360_hip.h, "robust kernels of the alignments against the
// map") takes w and rho from gn::robust_rho_w -- the pose graph's text -- under the launch's kind and delta; one double,
// w, is live across the accumulation block.  It counts the contributing points and those with w < 1: the two words a robust row has behind
// its method's.
struct UnitWeight {
    __device__ __forceinline__ void clear() {}
    template <class S, class Args>
    __device__ __forceinline__ void set(const S&, const Args&) {}
    __device__ __forceinline__ double operator()(double t) const { return t; }
    template <class S>
    __device__ __forceinline__ double rho(const S& s) const { return s(); }
    template <class Args>
    __device__ __forceinline__ void store(long long, const Args&) const {}
    __device__ __forceinline__ void row(double*) const {}
};
struct RobustWeight {
    double w = 0.0, rho_s = 0.0;     // of the point added last (w = 0: it does not contribute)
    unsigned n = 0, n_down = 0;
    __device__ __forceinline__ void clear() { w = 0.0; }
    template <class S, class Args>
    __device__ __forceinline__ void set(const S& s, const Args& a) {
        gn::robust_rho_w(a.kind, a.delta, s(), &rho_s, &w);
        n += 1u;
        n_down += w < 1.0 ? 1u : 0u;
    }
    __device__ __forceinline__ double operator()(double t) const {
#pragma clang fp contract(off)
        return w * t;
    }
    template <class S>
    __device__ __forceinline__ double rho(const S&) const { return rho_s; }
    template <class Args>
    __device__ __forceinline__ void store(long long index, const Args& a) const {
        if (a.w_out) a.w_out[index] = w;
    }
    __device__ __forceinline__ void row(double* out) const {
        out[0] = (double)n;
        out[1] = (double)n_down;
    }
};

// point-to-point's tail: the 17 sums of a kept match
template <class W>
struct PointTailT : PointsOnly {
    double acc[kIcpSums];
    W wt;
    __device__ __forceinline__ PointTailT() {
#pragma unroll
        for (int q = 0; q < kIcpSums; ++q) acc[q] = 0.0;
    }
    template <class Args>
    __device__ __forceinline__ void add(long long, const float*, const float w[3], const Match<NoSupport>& mt, bool kept, const Args& args) {
#pragma clang fp contract(off)
        wt.clear();
        if (kept) {
            const double wx = w[0], wy = w[1], wz = w[2], ex = mt.be[0], ey = mt.be[1], ez = mt.be[2];
            const auto s = [&] { return (ex * ex + ey * ey) + ez * ez; };
            wt.set(s, args);
            acc[0] += wt(1.0);
            acc[1] += wt(wx);
            acc[2] += wt(wy);
            acc[3] += wt(wz);
            acc[4] += wt(wx * wx);
            acc[5] += wt(wx * wy);
            acc[6] += wt(wx * wz);
            acc[7] += wt(wy * wy);
            acc[8] += wt(wy * wz);
            acc[9] += wt(wz * wz);
            acc[10] += wt(ex);
            acc[11] += wt(ey);
            acc[12] += wt(ez);
            acc[13] += wt(wy * ez - wz * ey);
            acc[14] += wt(wz * ex - wx * ez);
            acc[15] += wt(wx * ey - wy * ex);
            acc[16] += wt.rho(s);
        }
    }
    template <class Args>
    __device__ __forceinline__ void store(long long index, const Args& args) const { wt.store(index, args); }
    __device__ __forceinline__ void row(double* out) const {
#pragma unroll
        for (int q = 0; q < kIcpSums; ++q) out[q] = acc[q];
        wt.row(out + kIcpWords);
    }
};
using PointTail = PointTailT<UnitWeight>;

// What the loop and the evaluation need to know of a method: the row's width, where n and the traced sum of squares are, where the
// counters start (the sums lie in front of them: n_valid, n_box_rejected, n_out_of_range, the method's own, then probes and points
// searched), H and g; and eval_tile's Support, Args and Tail (TailT: the tail over a weight policy).
struct PointMethod {
    static constexpr int kWords = kIcpWords, kN = 0, kSumSq = 16, kCounters = 17, kProbes = 20, kSearched = 21;
    __host__ __device__ static void assemble(const double* s, float* H, float* g) { icp_assemble(s, H, g); }
    using Support = NoSupport;
    struct Args {};
    using Tail = PointTail;
    template <class W>
    using TailT = PointTailT<W>;
};

// The robust form of a method M: M's row with two words behind it -- the contributing points (the row's kN: min_matches, n_matched, the
// trace's n and the fitness count them, word 0 holds sum w) and those with w < 1 -- M's tail over RobustWeight, M's assemble.  kind and
// delta are runtime values, uniform over the launch: one instantiation per method.  w_out (tests; may be null): w per input point, 0.0
// for a point that does not contribute.
template <class M>
struct Robust {
    static constexpr int kWords = M::kWords + 2, kN = M::kWords, kDown = M::kWords + 1, kSumSq = M::kSumSq, kCounters = M::kCounters,
                         kProbes = M::kProbes, kSearched = M::kSearched;
    __host__ __device__ static void assemble(const double* s, float* H, float* g) { M::assemble(s, H, g); }
    using Support = typename M::Support;
    struct Args : M::Args {
        int kind;
        double delta;
        double* w_out;
    };
    using Tail = typename M::template TailT<RobustWeight>;
};
static_assert(Robust<PointMethod>::kWords <= kIcpMaxWords, "the buffers of a map hold the widest row");

template <int WORDS>
__device__ __forceinline__ void icp_init_state(LoopState<WORDS>* __restrict__ st, const float* guess) {
    const int t = threadIdx.x;
    if (t < 16) st->pose[t] = guess[t];
    if (t < WORDS) st->row[t] = 0.0;
    if (t < 36) st->H[t] = 0.f;
    if (t < 6) st->g[t] = 0.f;
    if (t == 0) st->done = st->status = st->iterations = st->converged = 0;
}
template <int WORDS>
__global__ void k_vmap_icp_init(LoopState<WORDS>* __restrict__ st, IcpPose guess) {
    icp_init_state(st, guess.m);
}

// the evaluation of the loop: the pose comes from the loop's state; a launch returns at once when the state says the loop has ended
template <class M, int SRC>
__global__ __launch_bounds__(kThreads) void k_vmap_eval(Params P, Source src, EvalCommon c, typename M::Args a, const LoopState<M::kWords>* __restrict__ st,
                                                        int final_pass, double* __restrict__ part) {
#pragma clang fp contract(off)
    if (!final_pass && st->done) return;
    __shared__ double s_red[kThreads / 64][M::kWords];
#pragma unroll
    for (int k = 0; k < 16; ++k) P.pose[k] = st->pose[k];
    eval_tile<M, SRC, true>(P, src, blockIdx.x, blockIdx.y, c, a, s_red, part + block_row<SRC>() * M::kWords);
}

// The solve of one alignment (the single kernel's, a job's of the batched one): the rows added in ascending order (one lane per column),
// then lane 0: H and g, gn::step, status and the stop test, one trace record per applied step, the new pose and the state word
template <class M>
__device__ __forceinline__ void icp_solve_rows(LoopState<M::kWords>* __restrict__ st, rgbd360_map_align_trace* __restrict__ trace, const double* __restrict__ part,
                                               int n_rows, int final_pass, long long min_matches, float eps, double* s_row) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    if (t < M::kWords) {         // the rows in ascending order
        double s = 0.0;
        for (int r = 0; r < n_rows; ++r) s += part[(size_t)r * M::kWords + t];
        s_row[t] = s;
        st->row[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    const long long n = (long long)s_row[M::kN];
    if (final_pass) {
        M::assemble(s_row, st->H, st->g);
        if (st->status == RGBD360_OK && n < min_matches) st->status = RGBD360_NO_VALID_PIXELS;
        st->done = 1;
        return;
    }
    if (n < min_matches) {
        st->status = RGBD360_NO_VALID_PIXELS;
        st->done = 1;
        return;
    }
    float H[36], g[6], pose[16], pose_new[16], u[6];
    M::assemble(s_row, H, g);
    for (int k = 0; k < 16; ++k) pose[k] = st->pose[k];
    if (gn::step(H, g, 0.f, pose, pose_new, u) != 0) {
        st->status = RGBD360_ILL_POSED;
        st->done = 1;
        return;
    }
    for (int k = 0; k < 16; ++k) st->pose[k] = pose_new[k];
    rgbd360_map_align_trace rec;
    rec.n = n;
    rec.sum_sq = s_row[M::kSumSq];
    for (int k = 0; k < 6; ++k) rec.update[k] = u[k];
    trace[st->iterations] = rec;
    st->iterations += 1;
    const float vv = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2], ww = (u[3] * u[3] + u[4] * u[4]) + u[5] * u[5];
    if (vv <= eps && ww <= eps) {
        st->converged = 1;
        st->done = 1;
    }
}
template <class M>
__global__ __launch_bounds__(64) void k_vmap_icp_solve(LoopState<M::kWords>* __restrict__ st, rgbd360_map_align_trace* __restrict__ trace,
                                                       const double* __restrict__ part, int n_rows, int final_pass, long long min_matches, float eps) {
    if (!final_pass && st->done) return;
    __shared__ double s_row[M::kWords];
    icp_solve_rows<M>(st, trace, part, n_rows, final_pass, min_matches, eps, s_row);
}

}  // namespace vmap

namespace {

// what one alignment call works on: the input in device memory, the launch grid, the checked parameters (min_support, max_flatness:
// point-to-plane and the normal layer of generalized ICP; the next three: generalized ICP, map_align_gicp.h; the last three: coloured ICP,
// map_align_colour.h)
struct IcpJob {
    MapSource src;
    dim3 grid;
    int n_rows;
    rgbd360_map_align_params p;
    int min_support;
    float max_flatness;
    float epsilon = 0.f;
    int use_target_normals = 0;
    const float* normal = nullptr;       // the source's normals in device memory, three floats per point of a cloud; null: none
    float lambda_geometric = 1.f;
    int min_gradient_support = 0;
    float min_spread = 0.f;
    int robust_kind = RGBD360_MAP_ROBUST_NONE;       // the robust form of a method alone (RobustIcp): the kind and delta of this call's level
    double robust_delta = 0.0;
};

int icp_check_params(rgbd360_map* m, const rgbd360_map_align_params* params, rgbd360_map_align_params& p) {
    if (params) p = *params;
    else rgbd360_map_default_align_params(m, &p);
    if (!(p.max_dist > 0.f && p.max_dist <= m->leaf)) return vmap_fail(m, -1, "max_dist must lie in (0, leaf]");
    if (p.max_iters < 0 || p.max_iters > vmap::kIcpMaxIters) return vmap_fail(m, -1, "max_iters must lie in 0 .. 1000");
    if (p.min_count < 1) return vmap_fail(m, -1, "min_count must be at least 1");
    if (!(p.eps >= 0.f)) return vmap_fail(m, -1, "eps must not be negative");
    return 0;
}
// the grid of a job's source and the buffers, wide enough for every method; icp_prepare: the checked, non-empty input of a call into
// device memory first (vmap_to_device)
int icp_buffers(rgbd360_map* m, IcpJob& job) {      // (job.src is set: also the source another map uploaded, map_pyramid.h)
    job.grid = vmap_grid(job.src);
    job.n_rows = (int)(job.grid.x * job.grid.y);
    const size_t state_bytes = sizeof(vmap::LoopState<vmap::kIcpMaxWords>) + (size_t)std::max(job.p.max_iters, 1) * sizeof(rgbd360_map_align_trace);
    HIPC(m, m->a_part.ensure((size_t)job.n_rows * vmap::kIcpMaxWords));
    HIPC(m, m->a_state.ensure(state_bytes));
    HIPC(m, m->a_host.ensure(state_bytes));
    return 0;
}
int icp_prepare(rgbd360_map* m, const MapInput& in, IcpJob& job) {
    if (const int rc = vmap_to_device(m, in, job.src)) return rc;
    job.normal = in.normal;
    if (in.normal && !in.on_device) {        // (a cloud's: behind its points on the stream)
        const size_t bytes = (size_t)in.n * 3 * sizeof(float);
        HIPC(m, m->up_normal.ensure(bytes));
        HIPC(m, hipMemcpyAsync(m->up_normal, in.normal, bytes, hipMemcpyHostToDevice, m->s->stream));
        job.normal = reinterpret_cast<const float*>(m->up_normal.get());
    }
    return icp_buffers(m, job);
}
// the input of an evaluation entry (rgbd360_hip_diag.h): the sphere frame where there is a depth image, otherwise the n points xyz
MapInput icp_eval_input(const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention, const float* xyz, long long n, int on_device) {
    return depth ? sphere_input(nullptr, 0, depth, depth_step, depth_type, rows, cols, convention, on_device) : cloud_input(xyz, nullptr, n, on_device);
}

// A method M (PointIcp here, PlaneIcp in map_align_plane.h) is its row (Row = vmap::PointMethod, also its base) and, for the host: Params and Result, the
// public structs; Out, the per-point output pointers of an evaluation; check(m, params, job), the checked parameters into the job;
// eval_args(m, job, out, args), what the evaluation kernel takes beyond EvalCommon; fill_extra(st, res), the result fields the method adds.
template <class M>
using IcpState = vmap::LoopState<M::kWords>;
template <class M>
IcpState<M>* icp_state(rgbd360_map* m) { return reinterpret_cast<IcpState<M>*>(m->a_state.get()); }
template <class M>
rgbd360_map_align_trace* icp_trace(rgbd360_map* m) { return reinterpret_cast<rgbd360_map_align_trace*>(m->a_state.get() + sizeof(IcpState<M>)); }

template <class M>
int icp_launch_init(rgbd360_map* m, const float pose[16]) {
    vmap::IcpPose g;
    memcpy(g.m, pose, sizeof(g.m));
    hipLaunchKernelGGL((vmap::k_vmap_icp_init<M::kWords>), dim3(1), dim3(64), 0, m->s->stream, icp_state<M>(m), g);
    HIPC(m, hipGetLastError());
    return 0;
}
// what every evaluation of a job takes; the per-point outputs of a final pass, or none
vmap::EvalCommon icp_common(rgbd360_map* m, const IcpJob& job, int32_t* key3, float* d2) {
    return {(const unsigned long long*)m->table.get(), m->n_slots - 1, (unsigned long long)job.p.min_count, job.p.max_dist * job.p.max_dist, key3, d2};
}
// the evaluation kernel of method M on a job: M::eval_args is the method's host-side preparation (its layers, its parameters, its outputs)
template <class M>
int icp_launch_eval(rgbd360_map* m, const IcpJob& job, const vmap::Params& P, int final_pass, const typename M::Out& o) {
    typename M::Args a{};
    if (const int rc = M::eval_args(m, job, o, a)) return rc;
    const vmap::EvalCommon c = icp_common(m, job, o.key3, o.d2);
    with_choice<0, 1>(job.src.cloud, [&](auto S) {
        hipLaunchKernelGGL((vmap::k_vmap_eval<typename M::Row, decltype(S)::value>), job.grid, dim3(vmap::kThreads), 0, m->s->stream, P, job.src, c, a,
                           (const IcpState<M>*)icp_state<M>(m), final_pass, m->a_part.get());
    });
    HIPC(m, hipGetLastError());
    return 0;
}
template <class M>
int icp_launch_solve(rgbd360_map* m, const IcpJob& job, int final_pass) {
    hipLaunchKernelGGL((vmap::k_vmap_icp_solve<typename M::Row>), dim3(1), dim3(64), 0, m->s->stream, icp_state<M>(m), icp_trace<M>(m), (const double*)m->a_part.get(),
                       job.n_rows, final_pass, job.p.min_matches, job.p.eps);
    HIPC(m, hipGetLastError());
    return 0;
}
// init, iters x (eval, solve), the final pass with the per-point outputs, the copy of the state and its trace: enqueued, not waited for
template <class M>
int icp_enqueue(rgbd360_map* m, const IcpJob& job, const float guess[16], int iters, const typename M::Out& out) {
    const vmap::Params P = vmap_params(m, guess);
    if (const int rc = icp_launch_init<M>(m, guess)) return rc;
    for (int it = 0; it < iters; ++it) {
        if (const int rc = icp_launch_eval<M>(m, job, P, 0, typename M::Out{})) return rc;
        if (const int rc = icp_launch_solve<M>(m, job, 0)) return rc;
    }
    if (const int rc = icp_launch_eval<M>(m, job, P, 1, out)) return rc;
    if (const int rc = icp_launch_solve<M>(m, job, 1)) return rc;
    const size_t bytes = sizeof(IcpState<M>) + (size_t)iters * sizeof(rgbd360_map_align_trace);
    HIPC(m, hipMemcpyAsync(m->a_host, m->a_state, bytes, hipMemcpyDeviceToHost, m->s->stream));
    return 0;
}
template <class M>
const IcpState<M>& icp_host_state(rgbd360_map* m) { return *reinterpret_cast<const IcpState<M>*>(m->a_host.get()); }

// the result struct of an alignment from the state it ended in (also of every job of a batch, map_align_batch.h)
template <class M>
void icp_fill_result(const IcpState<M>& st, typename M::Result* res) {
    const double nm = st.row[M::kN];
    res->status = st.status;
    res->iterations = st.iterations;
    res->converged = st.converged;
    res->n_valid = (long long)st.row[M::kCounters];
    res->n_box_rejected = (long long)st.row[M::kCounters + 1];
    res->n_out_of_range = (long long)st.row[M::kCounters + 2];
    res->n_matched = (long long)nm;
    res->fitness = nm > 0.0 ? st.row[M::kSumSq] / nm : 0.0;
    memcpy(res->hessian, st.H, sizeof(res->hessian));
    memcpy(res->gradient, st.g, sizeof(res->gradient));
    M::fill_extra(st.row, nm, res);
}

template <class M>
int icp_run(rgbd360_map* m, const IcpJob& job, const float guess[16], float pose_out[16], typename M::Result* res);
// what rgbd360_map_align_robust_info reports of an alignment of method M that ended with the row `row` (a quadratic one: every weight is 1)
template <class M>
rgbd360_map_robust_info icp_robust_info(const IcpJob& job, const double* row) {
    rgbd360_map_robust_info o = {};
    o.method = M::kMethod;
    o.kind = job.robust_kind;
    o.delta_eff = job.robust_delta;
    o.sum_w = row[0];
    o.n = (long long)row[M::kN];
    o.n_downweighted = job.robust_kind != RGBD360_MAP_ROBUST_NONE ? (long long)row[M::kWords - 1] : 0;      // (a robust row's last word)
    return o;
}
// an align call of method M: rgbd360_map_align_sphere / _cloud and their _plane forms
template <class M>
int icp_align(rgbd360_map* m, const MapInput& in, const float guess[16], const typename M::Params* params, float pose_out[16], typename M::Result* res) {
    if (!m) return -1;
    m->err.clear();
    IcpJob job;
    if (const int rc = M::check(m, params, job)) return rc;
    if (!guess || !pose_out) return vmap_fail(m, -1, "guess and pose_out must not be null");
    const int chk = vmap_check(m, in, true);
    if (chk < 0) return chk;
    if (chk == 0)
        if (const int rc = icp_prepare(m, in, job)) return rc;
    m->a_trace.clear();
    if (chk == 1) {              // nothing to align
        memcpy(pose_out, guess, 16 * sizeof(float));
        if (res) {
            memset(res, 0, sizeof(*res));
            res->status = RGBD360_NO_VALID_PIXELS;
        }
        return RGBD360_NO_VALID_PIXELS;
    }
    return icp_run<M>(m, job, guess, pose_out, res);
}
// the loop of a prepared job from `guess`: enqueue, the one synchronisation, the trace, the pose and the result
template <class M>
int icp_run(rgbd360_map* m, const IcpJob& job, const float guess[16], float pose_out[16], typename M::Result* res) {
    if (const int rc = icp_enqueue<M>(m, job, guess, job.p.max_iters, typename M::Out{})) return rc;
    HIPC(m, hipStreamSynchronize(m->s->stream));
    const IcpState<M>& st = icp_host_state<M>(m);
    const rgbd360_map_align_trace* tr = reinterpret_cast<const rgbd360_map_align_trace*>(m->a_host.get() + sizeof(IcpState<M>));
    m->a_trace.assign(tr, tr + st.iterations);
    memcpy(pose_out, st.pose, 16 * sizeof(float));
    if (res) icp_fill_result<M>(st, res);
    m->a_robust = icp_robust_info<M>(job, st.row);
    return st.status;
}
// one evaluation at `pose` (the diag entries): the sums in front of the counters, the method's counters, the per-point outputs
template <class M>
int icp_eval(rgbd360_map* m, const MapInput& in, const float pose[16], const typename M::Params* params, double* sums, long long* counters,
             const typename M::Out& out) {
    constexpr int n_counters = M::kProbes - M::kCounters;
    IcpJob job;
    if (const int rc = M::check(m, params, job)) return rc;
    const int chk = vmap_check(m, in, true);
    if (chk < 0 && !in.cloud) return chk;        // (a refused cloud has always left the outputs zeroed, a refused image untouched)
    for (int k = 0; k < M::kCounters && sums; ++k) sums[k] = 0.0;
    for (int k = 0; k < n_counters && counters; ++k) counters[k] = 0;
    if (chk != 0) return std::min(chk, 0);
    job.p.max_iters = 0;
    if (const int rc = icp_prepare(m, in, job)) return rc;
    if (const int rc = icp_enqueue<M>(m, job, pose, 0, out)) return rc;
    HIPC(m, hipStreamSynchronize(m->s->stream));
    const IcpState<M>& st = icp_host_state<M>(m);
    for (int k = 0; k < M::kCounters && sums; ++k) sums[k] = st.row[k];
    for (int k = 0; k < n_counters && counters; ++k) counters[k] = (long long)st.row[M::kCounters + k];
    return 0;
}
// measurement: probes per point searched of the evaluation summed last, and the wall time of a whole alignment
template <class M>
int icp_read_probes(rgbd360_map* m, double* probes) {
    IcpState<M> st;
    if (hipMemcpy(&st, m->a_state, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return vmap_fail(m, -100, "reading the state failed");
    *probes = st.row[M::kSearched] > 0.0 ? st.row[M::kProbes] / st.row[M::kSearched] : 0.0;
    return 0;
}
template <class M>
int icp_time_whole(rgbd360_map* m, const IcpJob& job, const float pose[16], int reps, float& avg_us) {
    double wall = 0.0;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        if (const int rc = icp_enqueue<M>(m, job, pose, job.p.max_iters, typename M::Out{})) return rc;
        HIPC(m, hipStreamSynchronize(m->s->stream));
        wall += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    avg_us = (float)(wall / reps);
    return 0;
}

// The robust form of the method B: B's host description on the row vmap::Robust<B::Row>.  The kind and delta are the
// map's setting for the method (rgbd360_map_set_align_robust) -- a level's is its root's, delta x 2^shift with scale_with_level -- read
// into the job by check(), so that one call uses one setting; Out has w per point behind B's outputs.
inline const rgbd360_map_robust& icp_robust_setting(const rgbd360_map* m, int method) { return (m->parent ? m->parent : m)->robust[method]; }
template <class B>
struct RobustIcp : vmap::Robust<typename B::Row> {
    using Row = vmap::Robust<typename B::Row>;
    using Params = typename B::Params;
    using Result = typename B::Result;
    using Args = typename Row::Args;
    static constexpr int kMethod = B::kMethod;
    struct Out : B::Out {
        double* w = nullptr;
    };
    static int check(rgbd360_map* m, const Params* params, IcpJob& job) {
        if (const int rc = B::check(m, params, job)) return rc;
        const rgbd360_map_robust& s = icp_robust_setting(m, kMethod);
        job.robust_kind = s.kind;
        job.robust_delta = s.scale_with_level ? ldexp(s.delta, m->shift) : s.delta;
        return 0;
    }
    static int eval_args(rgbd360_map* m, const IcpJob& job, const Out& o, Args& a) {
        if (const int rc = B::eval_args(m, job, o, a)) return rc;
        a.kind = job.robust_kind;
        a.delta = job.robust_delta;
        a.w_out = o.w;
        return 0;
    }
    static void fill_extra(const double* row, double n, Result* res) { B::fill_extra(row, n, res); }
};
// a call of method B in the form the map's setting for B asks for: f(IcpTag<M>), M = B with RGBD360_MAP_ROBUST_NONE (the quadratic call,
// as it was before there was a setting), else RobustIcp<B>
template <class M>
struct IcpTag {
    using type = M;
};
template <class B, class F>
int icp_by_setting(const rgbd360_map* m, F&& f) {
    return m && icp_robust_setting(m, B::kMethod).kind != RGBD360_MAP_ROBUST_NONE ? f(IcpTag<RobustIcp<B>>{}) : f(IcpTag<B>{});
}

struct PointIcp : vmap::PointMethod {
    using Row = vmap::PointMethod;
    static constexpr int kMethod = RGBD360_MAP_METHOD_POINT;
    using Params = rgbd360_map_align_params;
    using Result = rgbd360_map_align_result;
    struct Out {
        int32_t* key3 = nullptr;
        float* d2 = nullptr;
    };
    static int check(rgbd360_map* m, const Params* params, IcpJob& job) { return icp_check_params(m, params, job.p); }
    static int eval_args(rgbd360_map*, const IcpJob&, const Out&, Args&) { return 0; }
    static void fill_extra(const double*, double, Result*) {}
};
}  // namespace

extern "C" void rgbd360_map_default_align_params(const rgbd360_map* m, rgbd360_map_align_params* p) {
    if (!p) return;
    p->max_dist = m ? m->leaf : 0.05f;
    p->max_iters = 10;       // OdometryRGBD360.cpp:102
    p->eps = 1e-6f;
    p->min_count = 1;
    p->min_matches = 6;
}

extern "C" int rgbd360_map_align_sphere(rgbd360_map* m, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                        const float guess[16], int on_device, const rgbd360_map_align_params* params, float pose_out[16],
                                        rgbd360_map_align_result* result) {
    return icp_by_setting<PointIcp>(m, [&](auto M) {
        return icp_align<typename decltype(M)::type>(m, sphere_input(nullptr, 0, depth, depth_step, depth_type, rows, cols, convention, on_device), guess, params,
                                                     pose_out, result);
    });
}
extern "C" int rgbd360_map_align_cloud(rgbd360_map* m, const float* xyz, long long n, const float guess[16], int on_device,
                                       const rgbd360_map_align_params* params, float pose_out[16], rgbd360_map_align_result* result) {
    return icp_by_setting<PointIcp>(m, [&](auto M) {
        return icp_align<typename decltype(M)::type>(m, cloud_input(xyz, nullptr, n, on_device), guess, params, pose_out, result);
    });
}

// measurement and tests (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_align_eval(rgbd360_map* m, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                      const float* xyz, long long n, const float pose[16], int on_device, const rgbd360_map_align_params* params,
                                      double sums[17], long long counters[3], int32_t* key3_dev, float* d2_dev, int max_trace, int* n_trace,
                                      rgbd360_map_align_trace* trace) {
    if (!m) return -1;
    m->err.clear();
    if (n_trace) *n_trace = (int)m->a_trace.size();
    for (int k = 0; trace && k < max_trace && k < (int)m->a_trace.size(); ++k) trace[k] = m->a_trace[k];
    if (!pose) return 0;
    return icp_eval<PointIcp>(m, icp_eval_input(depth, depth_step, depth_type, rows, cols, convention, xyz, n, on_device), pose, params, sums, counters,
                              {key3_dev, d2_dev});
}

extern "C" int rgbd360_map_time_align(rgbd360_map* m, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                      const float pose[16], const rgbd360_map_align_params* params, int reps, float avg_us[5], double* probes) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;      // (avg_us[2] inserts the frame)
    const MapInput in = sphere_input(nullptr, 0, depth_dev, depth_step, depth_type, rows, cols, convention, 1);
    if (const int rc = vmap_check_timed(m, in, pose, reps, avg_us)) return rc;
    IcpJob job;
    if (const int rc = PointIcp::check(m, params, job)) return rc;
    if (const int rc = icp_prepare(m, in, job)) return rc;
    const size_t drow = (size_t)cols * (depth_type == 0 ? 2 : 4);
    HIPC(m, m->up_depth.ensure(drow * rows));
    hipStream_t stream = m->s->stream;
    const vmap::Params P = vmap_params(m, pose);
    VmapTimer timer(m, stream);      // made last
    if (timer.rc) return timer.rc;
    int& rc = timer.rc;
    rc = icp_launch_init<PointIcp>(m, pose);
    if (rc == 0) rc = icp_launch_eval<PointIcp>(m, job, P, 1, {});      // once untimed: code and tables loaded
    timer.timed(avg_us[0], reps, [&] { return icp_launch_eval<PointIcp>(m, job, P, 1, {}); });
    timer.timed(avg_us[1], reps, [&] { return icp_launch_solve<PointIcp>(m, job, 1); });
    if (rc == 0 && probes) rc = icp_read_probes<PointIcp>(m, probes);
    timer.timed(avg_us[2], 1, [&] { return vmap_launch_insert(m, P, job.src); });
    if (rc == 0) {
        rgbd360_map_stats stats;
        rc = std::min(vmap_finish_insert(m, &stats), 0);
    }
    timer.timed(avg_us[3], reps, [&] {
        return hipMemcpy2DAsync(m->up_depth, drow, depth_dev, depth_step, drow, rows, hipMemcpyDeviceToDevice, stream) == hipSuccess ? 0 : -100;
    });
    if (const int failed = timer.finish(avg_us, 0, reps)) return failed;
    return icp_time_whole<PointIcp>(m, job, pose, reps, avg_us[4]);
}
