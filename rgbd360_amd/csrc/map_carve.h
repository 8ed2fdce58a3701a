// map_carve.h -- free-space observation and carving of the resident voxel map (rgbd360_map_observe_* / _votes / _carve,
// include/rgbd360_hip.h; tests/map_carve_reference.py restates it).  Every measurement of a posed depth frame, or of a list
// of rays, is a line of sight: the map voxels it passes through well in front of the measured point are seen through.  They can be
// reported (the votes) and erased (the carve).  Part of the Frame360 translation unit, behind map_raycast.h, whose traversal it runs.
//
//   k_vmap_observe   one lane per measurement.  The segment o -> w is vmap::cast_ray with t_max = 1 under the policy ThroughVotes: the walk
//                    -- the same text as the ray cast's, brick jumps included -- does not end at a candidate; every candidate is handed to
//                    the policy, which applies the three rules of the through-vote and adds 1 to the slot's vote word.  Then the voxel the
//                    measurement would feed (vmap::point_key, insertion's step 5) gets its end-vote, 2^32 on the same word.  Every vote is
//                    one 64-bit atomicAdd; the add that returns 0 counts the voxel as newly voted, which does not depend on the order.
//                    The table is only read.  Counters: one add per wave and counter, as in k_vmap_raycast.
//   k_vmap_carve     one lane per slot: {key, count} as one 16-byte load and the vote word; a voxel that the thresholds condemn gets
//                    {key, 0} and 48 bytes of zeros as four 16-byte stores -- the tombstone a removal leaves.  One lane owns the slot: no
//                    atomics but the counters', one add per wave.
//   k_vmap_votes     one lane per slot, k_vmap_extract's shape: a wave reserves its output range with one add; six words per record.
//   host             the vote array (8 bytes per slot) is allocated on the first observation and belongs to the table's revision: an
//                    observation that accumulates, the read-out and the carve refuse votes taken on a table written since.  A carve moves
//                    the revision itself and takes the votes along, spent: readable, not to be carved or added to again.
#pragma once

namespace vmap {

enum { kObRays, kObValid, kObSkipped, kObMissBox, kObMaxSteps, kObSteps, kObLookups, kObThrough, kObEnd, kObVoted, kObWords };      // rgbd360_map_observe_stats
enum { kCvVoted, kCvVoxels, kCvPoints, kCvProtEnd, kCvProtCount, kCvWords };      // rgbd360_map_carve_stats but n_voxels, the host's

// The policy of a line of sight (cast_ray): a candidate seen through gets one vote and the walk goes on.
struct ThroughVotes {
    static constexpr bool kStops = false;
    const unsigned long long* table;
    unsigned long long* votes;
    double near2, margin_rel, margin2, off2_max;      // near^2, margin_rel, (margin_leaves leaf)^2, max_offset^2
    unsigned through, voted;
    __device__ __forceinline__ void cell(const unsigned long long* rec, double th, double dd, double off2) {
#pragma clang fp contract(off)
        if (!((th * th) * dd >= near2)) return;
        const double q = (1.0 - th) - margin_rel;
        if (!(q >= 0.0 && (q * q) * dd >= margin2 && off2 <= off2_max)) return;
        const unsigned long long old = atomicAdd(votes + (rec - table) / kFields, 1ull);
        ++through;
        voted += old == 0 ? 1u : 0u;
    }
};

struct ObserveJob {
    DevGrid G;
    RayParams P;                                     // t_max = 1; t_min unused
    unsigned long long* votes;
    double near2, margin_rel, margin2;
    Params pose;                                     // a sphere image: the pose; no box
    Source src;
    long long n;                                     // a list: its rays
    const float *origins, *endpoints;
    unsigned long long* stats;                       // kObWords counters
};

template <bool LAYER, bool SPHERE>
__global__ __launch_bounds__(kRayThreads) void k_vmap_observe(ObserveJob J) {
#pragma clang fp contract(off)
    static_assert(kRayThreads == kThreads, "load_points<0, 1>: a workgroup takes kThreads pixels of a row");
    float o[3], w[3];
    bool in, valid;
    unsigned long long key = 0;
    if (SPHERE) {
        float x[1], y[1], z[1];
        bool in1[1];
        long long index[1];
        load_points<0, 1>(J.src, x, y, z, in1, index);
        in = in1[0];
        long long f[3];
        valid = in && classify(J.pose, x[0], y[0], z[0], key, f, w) == 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = J.pose.pose[12 + k];
    } else {
        const long long idx = (long long)blockIdx.x * kRayThreads + threadIdx.x;
        in = idx < J.n;
        const size_t ii = in ? (size_t)idx : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = J.origins[3 * ii + k];
            w[k] = J.endpoints[3 * ii + k];
        }
        valid = in && fabsf(w[0]) < 4096.f && fabsf(w[1]) < 4096.f && fabsf(w[2]) < 4096.f;      // (a NaN fails)
        if (valid) key = point_key(w, J.P.inv_leaf);
    }
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = valid ? w[k] - o[k] : 0.f;
    RayResult H;
    H.status = kRayBad;
    H.steps = H.lookups = 0;
    ThroughVotes votes = {J.G.table, J.votes, J.near2, J.margin_rel, J.margin2, J.P.off2_max, 0u, 0u};
    if (valid) cast_ray<LAYER>(J.G, J.P, o, d, H, votes);      // (o or d not finite, d = 0: kRayBad)
    const bool ok = valid && H.status != kRayBad;
    unsigned end = 0;
    if (ok) {
        const unsigned long long* rec = J.G.voxel(key);
        if (rec && rec[1] != 0) {
            const unsigned long long old = atomicAdd(J.votes + (rec - J.G.table) / kFields, 1ull << 32);
            end = 1;
            votes.voted += old == 0 ? 1u : 0u;
        }
    }
    unsigned long long steps = (unsigned long long)H.steps, lookups = (unsigned long long)H.lookups;
    unsigned long long through = votes.through, voted = votes.voted;
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        steps += __shfl_xor(steps, off);
        lookups += __shfl_xor(lookups, off);
        through += __shfl_xor(through, off);
        voted += __shfl_xor(voted, off);
    }
    const unsigned long long b_in = __ballot(in), b_ok = __ballot(ok), b_miss = __ballot(ok && H.status == kRayMissBox),
                             b_max = __ballot(ok && H.status == kRayMaxSteps), b_end = __ballot(end != 0);
    if ((threadIdx.x & 63) == 0 && b_in) {      // one add per wave and counter
        atomicAdd(J.stats + kObRays, (unsigned long long)__popcll(b_in));
        if (b_ok) atomicAdd(J.stats + kObValid, (unsigned long long)__popcll(b_ok));
        if (b_in & ~b_ok) atomicAdd(J.stats + kObSkipped, (unsigned long long)__popcll(b_in & ~b_ok));
        if (b_miss) atomicAdd(J.stats + kObMissBox, (unsigned long long)__popcll(b_miss));
        if (b_max) atomicAdd(J.stats + kObMaxSteps, (unsigned long long)__popcll(b_max));
        if (steps) atomicAdd(J.stats + kObSteps, steps);
        if (lookups) atomicAdd(J.stats + kObLookups, lookups);
        if (through) atomicAdd(J.stats + kObThrough, through);
        if (b_end) atomicAdd(J.stats + kObEnd, (unsigned long long)__popcll(b_end));
        if (voted) atomicAdd(J.stats + kObVoted, voted);
    }
}

// min_through >= 1; max_count 0: no limit
__global__ __launch_bounds__(256) void k_vmap_carve(unsigned long long* __restrict__ table, unsigned long long n_slots, const unsigned long long* __restrict__ votes,
                                                    unsigned long long min_through, unsigned long long max_end, unsigned long long max_count,
                                                    unsigned long long* __restrict__ stats) {
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long sc = s < n_slots ? s : 0;
    ulonglong2* rec = reinterpret_cast<ulonglong2*>(table + sc * kFields);
    const ulonglong2 kc = rec[0];      // key, count
    const unsigned long long v = votes[sc];
    const bool voted = s < n_slots && kc.x != kEmpty && kc.y != 0 && v != 0;
    const unsigned long long b_voted = __ballot(voted);
    if (!b_voted) return;
    const unsigned long long through = v & 0xffffffffull, end = v >> 32;
    const bool seen = voted && through >= min_through, end_ok = end <= max_end, count_ok = max_count == 0 || kc.y <= max_count;
    const bool carve = seen && end_ok && count_ok;
    if (carve) {
        const ulonglong2 zero = {0ull, 0ull}, tomb = {kc.x, 0ull};
        rec[0] = tomb;
        rec[1] = zero;
        rec[2] = zero;
        rec[3] = zero;
    }
    unsigned long long points = carve ? kc.y : 0ull;
#pragma unroll
    for (int off = 32; off; off >>= 1) points += __shfl_xor(points, off);
    const unsigned long long b_carve = __ballot(carve), b_end = __ballot(seen && !end_ok), b_count = __ballot(seen && end_ok && !count_ok);
    if ((threadIdx.x & 63) == 0) {      // one add per wave and counter
        atomicAdd(stats + kCvVoted, (unsigned long long)__popcll(b_voted));
        if (b_carve) atomicAdd(stats + kCvVoxels, (unsigned long long)__popcll(b_carve));
        if (points) atomicAdd(stats + kCvPoints, points);
        if (b_end) atomicAdd(stats + kCvProtEnd, (unsigned long long)__popcll(b_end));
        if (b_count) atomicAdd(stats + kCvProtCount, (unsigned long long)__popcll(b_count));
    }
}

// one record per slot with a non-zero vote word: key3, through, end, count; records beyond max_out are counted, not written
__global__ __launch_bounds__(256) void k_vmap_votes(const unsigned long long* __restrict__ table, unsigned long long n_slots, const unsigned long long* __restrict__ votes,
                                                    long long max_out, unsigned long long* __restrict__ counter, int32_t* __restrict__ out) {
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long sc = s < n_slots ? s : 0;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(table + sc * kFields);
    const unsigned long long v = votes[sc];
    const bool has = s < n_slots && v != 0;
    const unsigned long long wave = __ballot(has);
    unsigned long long base = 0;
    if (lane == 0 && wave) base = atomicAdd(counter, (unsigned long long)__popcll(wave));      // one add per wave
    base = __shfl(base, 0);
    const unsigned long long o = base + (unsigned long long)__popcll(wave & ((1ull << lane) - 1ull));
    if (!has || (long long)o >= max_out) return;
    unpack_key3(kc.x, out + 6 * o);
    out[6 * o + 3] = (int32_t)(v & 0xffffffffull);
    out[6 * o + 4] = (int32_t)(v >> 32);
    out[6 * o + 5] = (int32_t)kc.y;
}

}  // namespace vmap

namespace {

static_assert(sizeof(rgbd360_map_observe_params) == 28, "seven 4-byte fields");
static_assert(sizeof(rgbd360_map_observe_stats) == vmap::kObWords * sizeof(unsigned long long), "the statistics are the counters in their order");
static_assert(sizeof(rgbd360_map_carve_stats) == (vmap::kCvWords + 1) * sizeof(unsigned long long), "the counters in their order, then n_voxels");

int observe_check_params(rgbd360_map* m, const rgbd360_map_observe_params* params, rgbd360_map_observe_params& p) {
    if (params) p = *params;
    else rgbd360_map_default_observe_params(m, &p);
    if (p.min_count < 1) return vmap_fail(m, -1, "min_count must be at least 1");
    if (!(p.near >= 0.f) || !std::isfinite(p.near)) return vmap_fail(m, -1, "near must be finite and not negative");
    if (!(p.margin_leaves >= 0.f) || !std::isfinite(p.margin_leaves)) return vmap_fail(m, -1, "margin_leaves must be finite and not negative");
    if (!(p.margin_rel >= 0.f) || !std::isfinite(p.margin_rel)) return vmap_fail(m, -1, "margin_rel must be finite and not negative");
    if (!(p.max_offset >= 0.f)) return vmap_fail(m, -1, "max_offset must not be negative");
    if (p.max_steps < 1 || p.max_steps > (1 << 23)) return vmap_fail(m, -1, "max_steps must lie in 1 .. 2^23");
    if (p.accumulate != 0 && p.accumulate != 1) return vmap_fail(m, -1, "accumulate must be 0 or 1");
    return 0;
}
void observe_fill_stats(const unsigned long long* w, rgbd360_map_observe_stats* st) {
    if (!st) return;
    long long* out = &st->n_rays;
    for (int k = 0; k < vmap::kObWords; ++k) out[k] = w ? (long long)w[k] : 0;
}
// whether the votes the map holds are those of the table as it stands
bool votes_current(const rgbd360_map* m) { return m->vt_have && m->vt_rev == m->revision; }
// what an accumulating observation of n measurements refuses before anything is touched
int observe_check_accumulate(rgbd360_map* m, const rgbd360_map_observe_params& p, long long n) {
    if (!p.accumulate || !m->vt_have) return 0;      // (no votes: the observation starts them)
    if (m->vt_spent) return vmap_fail(m, -1, "the votes are spent: a carve has used them");
    if (m->vt_rev != m->revision) return vmap_fail(m, -1, "the map was written since the votes were taken");
    if (m->vt_rays_n + n >= (1ll << 31)) return vmap_fail(m, -1, "the accumulated measurements would reach 2^31");
    return 0;
}
// The vote array of the table as it stands, zeroed unless the observation accumulates; the counters; the coarse layer.  n_voxels > 0.
int observe_prepare(rgbd360_map* m, const rgbd360_map_observe_params& p) {
    hipSetDevice(m->s->p.device);
    HIPC(m, m->vt_stats.ensure(vmap::kObWords));
    HIPC(m, m->vt_hstats.ensure(vmap::kObWords));
    if (!p.accumulate || !m->vt_have) {
        m->vt_have = false;
        HIPC(m, m->vt_votes.ensure(m->n_slots));
        HIPC(m, hipMemsetAsync(m->vt_votes, 0, m->n_slots * sizeof(unsigned long long), m->s->stream));
        m->vt_rays_n = m->vt_voted = 0;
        m->vt_spent = false;
        m->vt_rev = m->revision;
        m->vt_have = true;
    }
    return ray_prepare(m);
}
vmap::ObserveJob observe_job(const rgbd360_map* m, const rgbd360_map_observe_params& p) {
    vmap::ObserveJob J = {};
    J.G = {m->table, m->n_slots - 1, m->rc_bkeys, m->rc_bslots - 1, m->rc_bidx, m->rc_masks};
    J.P.min_count = (unsigned long long)p.min_count;
    J.P.t_min = 0.0;
    J.P.t_max = 1.0;
    J.P.off2_max = (double)p.max_offset * (double)p.max_offset;
    J.P.max_steps = p.max_steps;
    J.P.inv_leaf = m->inv_leaf;
    for (int k = 0; k < 3; ++k) J.P.lo[k] = m->rc_lo[k], J.P.hi[k] = m->rc_hi[k];
    J.votes = m->vt_votes;
    J.near2 = (double)p.near * (double)p.near;
    J.margin_rel = (double)p.margin_rel;
    const double margin = (double)p.margin_leaves * (double)m->leaf;
    J.margin2 = margin * margin;
    J.stats = m->vt_stats;
    return J;
}
// the kernel over the job, enqueued behind the clear of its counters
int observe_launch(rgbd360_map* m, const vmap::ObserveJob& J, const dim3& grid, bool sphere, bool plain) {
    HIPC(m, hipMemsetAsync(m->vt_stats, 0, vmap::kObWords * sizeof(unsigned long long), m->s->stream));
    with_choice<1, 0>(plain, [&](auto L) {
        with_choice<0, 1>(sphere, [&](auto S) {
            hipLaunchKernelGGL((vmap::k_vmap_observe<decltype(L)::value != 0, decltype(S)::value != 0>), grid, dim3(vmap::kRayThreads), 0, m->s->stream, J);
        });
    });
    HIPC(m, hipGetLastError());
    return 0;
}
// how an observation of n measurements ends: the counters on the host, the votes' books brought up to date
int observe_finish(rgbd360_map* m, long long n, rgbd360_map_observe_stats* stats) {
    HIPC(m, hipMemcpyAsync(m->vt_hstats, m->vt_stats, vmap::kObWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->s->stream));
    HIPC(m, hipStreamSynchronize(m->s->stream));
    m->vt_rays_n += n;
    m->vt_voted += (long long)m->vt_hstats[vmap::kObVoted];
    observe_fill_stats(m->vt_hstats, stats);
    return 0;
}
dim3 observe_sphere_grid(int rows, int cols) { return dim3((cols + vmap::kRayThreads - 1) / vmap::kRayThreads, rows); }
void observe_sphere_job(const rgbd360_map* m, vmap::ObserveJob& J, const MapSource& src, const float* pose) {
    J.pose = vmap_params(m, pose);
    J.pose.has_box = 0;      // a point outside the box is not stored, but it still proves free space
    J.src = src;
}
// the carve kernel over the table, enqueued behind the clear of its counters (vt_stats)
int carve_launch(rgbd360_map* m, unsigned long long min_through, unsigned long long max_end, unsigned long long max_count) {
    HIPC(m, hipMemsetAsync(m->vt_stats, 0, vmap::kCvWords * sizeof(unsigned long long), m->s->stream));
    hipLaunchKernelGGL(vmap::k_vmap_carve, dim3((unsigned)((m->n_slots + 255) / 256)), dim3(256), 0, m->s->stream, m->table, m->n_slots, m->vt_votes, min_through,
                       max_end, max_count, m->vt_stats);
    HIPC(m, hipGetLastError());
    return 0;
}
static_assert(vmap::kCvWords <= vmap::kObWords, "the carve's counters live in the observation's words");

}  // namespace

extern "C" void rgbd360_map_default_observe_params(const rgbd360_map* m, rgbd360_map_observe_params* p) {
    if (!p) return;
    p->min_count = 1;
    p->near = m ? m->leaf : 0.05f;
    p->margin_leaves = 2.0f;
    p->margin_rel = 0.f;
    p->max_offset = 0.5f;
    p->max_steps = 8192;
    p->accumulate = 0;
}

extern "C" int rgbd360_map_observe_sphere(rgbd360_map* m, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                          const float pose[16], int on_device, const rgbd360_map_observe_params* params, rgbd360_map_observe_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;
    rgbd360_map_observe_params p;
    if (const int rc = observe_check_params(m, params, p)) return rc;
    const MapInput in = sphere_input(nullptr, 0, depth, depth_step, depth_type, rows, cols, convention, on_device);
    const int chk = vmap_check(m, in, pose != nullptr);
    if (chk < 0) return chk;
    const long long n = (long long)rows * cols;
    if (const int rc = observe_check_accumulate(m, p, n)) return rc;
    observe_fill_stats(nullptr, stats);
    if (chk == 1 || m->n_voxels == 0) return 0;
    if (const int rc = observe_prepare(m, p)) return rc;
    MapSource src;
    if (const int rc = vmap_to_device(m, in, src)) return rc;
    vmap::ObserveJob J = observe_job(m, p);
    observe_sphere_job(m, J, src, pose);
    if (const int rc = observe_launch(m, J, observe_sphere_grid(rows, cols), true, m->rc_plain)) return rc;
    return observe_finish(m, n, stats);
}

extern "C" int rgbd360_map_observe_rays(rgbd360_map* m, long long n, const float* origins, const float* endpoints, int on_device,
                                        const rgbd360_map_observe_params* params, rgbd360_map_observe_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;
    rgbd360_map_observe_params p;
    if (const int rc = observe_check_params(m, params, p)) return rc;
    if (n < 0 || n >= (1ll << 31)) return vmap_fail(m, -1, "bad ray count");
    if (n > 0 && (!origins || !endpoints)) return vmap_fail(m, -1, "origins and endpoints must not be null");
    if (const int rc = observe_check_accumulate(m, p, n)) return rc;
    observe_fill_stats(nullptr, stats);
    if (n == 0 || m->n_voxels == 0) return 0;
    if (const int rc = observe_prepare(m, p)) return rc;
    vmap::ObserveJob J = observe_job(m, p);
    const size_t N = (size_t)n;
    J.n = n;
    if (on_device) {
        J.origins = origins, J.endpoints = endpoints;
    } else {
        HIPC(m, m->vt_rays.ensure(6 * N));
        HIPC(m, hipMemcpyAsync(m->vt_rays, origins, 3 * N * sizeof(float), hipMemcpyHostToDevice, m->s->stream));
        HIPC(m, hipMemcpyAsync(m->vt_rays + 3 * N, endpoints, 3 * N * sizeof(float), hipMemcpyHostToDevice, m->s->stream));
        J.origins = m->vt_rays, J.endpoints = m->vt_rays + 3 * N;
    }
    const dim3 grid((unsigned)((n + vmap::kRayThreads - 1) / vmap::kRayThreads));
    if (const int rc = observe_launch(m, J, grid, false, m->rc_plain)) return rc;
    return observe_finish(m, n, stats);
}

extern "C" long long rgbd360_map_votes(rgbd360_map* m, long long max_out, int32_t* key3, int32_t* through, int32_t* end, int32_t* count) {
    if (!m) return -1;
    m->err.clear();
    if (max_out < 0) return vmap_fail(m, -1, "max_out must not be negative");
    if (!m->vt_have) return vmap_fail(m, -1, "the map holds no votes");
    if (!votes_current(m)) return vmap_fail(m, -1, "the map was written since the votes were taken");
    const size_t n = (size_t)m->vt_voted, n_out = std::min(n, (size_t)max_out);
    if (n_out == 0) return m->vt_voted;
    hipSetDevice(m->s->p.device);
    // every record unsorted (the first max_out of the SORTED records are wanted), then the order of the keys on the host
    HIPC(m, m->vt_out.ensure(6 * n));
    HIPC(m, hipMemsetAsync(m->vt_stats, 0, sizeof(unsigned long long), m->s->stream));
    hipLaunchKernelGGL(vmap::k_vmap_votes, dim3((unsigned)((m->n_slots + 255) / 256)), dim3(256), 0, m->s->stream, m->table, m->n_slots, m->vt_votes, (long long)n,
                       m->vt_stats, m->vt_out);
    HIPC(m, hipGetLastError());
    std::vector<int32_t> rec(6 * n);
    HIPC(m, hipMemcpyAsync(rec.data(), m->vt_out, 6 * n * sizeof(int32_t), hipMemcpyDeviceToHost, m->s->stream));
    HIPC(m, hipStreamSynchronize(m->s->stream));
    std::vector<size_t> order(n);
    for (size_t k = 0; k < n; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {      // (i_z, i_y, i_x) ascending, as rgbd360_map_extract
        for (int q = 2; q >= 0; --q)
            if (rec[6 * a + q] != rec[6 * b + q]) return rec[6 * a + q] < rec[6 * b + q];
        return false;
    });
    for (size_t o = 0; o < n_out; ++o) {
        const int32_t* r = rec.data() + 6 * order[o];
        for (int q = 0; q < 3 && key3; ++q) key3[3 * o + q] = r[q];
        if (through) through[o] = r[3];
        if (end) end[o] = r[4];
        if (count) count[o] = r[5];
    }
    return m->vt_voted;
}

extern "C" int rgbd360_map_carve(rgbd360_map* m, int min_through, int max_end, int max_count, rgbd360_map_carve_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    if (stats) *stats = {0, 0, 0, 0, 0, m->n_voxels};
    if (const int rc = vmap_refuse_level(m)) return rc;
    if (min_through < 1 || max_end < 0 || max_count < 0) return vmap_fail(m, -1, "min_through must be at least 1, max_end and max_count not negative");
    if (!m->vt_have) return vmap_fail(m, -1, "the map holds no votes");
    if (m->vt_spent) return vmap_fail(m, -1, "the votes are spent: a carve has used them");
    if (!votes_current(m)) return vmap_fail(m, -1, "the map was written since the votes were taken");
    hipSetDevice(m->s->p.device);
    if (const int rc = carve_launch(m, (unsigned long long)min_through, (unsigned long long)max_end, (unsigned long long)max_count)) return rc;
    HIPC(m, hipMemcpyAsync(m->vt_hstats, m->vt_stats, vmap::kCvWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->s->stream));
    HIPC(m, hipStreamSynchronize(m->s->stream));
    const unsigned long long* w = m->vt_hstats;
    m->n_voxels -= (long long)w[vmap::kCvVoxels];
    if (w[vmap::kCvVoxels]) {      // the table was written: the derived layers rebuild on their next use
        m->may_hold_tombstones = true;
        ++m->revision;
    }
    m->vt_rev = m->revision;      // the votes go along, spent
    m->vt_spent = true;
    if (stats)
        *stats = {(long long)w[vmap::kCvVoted],   (long long)w[vmap::kCvVoxels],    (long long)w[vmap::kCvPoints],
                  (long long)w[vmap::kCvProtEnd], (long long)w[vmap::kCvProtCount], m->n_voxels};
    return 0;
}

extern "C" size_t rgbd360_map_vote_bytes(const rgbd360_map* m) { return m ? m->vt_votes.capacity() * sizeof(unsigned long long) : 0; }
extern "C" int rgbd360_map_release_votes(rgbd360_map* m) {
    if (!m) return -1;
    m->err.clear();
    vmap_drop_votes(m);
    return 0;
}

// measurement (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_time_observe(rgbd360_map* m, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                        const float pose[16], const rgbd360_map_observe_params* params, int plain, int reps, float* observe_us, float* carve_us,
                                        rgbd360_map_observe_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;
    rgbd360_map_observe_params p;
    if (const int rc = observe_check_params(m, params, p)) return rc;
    const MapInput in = sphere_input(nullptr, 0, depth_dev, depth_step, depth_type, rows, cols, convention, 1);
    if (const int rc = vmap_check_timed(m, in, pose, reps, observe_us)) return rc;
    if (m->n_voxels == 0) return vmap_fail(m, -1, "bad arguments");
    p.accumulate = 0;
    if (const int rc = observe_prepare(m, p)) return rc;
    MapSource src;
    if (const int rc = vmap_to_device(m, in, src)) return rc;
    vmap::ObserveJob J = observe_job(m, p);
    observe_sphere_job(m, J, src, pose);
    VmapTimer timer(m, m->s->stream);
    for (int r = 0; r < reps && timer.rc == 0; ++r) {
        timer.rc = hipMemsetAsync(m->vt_votes, 0, m->n_slots * sizeof(unsigned long long), m->s->stream) == hipSuccess ? 0 : vmap_fail(m, -100, "hipMemsetAsync failed");
        timer.timed(observe_us[r], 1, [&] { return observe_launch(m, J, observe_sphere_grid(rows, cols), true, plain != 0); });
        if (r == reps - 1 && timer.rc == 0) timer.rc = observe_finish(m, (long long)rows * cols, stats);
        // the scan alone: thresholds nothing meets, so that the table stays as it is
        if (carve_us) timer.timed(carve_us[r], 1, [&] { return carve_launch(m, ~0ull, 0ull, 0ull); });
    }
    if (timer.rc) {
        (void)hipGetLastError();
        return timer.rc;
    }
    HIPC(m, hipStreamSynchronize(m->s->stream));
    m->vt_rays_n = (long long)rows * cols;      // the votes of the last repetition stay, current
    m->vt_voted = (long long)m->vt_hstats[vmap::kObVoted];
    return 0;
}
