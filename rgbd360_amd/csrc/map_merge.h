// map_merge.h -- composing voxel maps: merge at a pose, exact un-merge, table records (rgbd360_map_merge / _unmerge / _records /
// _add_records, include/rgbd360_hip.h; tests/map_merge_reference.py restates it in numpy).  Part of the Frame360
// translation unit, behind map_pyramid.h, whose kernel shape it starts from; the table, find_or_claim, find, centroid and point_key are
// those of voxel_map.h / map_table.h: one layout, one hash, one probe bound, one read-out.
//
// Submaps are what a pose graph can move: a small map per keyframe window, the global map composed from them.  The sums are integers, so
// a voxel record is a term that can be added to another table and taken off again, exactly.  The source is the set of live voxels of a
// table (count >= min_count), or a dense list of records.  Per source voxel {key, n, S, C}:
//   sum mode     the key is kept and the seven words are added (equal leaves): the map that received both maps' insertions.
//   pose mode    c = vmap::centroid (the read-out's bits); w = pose c in float32 without contraction (step 3 of an insert); dropped
//                unless |w_k| < 4096 and n < 2^31; the destination key from w and the DESTINATION's inv_leaf; count += n,
//                S_k += n llrint((double)w_k 2^20), the colour sums as they are: n coincident points at the posed centroid.
//   un-merge     the same terms taken off in removal's manner (map_edit.h): a read-only find, the count lowered in a compare-and-swap loop
//                clamped at zero, the negatives of the six sums; a voxel that is missing or short keeps its sums (counted).
//
//   k_vmap_merge    one template over {table slots | record list} x {add | subtract} x {pose | sums}.  k_vmap_coarsen's shape: eight
//                   lanes per 64-byte source slot, lane q holds word q, key and count (and in pose mode the three coordinate sums) reach
//                   the others by lane exchange.  Every lane of a slot forms the centroid, the posed point and the range verdict (the same
//                   bits in all eight: no divergence, no second exchange); the lead lane finds or claims (add) or finds and takes
//                   (subtract) the destination slot and hands it on; lane q then adds ITS term to word q: n, n fix(w_q), or the colour
//                   word as it is -- one atomic wave-instruction carries eight slots of 56 contiguous bytes.  64-bit integer atomics only;
//                   no floating-point atomics, no fences, no ticket: the kernel boundary is the synchronisation.  A destination that may
//                   hold tombstones counts a new voxel as the count add that returned 0 (claim or revival; voxel_map.h, kInsertRevive);
//                   otherwise as the claim.  Counters: a wave's counts by ballot / butterfly, the block's through LDS, one global add per
//                   block and counter.
//   no LDS pre-merge   under a rigid pose between equal leaves a workgroup's 32 source slots arrive in hash order and share next to no
//                   destination voxel.  Measured (profiles/map_merge_perf.txt; a submap of eight 2048 x 1024 frames,
//                   46 322 voxels): 0.973 destination voxels per source voxel at equal leaves -- a block-level merge could save at most
//                   one update in 37 -- and the launch costs 1.8 - 2.0 scans of the source table (k_vmap_extract over it), as
//                   k_vmap_coarsen does.  Into a destination leaf 8 x the source's, 52 source voxels share a destination voxel and the
//                   add launch takes the same time (65.9 us against 66.4 us): it is not bound by its same-address atomics.  The
//                   subtract launch is 1.25 x slower there (81.0 us against 64.9 us): its count step is a compare-and-swap loop that
//                   retries under contention.  A pre-merge keyed by destination for un-merging into coarse destinations is the named
//                   open item; nothing was built for it.
//   k_vmap_check_records   one lane per record of a list against the census rules, before anything is written: the bad ones counted.
//   k_vmap_records  one lane per slot, a wave reserves its output range with one counter add (k_vmap_extract's shape) and every live lane
//                   stores its 64 bytes; the host sorts by key.
//   host            one launch and one synchronisation per merge / un-merge; both maps live on one context, whose stream every entry
//                   leaves drained, so the source's table is at rest.  The counters use the map's d_stats / h_stats (grown to kMgWords).
#pragma once

namespace vmap {

enum {
    kMgVoxRead, kMgPtsRead, kMgVoxBelow, kMgPtsBelow, kMgVoxRange, kMgPtsRange, kMgVoxAdded, kMgPtsAdded, kMgVoxNew, kMgVoxDropped, kMgPtsDropped,
    kMgMissing, kMgUnderflow, kMgWords
};
constexpr unsigned long long kMaxMergeCount = 1ull << 31;      // a posed voxel's n fix(w) stays in int64 below it; a record's count too

struct MergeParams {
    float pose[16];
    float inv_leaf;                  // the destination's
    unsigned long long min_count;
    int revive;                      // the destination may hold tombstones: a new voxel is the count add that returned 0
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// SRC 0: the n_src slots of a table; 1: a dense list of n_src checked records.  SUB: the terms are taken off.  POSE: pose mode.
template <int SRC, int SUB, int POSE>
__global__ __launch_bounds__(256) void k_vmap_merge(MergeParams P, const unsigned long long* __restrict__ src, unsigned long long n_src,
                                                    unsigned long long* __restrict__ dst, unsigned long long mask, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_stat[kMgWords];
    const int t = threadIdx.x, q = t & 7, lane = t & 63, lead = lane & ~7;
    if (t < kMgWords) s_stat[t] = 0;
    __syncthreads();
    // eight lanes per slot: lane q holds word q (a slot past the source reads slot 0 and counts as empty)
    const unsigned long long slot = ((unsigned long long)blockIdx.x * 256 + t) >> 3;
    const bool in = slot < n_src;
    const unsigned long long v = src[(in ? slot : 0) * kFields + q];
    const unsigned long long key = __shfl(v, lead), n = __shfl(v, lead + 1);
    const bool live = in && (SRC == 1 || (key != kEmpty && n != 0));      // (count 0: a tombstone)
    int cls = !live ? 0 : n < P.min_count ? 1 : 3;                         // 1 below min_count, 2 out of range, 3 goes on
    unsigned long long to_key = key, term = v;
    if (POSE) {
        unsigned long long rec[5];
        rec[2] = __shfl(v, lead + 2), rec[3] = __shfl(v, lead + 3), rec[4] = __shfl(v, lead + 4);
        float c[3], w[3];
        centroid(rec, n ? n : 1ull, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = ((P.pose[k] * c[0] + P.pose[k + 4] * c[1]) + P.pose[k + 8] * c[2]) + P.pose[k + 12];
        if (cls == 3 && !(fabsf(w[0]) < 4096.f && fabsf(w[1]) < 4096.f && fabsf(w[2]) < 4096.f && n < kMaxMergeCount)) cls = 2;
        if (cls == 3) {
            to_key = point_key(w, P.inv_leaf);
            const float wq = q == 2 ? w[0] : q == 3 ? w[1] : w[2];
            if (q >= 2 && q <= 4) term = (unsigned long long)((long long)n * llrint((double)wq * kFix));
        }
    }
    // the lead lane: the destination slot, claimed (add) or its count lowered (subtract)
    long long to = -1;
    bool fresh = false;                                    // add: claimed; subtract: emptied
    unsigned long long took = 0, missing = 0, underflow = 0;
    if (cls == 3 && q == 0) {
        if (!SUB) {
            to = find_or_claim(dst, mask, to_key, fresh);
        } else {
            const unsigned long long first = mix64(to_key) & mask;
            unsigned probes = 0;
            const long long at = find(dst, mask, to_key, first, dst[first * kFields], probes);
            if (at < 0) {
                missing = n;
            } else {      // (find_and_take's step with a 64-bit count: clamped to what is there, the sums of a short voxel are left alone)
                unsigned long long* cp = dst + (unsigned long long)at * kFields + 1;
                unsigned long long cur = __hip_atomic_load(cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                for (;;) {
                    took = cur < n ? cur : n;
                    if (took == 0) break;
                    const unsigned long long seen = atomicCAS(cp, cur, cur - took);
                    if (seen == cur) break;
                    cur = seen;
                }
                fresh = took && cur == took;
                if (took < n) underflow = n - took;
                else to = at;
            }
        }
    }
    to = __shfl(to, lead);
    bool revived = false;
    if (cls == 3 && to >= 0 && term) {
        unsigned long long* word = dst + (unsigned long long)to * kFields + q;
        if (!SUB && q == 1 && P.revive) revived = atomicAdd(word, term) == 0;
        else if (!SUB && q >= 1) atomicAdd(word, term);
        else if (SUB && q >= 2) atomicAdd(word, 0ull - term);
    }
    // the counters, by the slot's first lane (a revival: by its count lane)
    const bool first = q == 0;
    const bool is_new = SUB ? first && fresh : P.revive ? revived : first && fresh;
    const unsigned long long c_read = __popcll(__ballot(first && live)), c_below = __popcll(__ballot(first && cls == 1)),
                             c_range = __popcll(__ballot(first && cls == 2)), c_added = __popcll(__ballot(first && cls == 3 && to >= 0)),
                             c_dropped = __popcll(__ballot(first && cls == 3 && to < 0)), c_new = __popcll(__ballot(is_new));
    const unsigned long long mine = first && live ? n : 0ull;
    const unsigned long long p_read = wave_sum(mine), p_below = wave_sum(cls == 1 ? mine : 0ull), p_range = wave_sum(cls == 2 ? mine : 0ull);
    const unsigned long long p_added = wave_sum(SUB ? took : cls == 3 && to >= 0 ? mine : 0ull);
    const unsigned long long p_missing = SUB ? wave_sum(missing) : 0ull, p_underflow = SUB ? wave_sum(underflow) : 0ull;
    const unsigned long long p_dropped = SUB ? p_missing + p_underflow : wave_sum(cls == 3 && to < 0 ? mine : 0ull);
    if (lane == 0 && c_read) {
        atomicAdd(&s_stat[kMgVoxRead], c_read);
        atomicAdd(&s_stat[kMgPtsRead], p_read);
        if (c_below) atomicAdd(&s_stat[kMgVoxBelow], c_below), atomicAdd(&s_stat[kMgPtsBelow], p_below);
        if (c_range) atomicAdd(&s_stat[kMgVoxRange], c_range), atomicAdd(&s_stat[kMgPtsRange], p_range);
        if (c_added) atomicAdd(&s_stat[kMgVoxAdded], c_added);
        if (p_added) atomicAdd(&s_stat[kMgPtsAdded], p_added);
        if (c_new) atomicAdd(&s_stat[kMgVoxNew], c_new);
        if (c_dropped) atomicAdd(&s_stat[kMgVoxDropped], c_dropped), atomicAdd(&s_stat[kMgPtsDropped], p_dropped);
        if (p_missing) atomicAdd(&s_stat[kMgMissing], p_missing);
        if (p_underflow) atomicAdd(&s_stat[kMgUnderflow], p_underflow);
    }
    __syncthreads();
    if (t < kMgWords && s_stat[t]) atomicAdd(stats + t, s_stat[t]);
}

// the census rules (map_edit.h) and the key's range, per record of a list; bad[0]: the records that break one
__global__ __launch_bounds__(256) void k_vmap_check_records(const unsigned long long* __restrict__ records, unsigned long long n, unsigned long long* __restrict__ bad) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long* rec = records + (i < n ? i : 0) * kFields;
    const unsigned long long key = rec[0], count = rec[1];
    bool wrong = key == kEmpty || (key >> 63) != 0 || count == 0 || count >= kMaxMergeCount;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned long long S = rec[2 + k], col = rec[5 + k], mag = (long long)S < 0 ? 0ull - S : S;
        wrong = wrong || (mag >> 32) >= count || col > 255ull * count;      // (count < 2^31: the product does not wrap)
    }
    const unsigned long long wave = __ballot(i < n && wrong);
    if ((threadIdx.x & 63) == 0 && wave) atomicAdd(bad, (unsigned long long)__popcll(wave));
}

// the live slots as they are, unsorted, into out[8 * max_out]; records beyond max_out are counted, not written
__global__ __launch_bounds__(256) void k_vmap_records(const unsigned long long* __restrict__ table, unsigned long long n_slots, long long max_out,
                                                      unsigned long long* __restrict__ counter, unsigned long long* __restrict__ out) {
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const ulonglong2* rec = reinterpret_cast<const ulonglong2*>(table + (s < n_slots ? s : 0) * kFields);
    const ulonglong2 kc = rec[0];      // key, count
    const bool occupied = s < n_slots && kc.x != kEmpty && kc.y != 0;
    const unsigned long long wave = __ballot(occupied);
    unsigned long long base = 0;
    if (lane == 0 && wave) base = atomicAdd(counter, (unsigned long long)__popcll(wave));      // one add per wave
    base = __shfl(base, 0);
    const unsigned long long o = base + (unsigned long long)__popcll(wave & ((1ull << lane) - 1ull));
    if (!occupied || (long long)o >= max_out) return;
    ulonglong2* to = reinterpret_cast<ulonglong2*>(out + o * kFields);
    to[0] = kc;
    to[1] = rec[1];
    to[2] = rec[2];
    to[3] = rec[3];
}

}  // namespace vmap

namespace {

static_assert(vmap::kMgWords <= 2 * vmap::kStWords, "the merge counters fit the pinned statistics words");

// What a merge works from: the slots of a table or a list of records, in device memory
struct MergeSource {
    const unsigned long long* words;
    unsigned long long n;
    bool records;
};

// the merge kernel over `from` into `table` (n_slots slots), enqueued behind the clear of the counters (dst's d_stats)
int mg_launch(rgbd360_map* dst, const MergeSource& from, bool sub, const float* pose, int min_count, unsigned long long* table, unsigned long long n_slots,
              bool revive) {
    vmap::MergeParams P;
    memset(&P, 0, sizeof(P));
    if (pose) memcpy(P.pose, pose, sizeof(P.pose));
    P.inv_leaf = dst->inv_leaf;
    P.min_count = (unsigned long long)min_count;
    P.revive = revive ? 1 : 0;
    HIPC(dst, hipMemsetAsync(dst->d_stats, 0, vmap::kMgWords * sizeof(unsigned long long), dst->s->stream));
    const dim3 grid((unsigned)((from.n * vmap::kFields + 255) / 256));
    with_choice<0, 1>(from.records, [&](auto S) {
        with_choice<0, 1>(sub, [&](auto U) {
            with_choice<0, 1>(pose != nullptr, [&](auto Q) {
                hipLaunchKernelGGL((vmap::k_vmap_merge<decltype(S)::value, decltype(U)::value, decltype(Q)::value>), grid, dim3(256), 0, dst->s->stream, P,
                                   from.words, from.n, table, n_slots - 1, dst->d_stats.get());
            });
        });
    });
    HIPC(dst, hipGetLastError());
    return 0;
}
void mg_fill_stats(const rgbd360_map* m, const unsigned long long* w, rgbd360_map_merge_stats* st) {
    if (!st) return;
    auto word = [&](int k) { return w ? (long long)w[k] : 0ll; };
    *st = {word(vmap::kMgVoxRead),  word(vmap::kMgPtsRead),  word(vmap::kMgVoxBelow), word(vmap::kMgPtsBelow),   word(vmap::kMgVoxRange),
           word(vmap::kMgPtsRange), word(vmap::kMgVoxAdded), word(vmap::kMgPtsAdded), word(vmap::kMgVoxNew),     word(vmap::kMgVoxDropped),
           word(vmap::kMgPtsDropped), word(vmap::kMgMissing), word(vmap::kMgUnderflow), m->n_voxels};
}
// how a merge / un-merge ends once its counters `w` are on the host: the map's size brought up to date, the statistics, the status
int mg_close(rgbd360_map* dst, const unsigned long long* w, bool sub, rgbd360_map_merge_stats* stats) {
    if (sub) {
        dst->n_voxels -= (long long)w[vmap::kMgVoxNew];
        if (w[vmap::kMgVoxNew]) dst->may_hold_tombstones = true;
    } else {
        dst->n_voxels += (long long)w[vmap::kMgVoxNew];
    }
    mg_fill_stats(dst, w, stats);
    if (sub && (w[vmap::kMgMissing] || w[vmap::kMgUnderflow])) {
        dst->err = "mismatch: voxels were un-merged that the map does not hold; its content is unspecified, clear it";
        return RGBD360_MAP_MISMATCH;
    }
    if (!sub && w[vmap::kMgVoxDropped]) {
        dst->err = "the map is full: new voxels of the merge were dropped";
        return RGBD360_MAP_FULL;
    }
    return 0;
}
// the launch over `from`, the one wait, the books
int mg_run(rgbd360_map* dst, const MergeSource& from, bool sub, const float* pose, int min_count, rgbd360_map_merge_stats* stats) {
    ++dst->revision;
    if (const int rc = mg_launch(dst, from, sub, pose, min_count, dst->table, dst->n_slots, dst->may_hold_tombstones)) return rc;
    if (const int rc = vmap_read_stats(dst, vmap::kMgWords)) return rc;
    return mg_close(dst, dst->h_stats, sub, stats);
}
// what rgbd360_map_merge / _unmerge / _time_merge refuse before anything is touched; p: the parameters in force
int mg_check(rgbd360_map* dst, rgbd360_map* src, const float* pose, const rgbd360_map_merge_params* params, rgbd360_map_merge_params& p) {
    if (const int rc = vmap_refuse_level(dst)) return rc;
    if (!src) return vmap_fail(dst, -1, "the source map must not be null");
    if (src == dst) return vmap_fail(dst, -1, "a map cannot be merged with itself");
    if (src->ctx != dst->ctx) return vmap_fail(dst, -1, "both maps must belong to one context");
    if (params) p = *params;
    else rgbd360_map_default_merge_params(dst, &p);
    if (p.min_count < 1) return vmap_fail(dst, -1, "min_count must be at least 1");
    if (!pose && memcmp(&src->leaf, &dst->leaf, sizeof(float)) != 0) return vmap_fail(dst, -1, "sum mode (pose == NULL) needs maps of one leaf");
    for (int k = 0; pose && k < 16; ++k)
        if (!std::isfinite(pose[k])) return vmap_fail(dst, -1, "the pose has a non-finite entry");
    return 0;
}
int mg_entry(rgbd360_map* dst, rgbd360_map* src, const float* pose, const rgbd360_map_merge_params* params, rgbd360_map_merge_stats* stats, bool sub) {
    if (!dst) return -1;
    dst->err.clear();
    rgbd360_map_merge_params p;
    if (const int rc = mg_check(dst, src, pose, params, p)) return rc;
    mg_fill_stats(dst, nullptr, stats);
    if (src->n_voxels == 0) return 0;
    hipSetDevice(dst->s->p.device);
    HIPC(dst, dst->d_stats.ensure(vmap::kMgWords));
    return mg_run(dst, {src->table.get(), src->n_slots, false}, sub, pose, p.min_count, stats);
}

}  // namespace

extern "C" void rgbd360_map_default_merge_params(const rgbd360_map*, rgbd360_map_merge_params* p) {
    if (p) p->min_count = 1;
}
extern "C" int rgbd360_map_merge(rgbd360_map* dst, rgbd360_map* src, const float pose[16], const rgbd360_map_merge_params* params,
                                 rgbd360_map_merge_stats* stats) {
    return mg_entry(dst, src, pose, params, stats, false);
}
extern "C" int rgbd360_map_unmerge(rgbd360_map* dst, rgbd360_map* src, const float pose[16], const rgbd360_map_merge_params* params,
                                   rgbd360_map_merge_stats* stats) {
    return mg_entry(dst, src, pose, params, stats, true);
}

extern "C" long long rgbd360_map_records(rgbd360_map* m, long long max_out, uint64_t* records) {
    if (!m) return -1;
    m->err.clear();
    if (max_out < 0) return vmap_fail(m, -1, "max_out must not be negative");
    const size_t n = (size_t)m->n_voxels, n_out = std::min(n, (size_t)max_out);
    if (n_out == 0 || !records) return m->n_voxels;
    hipSetDevice(m->s->p.device);
    // the whole map unsorted (the first max_out of the SORTED map are wanted), then the order of the keys on the host
    HIPC(m, m->mg_records.ensure(n * vmap::kFields));
    unsigned long long* counter = m->d_stats + vmap::kStExtract;
    HIPC(m, hipMemsetAsync(counter, 0, sizeof(unsigned long long), m->s->stream));
    hipLaunchKernelGGL(vmap::k_vmap_records, dim3((unsigned)((m->n_slots + 255) / 256)), dim3(256), 0, m->s->stream, (const unsigned long long*)m->table.get(),
                       m->n_slots, (long long)n, counter, m->mg_records.get());
    HIPC(m, hipGetLastError());
    std::vector<unsigned long long> h(n * vmap::kFields);
    HIPC(m, hipMemcpyAsync(h.data(), m->mg_records, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->s->stream));
    HIPC(m, hipStreamSynchronize(m->s->stream));
    std::vector<size_t> order(n);
    for (size_t k = 0; k < n; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return h[a * vmap::kFields] < h[b * vmap::kFields]; });
    for (size_t o = 0; o < n_out; ++o) memcpy(records + o * vmap::kFields, h.data() + order[o] * vmap::kFields, vmap::kFields * sizeof(unsigned long long));
    return m->n_voxels;
}

extern "C" int rgbd360_map_add_records(rgbd360_map* m, const uint64_t* records, long long n, int on_device, rgbd360_map_merge_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;
    if (n < 0 || n > (1ll << 30)) return vmap_fail(m, -1, "bad record count");
    if (n > 0 && !records) return vmap_fail(m, -1, "records must not be null");
    mg_fill_stats(m, nullptr, stats);
    if (n == 0) return 0;
    hipSetDevice(m->s->p.device);
    const size_t words = (size_t)n * vmap::kFields;
    const unsigned long long* dev = reinterpret_cast<const unsigned long long*>(records);
    if (!on_device) {
        HIPC(m, m->mg_records.ensure(words));
        HIPC(m, hipMemcpyAsync(m->mg_records, records, words * sizeof(unsigned long long), hipMemcpyHostToDevice, m->s->stream));
        dev = m->mg_records;
    }
    HIPC(m, m->d_stats.ensure(vmap::kMgWords));
    // every record against the rules before anything is written
    HIPC(m, hipMemsetAsync(m->d_stats, 0, sizeof(unsigned long long), m->s->stream));
    hipLaunchKernelGGL(vmap::k_vmap_check_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->s->stream, dev, (unsigned long long)n, m->d_stats.get());
    HIPC(m, hipGetLastError());
    if (const int rc = vmap_read_stats(m, 1)) return rc;
    if (m->h_stats[0]) {
        m->err = std::to_string(m->h_stats[0]) + " of " + std::to_string(n) +
                 " records break the table's rules (key, count in 1 .. 2^31 - 1, colour sums <= 255 count, |S| < count 2^32); the map is unchanged";
        return -1;
    }
    return mg_run(m, {dev, (unsigned long long)n, true}, false, nullptr, 1, stats);
}

// measurement (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_time_merge(rgbd360_map* dst, rgbd360_map* src, const float pose[16], int reps, float* avg_us) {
    if (!dst) return -1;
    dst->err.clear();
    rgbd360_map_merge_params p;
    if (const int rc = mg_check(dst, src, pose, nullptr, p)) return rc;
    if (reps < 1 || !avg_us || src->n_voxels == 0) return vmap_fail(dst, -1, "bad arguments");
    hipSetDevice(dst->s->p.device);
    HIPC(dst, dst->d_stats.ensure(vmap::kMgWords));
    DevBuf<unsigned long long> scratch;
    const unsigned long long words = dst->n_slots * vmap::kFields;
    if (scratch.ensure(words) != hipSuccess || src->x_xyz.ensure(3 * (size_t)src->n_voxels + 3) != hipSuccess) {
        (void)hipGetLastError();
        return vmap_fail(dst, -103, "out of memory");
    }
    const MergeSource from = {src->table.get(), src->n_slots, false};
    VmapTimer timer(dst, dst->s->stream);        // made last
    for (int r = 0; r < reps && timer.rc == 0; ++r) {
        hipLaunchKernelGGL(vmap::k_vmap_clear, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, dst->s->stream, scratch.get(), words);
        timer.add(0, [&] { return mg_launch(dst, from, false, pose, p.min_count, scratch, dst->n_slots, false); });
        timer.add(1, [&] { return mg_launch(dst, from, false, pose, p.min_count, scratch, dst->n_slots, false); });
        timer.add(2, [&] { return mg_launch(dst, from, true, pose, p.min_count, scratch, dst->n_slots, false); });
        timer.add(3, [&] {
            const int rc = vmap_launch_extract_scan(src);
            if (rc) dst->err = src->err;
            return rc;
        });
    }
    const int rc = timer.finish(avg_us, 4, reps);
    hipStreamSynchronize(dst->s->stream);        // (the scratch table goes with this call)
    return rc;
}
