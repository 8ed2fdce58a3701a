// map_pyramid.h -- the resident map pyramid and coarse-to-fine ICP against it (rgbd360_map_level, rgbd360_map_align_c2f_*,
// include/rgbd360_hip.h; tests/map_pyramid_reference.py restates both in numpy).  Part of the Frame360 translation unit,
// behind voxel_map.h, map_edit.h, map_align.h and map_align_plane.h, whose table, find_or_claim, input description and loop driver it uses.
//
// Both ICPs match within one leaf (map_align.h), so they capture one leaf; the reference's call sites run their cloud ICP at 0.3 - 0.4 m.
// The coarser maps a wider basin needs are a FUNCTION OF THE TABLE: the sums are integers and i = floorf(w * inv_leaf), so for
// leaf' = leaf * 2^s the index is i >> s (arithmetic) and the sums add.  Level s of a map: leaf * 2^s, inv_leaf * 2^-s, the same box, one
// voxel per distinct (i_x >> s, i_y >> s, i_z >> s) over the live voxels (count > 0), its seven words the integer sums of theirs.  Each
// level is a whole rgbd360_map, so every reader works on it unchanged; rgbd360_map::parent marks it and every writer refuses it.
//
//   k_vmap_coarsen   level s out of level s - 1 (level 0: the parent): the work shrinks geometrically, and integer adds make the result
//                    that of merging level 0 by s.  The source table is read as k_vmap_insert's add phase touches it -- a slot's 64 bytes
//                    by eight consecutive lanes, one word each; key and count reach the other lanes by lane exchange.  For a live slot
//                    lane 0 re-keys (a biased index b becomes (b >> 1) + 2^19) and finds or claims the slot in the destination
//                    (voxel_map.h's find_or_claim: one layout, one hash, one probe bound); lanes 1 .. 7 add their word there with 64-bit
//                    integer atomics.  No floating-point atomics, no fences: the kernel boundary is the synchronisation.  No LDS
//                    pre-merge: the slots of the source arrive in hash order, so a workgroup's 32 slots share next to no destination.
//                    Counters: live slots read, voxels created (claims: the destination starts empty), points carried, voxels dropped;
//                    a wave's counts by ballot / butterfly, the block's through LDS, one global add per block and counter.
//   sizing           the destination has the next power of two at or above twice the live voxels of the level below, at least 1024
//                    slots: at most half full, where a probe run of kMaxProbes does not occur (voxel_map.h, probe bound).  A build
//                    that reports a drop all the same is an error and leaves no level behind.
//   staleness        a level remembers the parent's revision it was built from (lv_rev) and is rebuilt when they differ; a rebuild bumps
//                    the level's own revision, so its brick layer (map_raycast.h) and normal layer (map_normals.h) follow.  One
//                    synchronisation per level built (the size of the next table comes from the counters).  Nothing incremental.
//   c2f              the input is checked and uploaded once, into the parent's staging (MapInput / vmap_check / vmap_to_device); for
//                    s = top_shift .. 0 the loop of map_align.h (icp_run<M>) runs on level s over that one device source, one
//                    synchronisation per level.  A level that ends not OK hands its incoming pose on.  Nothing is written but the levels'
//                    own work buffers: each level's step is the single-level entry on that level, bit for bit.
#pragma once

namespace vmap {

constexpr int kMaxShift = RGBD360_MAP_MAX_SHIFT;
constexpr unsigned long long kMinLevelSlots = 1024;
enum { kCoLive, kCoCreated, kCoPoints, kCoDropped, kCoWords };

// `key` one level up: every unbiased index i becomes i >> 1 (arithmetic); on the biased b = i + 2^20 that is (b >> 1) + 2^19
__host__ __device__ inline unsigned long long coarser_key(unsigned long long key) {
    const unsigned long long h = (unsigned long long)kBias >> 1;
    return pack_key(((key & 0x1fffffull) >> 1) + h, (((key >> 21) & 0x1fffffull) >> 1) + h, ((key >> 42) >> 1) + h);
}

__global__ __launch_bounds__(256) void k_vmap_coarsen(const unsigned long long* __restrict__ src, unsigned long long n_src, unsigned long long* __restrict__ dst,
                                                      unsigned long long mask, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_stat[kCoWords];
    const int t = threadIdx.x, q = t & 7, lane = t & 63, lead = lane & ~7;
    if (t < kCoWords) s_stat[t] = 0;
    __syncthreads();
    // eight lanes per slot: lane q holds word q (a slot past the table reads slot 0 and counts as empty)
    const unsigned long long slot = ((unsigned long long)blockIdx.x * 256 + t) >> 3;
    const bool in = slot < n_src;
    const unsigned long long v = src[(in ? slot : 0) * kFields + q];
    const unsigned long long key = __shfl(v, lead), count = __shfl(v, lead + 1);
    const bool live = in && key != kEmpty && count != 0;      // (count 0: a tombstone)
    long long to = -1;
    bool claimed = false;
    if (live && q == 0) to = find_or_claim(dst, mask, coarser_key(key), claimed);
    to = __shfl(to, lead);
    if (live && to >= 0 && q != 0 && v) atomicAdd(dst + (unsigned long long)to * kFields + q, v);
    // the counters, by the slot's first lane
    const bool first = live && q == 0;
    const unsigned long long n_live = __popcll(__ballot(first)), n_created = __popcll(__ballot(first && claimed)), n_dropped = __popcll(__ballot(first && to < 0));
    unsigned long long points = first && to >= 0 ? count : 0ull;
#pragma unroll
    for (int off = 32; off; off >>= 1) points += __shfl_xor(points, off);
    if (lane == 0 && n_live) {
        atomicAdd(&s_stat[kCoLive], n_live);
        if (n_created) atomicAdd(&s_stat[kCoCreated], n_created);
        if (points) atomicAdd(&s_stat[kCoPoints], points);
        if (n_dropped) atomicAdd(&s_stat[kCoDropped], n_dropped);
    }
    __syncthreads();
    if (t < kCoWords && s_stat[t]) atomicAdd(stats + t, s_stat[t]);
}

}  // namespace vmap

namespace {

static_assert(vmap::kCoWords <= vmap::kStWords, "the build's counters live in the statistics words");

// the table a level built out of `below` gets
unsigned long long pyr_slots(const rgbd360_map* below) {
    unsigned long long n = vmap::kMinLevelSlots;
    while (n < 2ull * (unsigned long long)below->n_voxels) n <<= 1;
    return n;
}
// the build of `lv` out of `below`, enqueued: the clears of the table and of the counters, the kernel; lv's table has lv->n_slots slots
int pyr_launch_build(rgbd360_map* below, rgbd360_map* lv) {
    const unsigned long long words = lv->n_slots * vmap::kFields;
    HIPC(lv, hipMemsetAsync(lv->d_stats, 0, vmap::kCoWords * sizeof(unsigned long long), lv->s->stream));
    hipLaunchKernelGGL(vmap::k_vmap_clear, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, lv->s->stream, lv->table, words);
    hipLaunchKernelGGL(vmap::k_vmap_coarsen, dim3((unsigned)((below->n_slots * vmap::kFields + 255) / 256)), dim3(256), 0, lv->s->stream,
                       (const unsigned long long*)below->table.get(), below->n_slots, lv->table.get(), lv->n_slots - 1, lv->d_stats.get());
    HIPC(lv, hipGetLastError());
    return 0;
}
// level `lv` brought to the content of `below` (complete when the call returns); 0, RGBD360_MAP_FULL, or a negative error in lv->err
int pyr_build(rgbd360_map* below, rgbd360_map* lv) {
    const unsigned long long n_slots = pyr_slots(below);
    if (n_slots != lv->n_slots) {      // (the stream is idle: every entry waits for it before it returns)
        lv->table.release();
        lv->n_slots = 0;
        if (lv->table.ensure(n_slots * vmap::kFields) != hipSuccess) {
            (void)hipGetLastError();
            return vmap_fail(lv, -103, "rgbd360_map_level: out of memory");
        }
        lv->n_slots = n_slots;
    }
    ++lv->revision;
    if (const int rc = pyr_launch_build(below, lv)) return rc;
    if (const int rc = vmap_read_stats(lv, vmap::kCoWords)) return rc;
    const unsigned long long* w = lv->h_stats;
    lv->n_voxels = (long long)w[vmap::kCoCreated];
    lv->may_hold_tombstones = false;
    if (w[vmap::kCoDropped]) return vmap_fail(lv, RGBD360_MAP_FULL, "rgbd360_map_level: voxels found no free slot within the probe bound of the level's table");
    return 0;
}
// levels 1 .. shift of `m` exist and hold its content; on a failure levels from the failing one up are gone and m->err says why
int pyr_refresh(rgbd360_map* m, int shift) {
    hipSetDevice(m->s->p.device);
    for (int s = 1; s <= shift; ++s) {
        if ((int)m->levels.size() < s) {
            std::unique_ptr<rgbd360_map> lv(new rgbd360_map());
            lv->ctx = m->ctx;
            lv->s = m->s;
            lv->leaf = ldexpf(m->leaf, s);
            lv->inv_leaf = ldexpf(m->inv_leaf, -s);
            lv->parent = m;
            lv->shift = s;
            if (lv->d_stats.ensure(vmap::kStWords) != hipSuccess || lv->h_stats.ensure(2 * vmap::kStWords) != hipSuccess) {
                (void)hipGetLastError();
                return vmap_fail(m, -103, "rgbd360_map_level: out of memory");
            }
            m->levels.push_back(std::move(lv));
        }
        rgbd360_map* lv = m->levels[s - 1].get();
        lv->has_box = m->has_box;
        memcpy(lv->lo, m->lo, sizeof(lv->lo));
        memcpy(lv->hi, m->hi, sizeof(lv->hi));
        if (lv->lv_rev == m->revision) continue;
        lv->err.clear();
        if (const int rc = pyr_build(s == 1 ? m : m->levels[s - 2].get(), lv)) {
            m->err = lv->err;
            m->levels.resize(s - 1);
            return rc;
        }
        lv->lv_rev = m->revision;
    }
    return 0;
}

int c2f_check(rgbd360_map* m, const rgbd360_map_c2f_params* params, rgbd360_map_c2f_params& p) {
    if (params) p = *params;
    else rgbd360_map_default_c2f_params(m, &p);
    if (m->parent) return vmap_fail(m, -1, "a level of a map pyramid has no levels of its own");
    if (p.top_shift < 0 || p.top_shift > vmap::kMaxShift) return vmap_fail(m, -1, "top_shift must lie in 0 .. 6");
    if (p.kind != 0 && p.kind != 1) return vmap_fail(m, -1, "kind must be 0 (point-to-point) or 1 (point-to-plane)");
    if (!(p.max_dist_leaves > 0.f && p.max_dist_leaves <= 1.f)) return vmap_fail(m, -1, "max_dist_leaves must lie in (0, 1]");
    return 0;
}
// the parameters of method M on level `lv`
void c2f_level_params(const rgbd360_map* lv, const rgbd360_map_c2f_params& p, rgbd360_map_align_params& out) {
    out = {p.max_dist_leaves * lv->leaf, p.max_iters, p.eps, p.min_count, p.min_matches};
}
void c2f_level_params(const rgbd360_map* lv, const rgbd360_map_c2f_params& p, rgbd360_map_align_plane_params& out) {
    out = {p.max_dist_leaves * lv->leaf, p.max_iters, p.eps, p.min_count, p.min_matches, p.min_support, p.max_flatness};
}

// the chain of method M over the checked parameters p
template <class M>
int c2f_chain(rgbd360_map* m, const MapInput& in, const float guess[16], const rgbd360_map_c2f_params& p, float pose_out[16], rgbd360_map_c2f_result* res) {
    auto level = [&](int s) { return s == 0 ? m : m->levels[s - 1].get(); };
    // every level's parameters are checked before anything is touched
    typename M::Params lp[vmap::kMaxShift + 1];
    for (int s = 0; s <= p.top_shift; ++s) {
        IcpJob job;
        rgbd360_map probe;      // (the level's leaf is all the check reads; the level itself may not exist yet)
        probe.leaf = ldexpf(m->leaf, s);
        c2f_level_params(&probe, p, lp[s]);
        if (const int rc = M::check(&probe, &lp[s], job)) return vmap_fail(m, rc, probe.err.c_str());
    }
    if (!guess || !pose_out) return vmap_fail(m, -1, "guess and pose_out must not be null");
    const int chk = vmap_check(m, in, true);
    if (chk < 0) return chk;
    if (res) {
        memset(res, 0, sizeof(*res));
        res->n_levels = p.top_shift + 1;
        for (int k = 0; k <= p.top_shift; ++k) res->levels[k].shift = p.top_shift - k;
    }
    memcpy(pose_out, guess, 16 * sizeof(float));
    m->a_trace.clear();
    if (chk == 1) {              // nothing to align
        for (int k = 0; res && k <= p.top_shift; ++k) {
            res->levels[k].status = RGBD360_NO_VALID_PIXELS;
            memcpy(res->levels[k].pose, guess, 16 * sizeof(float));
        }
        return RGBD360_NO_VALID_PIXELS;
    }
    if (const int rc = pyr_refresh(m, p.top_shift)) return rc;
    MapSource src;
    if (const int rc = vmap_to_device(m, in, src)) return rc;
    float pose[16];
    memcpy(pose, guess, sizeof(pose));
    int status = 0;
    for (int s = p.top_shift; s >= 0; --s) {
        rgbd360_map* lv = level(s);
        lv->err.clear();
        IcpJob job;
        int rc = M::check(lv, &lp[s], job);
        job.src = src;
        if (rc == 0) rc = icp_buffers(lv, job);
        float ended[16];
        typename M::Result r;
        if (rc == 0) rc = icp_run<M>(lv, job, pose, ended, &r);
        if (rc >= 0 && lv != m) m->a_robust = lv->a_robust;      // (the root reports the finest level run)
        if (rc < 0) {
            if (lv != m) m->err = lv->err;
            return rc;
        }
        if (res) {
            rgbd360_map_c2f_level& o = res->levels[p.top_shift - s];
            o.status = r.status, o.iterations = r.iterations, o.converged = r.converged;
            o.n_valid = r.n_valid, o.n_box_rejected = r.n_box_rejected, o.n_out_of_range = r.n_out_of_range, o.n_matched = r.n_matched;
            o.fitness = r.fitness;
            memcpy(o.pose, ended, sizeof(o.pose));
            if (s == 0) {
                memcpy(res->hessian, r.hessian, sizeof(res->hessian));
                memcpy(res->gradient, r.gradient, sizeof(res->gradient));
            }
        }
        status = rc;
        if (rc == RGBD360_OK || s == 0) memcpy(s == 0 ? pose_out : pose, ended, sizeof(pose));
    }
    return status;
}
int c2f_align(rgbd360_map* m, const MapInput& in, const float guess[16], const rgbd360_map_c2f_params* params, float pose_out[16], rgbd360_map_c2f_result* res) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_c2f_params p;
    if (const int rc = c2f_check(m, params, p)) return rc;
    auto chain = [&](auto M) { return c2f_chain<typename decltype(M)::type>(m, in, guess, p, pose_out, res); };
    return p.kind == 0 ? icp_by_setting<PointIcp>(m, chain) : icp_by_setting<PlaneIcp>(m, chain);
}

}  // namespace

extern "C" int rgbd360_map_level(rgbd360_map* m, int shift, rgbd360_map** level) {
    if (level) *level = nullptr;
    if (!m) return -1;
    m->err.clear();
    if (!level) return vmap_fail(m, -1, "level must not be null");
    if (m->parent) return vmap_fail(m, -1, "a level of a map pyramid has no levels of its own");
    if (shift < 1 || shift > vmap::kMaxShift) return vmap_fail(m, -1, "shift must lie in 1 .. 6");
    if (const int rc = pyr_refresh(m, shift)) return rc;
    *level = m->levels[shift - 1].get();
    return 0;
}
extern "C" size_t rgbd360_map_pyramid_bytes(const rgbd360_map* m) {
    size_t bytes = 0;
    for (size_t k = 0; m && k < m->levels.size(); ++k) bytes += m->levels[k]->table.capacity() * sizeof(unsigned long long);
    return bytes;
}
extern "C" int rgbd360_map_release_levels(rgbd360_map* m) {
    if (!m) return -1;
    m->err.clear();
    if (m->parent) return vmap_fail(m, -1, "a level of a map pyramid has no levels of its own");
    hipSetDevice(m->s->p.device);
    HIPC(m, hipStreamSynchronize(m->s->stream));
    m->levels.clear();
    return 0;
}

extern "C" void rgbd360_map_default_c2f_params(const rgbd360_map* m, rgbd360_map_c2f_params* p) {
    if (!p) return;
    rgbd360_map_align_plane_params single;
    rgbd360_map_default_align_plane_params(m, &single);
    p->top_shift = 3;
    p->kind = 0;
    p->max_iters = single.max_iters;
    p->min_count = single.min_count;
    p->eps = single.eps;
    p->max_dist_leaves = 1.f;
    p->min_matches = single.min_matches;
    p->min_support = single.min_support;
    p->max_flatness = single.max_flatness;
}
extern "C" int rgbd360_map_align_c2f_sphere(rgbd360_map* m, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                            const float guess[16], int on_device, const rgbd360_map_c2f_params* params, float pose_out[16],
                                            rgbd360_map_c2f_result* result) {
    return c2f_align(m, sphere_input(nullptr, 0, depth, depth_step, depth_type, rows, cols, convention, on_device), guess, params, pose_out, result);
}
extern "C" int rgbd360_map_align_c2f_cloud(rgbd360_map* m, const float* xyz, long long n, const float guess[16], int on_device,
                                           const rgbd360_map_c2f_params* params, float pose_out[16], rgbd360_map_c2f_result* result) {
    return c2f_align(m, cloud_input(xyz, nullptr, n, on_device), guess, params, pose_out, result);
}

// measurement (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_time_coarsen(rgbd360_map* m, int top_shift, int reps, float avg_us[8], long long* counters) {
    if (!m) return -1;
    m->err.clear();
    if (m->parent) return vmap_fail(m, -1, "a level of a map pyramid has no levels of its own");
    if (top_shift < 1 || top_shift > vmap::kMaxShift || reps < 1 || !avg_us) return vmap_fail(m, -1, "bad arguments");
    if (const int rc = pyr_refresh(m, top_shift)) return rc;
    for (int s = 1; s <= top_shift && counters; ++s)       // (the counters of the last build of each level: these tables, this content)
        for (int k = 0; k < vmap::kCoWords; ++k) counters[4 * (s - 1) + k] = 0;
    if (m->x_xyz.ensure(3 * (size_t)m->n_voxels + 3) != hipSuccess) {
        (void)hipGetLastError();
        return vmap_fail(m, -103, "out of memory");
    }
    auto below = [&](int s) { return s == 1 ? m : m->levels[s - 2].get(); };
    VmapTimer timer(m, m->s->stream);        // made last
    // (a rebuild over the same source into the same table leaves the same content: the levels stay valid)
    for (int r = 0; r < reps && timer.rc == 0; ++r) {
        for (int s = 1; s <= top_shift; ++s) timer.add(s - 1, [&] { return pyr_launch_build(below(s), m->levels[s - 1].get()); });
        timer.add(6, [&] {
            for (int s = 1; s <= top_shift; ++s)
                if (const int rc = pyr_launch_build(below(s), m->levels[s - 1].get())) return rc;
            return 0;
        });
        timer.add(7, [&] { return vmap_launch_extract_scan(m); });
    }
    for (int s = 1; s <= top_shift && counters && timer.rc == 0; ++s) {
        rgbd360_map* lv = m->levels[s - 1].get();
        if ((timer.rc = vmap_read_stats(lv, vmap::kCoWords)) != 0) break;
        for (int k = 0; k < vmap::kCoWords; ++k) counters[4 * (s - 1) + k] = (long long)lv->h_stats[k];
    }
    return timer.finish(avg_us, 8, reps);
}
