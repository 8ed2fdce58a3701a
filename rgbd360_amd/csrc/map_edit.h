// map_edit.h -- editing the resident voxel map: exact removal, re-posing, rehash and census (rgbd360_map_remove_* / _move_* / _rehash /
// _census, include/rgbd360_hip.h).  Part of the Frame360 translation unit, directly behind voxel_map.h, whose table,
// Source, Params, kernels and input description (MapInput, vmap_check, vmap_to_device) it works with.
//
// What the reference's programs do with a map beyond appending to it: SphereGraphSLAM.cpp and KFsphere_SLAM.cpp optimise their keyframe
// poses continuously (optimizer.optimizeGraph(), getPoses(Map.vOptimizedPoses)) and redraw the map from the corrected poses; a local
// map of the last N frames is the usual odometry target.  Both need frames to LEAVE the map.  The map's sums are integers and steps 1-5
// of an insertion are a pure function of (point, box, pose, leaf): subtracting the same integer terms undoes an insertion exactly,
// whatever was inserted in between.
//
//   removal         k_vmap_insert<SRC, kRemove> (voxel_map.h: one kernel text for both directions).  A slot whose count reaches 0 keeps its
//                   key -- a tombstone, the probe runs stay intact -- and every reader takes count == 0 as absent.  Integer atomics
//                   only, no fences: the kernel boundary is the synchronisation.
//   size            rgbd360_map_size = slots with count > 0.  Removal takes the emptied voxels off it.  An insert into a map that may hold
//                   tombstones (a removal has emptied a voxel since the last clear / rehash) runs as kInsertRevive: a new voxel is the
//                   count add that returned 0, claim or revival -- exactly one add per slot sees 0.  A map that never had a voxel
//                   emptied keeps the claim count and its no-return adds.
//   move            the removal launch at pose_old, then the insert launch (kInsertRevive) at pose_new over ONE upload of the source,
//                   one synchronisation.  No fused kernel: it would save one read of the source and cost a second definition of both phases.
//   k_vmap_rehash   one lane per OLD slot: {key, count} as one 16-byte load, the other three only for live slots (k_vmap_extract's access
//                   shape); find_or_claim in the new table; keys are unique in the old table, so the seven payload words are plain vector
//                   stores and the claim is the only atomic.  A lane that finds no slot within the probe bound raises a counter and the
//                   host swaps the tables only if it stayed 0.
//   k_vmap_census   one lane per slot and step of a grid-stride loop, the four counts kept in registers; at the end a 64-bit wave sum, the
//                   waves' sums through LDS, one atomic per BLOCK and counter.  (One atomic per wave and counter, k_vmap_extract's form, made
//                   the scan cost twice an extract scan -- 647 us against 330 us over 2^21 slots: both are bound by their same-address
//                   atomics, one per wave there, two here -- DESIGN.md 3.15.)
#pragma once

namespace vmap {

enum { kCnLive, kCnTombstones, kCnPoints, kCnInconsistent, kCnWords };

__global__ __launch_bounds__(256) void k_vmap_rehash(const unsigned long long* __restrict__ old_table, unsigned long long n_old,
                                                     unsigned long long* __restrict__ table, unsigned long long mask, unsigned long long* __restrict__ failed) {
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const ulonglong2* rec = reinterpret_cast<const ulonglong2*>(old_table + (s < n_old ? s : 0) * kFields);
    const ulonglong2 kc = rec[0];      // key, count
    const bool live = s < n_old && kc.x != kEmpty && kc.y != 0;
    long long slot = 0;
    if (live) {
        const ulonglong2 s01 = rec[1], s2r = rec[2], sgb = rec[3];
        bool claimed = false;
        slot = find_or_claim(table, mask, kc.x, claimed);
        if (slot >= 0) {
            unsigned long long* out = table + (unsigned long long)slot * kFields;
            out[1] = kc.y;
            ulonglong2* out2 = reinterpret_cast<ulonglong2*>(out);
            out2[1] = s01;
            out2[2] = s2r;
            out2[3] = sgb;
        }
    }
    const unsigned long long lost = __ballot(live && slot < 0);
    if ((threadIdx.x & 63) == 0 && lost) atomicAdd(failed, (unsigned long long)__popcll(lost));
}

constexpr int kCensusBlocks = 2048;      // at most: eight blocks of 256 for each of the 256 compute units

__global__ __launch_bounds__(256) void k_vmap_census(const unsigned long long* __restrict__ table, unsigned long long n_slots, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_part[4][kCnWords];
    unsigned long long n[kCnWords] = {0, 0, 0, 0};
    for (unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x; s < n_slots; s += (unsigned long long)gridDim.x * 256) {
        const ulonglong2* rec = reinterpret_cast<const ulonglong2*>(table + s * kFields);
        const ulonglong2 kc = rec[0];      // key, count
        if (kc.x == kEmpty) continue;
        const bool live = kc.y != 0;
        const ulonglong2 w[3] = {rec[1], rec[2], rec[3]};
        const unsigned long long S[3] = {w[0].x, w[0].y, w[1].x}, col[3] = {w[1].y, w[2].x, w[2].y};
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned long long mag = (long long)S[k] < 0 ? 0ull - S[k] : S[k];
            // count == 0: any sum left over; otherwise |S_k| >= count 2^32 (|w| < 4096 at 2^20) or a colour sum above 255 count
            bad = bad || (live ? (mag >> 32) >= kc.y || col[k] / 255ull > kc.y || (col[k] / 255ull == kc.y && col[k] % 255ull != 0) : (S[k] | col[k]) != 0);
        }
        n[kCnLive] += live ? 1 : 0;
        n[kCnTombstones] += live ? 0 : 1;
        n[kCnPoints] += kc.y;
        n[kCnInconsistent] += bad ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < kCnWords; ++q) {
#pragma unroll
        for (int off = 32; off; off >>= 1) n[q] += __shfl_xor(n[q], off);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][q] = n[q];
    }
    __syncthreads();
    if (threadIdx.x < kCnWords) {      // one add per block and counter
        const unsigned long long v = (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
        if (v) atomicAdd(out + threadIdx.x, v);
    }
}

}  // namespace vmap

namespace {

void vmap_fill_edit_stats(const rgbd360_map* m, const unsigned long long* w, rgbd360_map_edit_stats* st) {
    if (!st) return;
    st->n_valid = w ? (long long)w[vmap::kStValid] : 0;
    st->n_box_rejected = w ? (long long)w[vmap::kStBox] : 0;
    st->n_out_of_range = w ? (long long)w[vmap::kStRange] : 0;
    st->n_removed = w ? (long long)w[vmap::kStAdded] : 0;
    st->n_missing = w ? (long long)w[vmap::kStDropped] : 0;
    st->n_underflow = w ? (long long)w[vmap::kStUnderflow] : 0;
    st->n_voxels_emptied = w ? (long long)w[vmap::kStNew] : 0;
    st->n_voxels = m->n_voxels;
}
// how a removal ends once its counters `w` are on the host: the map's size brought up to date, the statistics, the status
int vmap_close_remove(rgbd360_map* m, const unsigned long long* w, rgbd360_map_edit_stats* stats) {
    m->n_voxels -= (long long)w[vmap::kStNew];
    if (w[vmap::kStNew]) m->may_hold_tombstones = true;
    vmap_fill_edit_stats(m, w, stats);
    if (w[vmap::kStDropped] || w[vmap::kStUnderflow]) {
        m->err = "mismatch: points were removed that the map does not hold; its content is unspecified, clear it";
        return RGBD360_MAP_MISMATCH;
    }
    return 0;
}
// the launches of an edit over `src`: the removal at pose_old, then (pose_new != null: a move) the insertion at pose_new; one wait
int vmap_edit(rgbd360_map* m, const MapSource& src, const float* pose_old, const float* pose_new, rgbd360_map_edit_stats* removed, rgbd360_map_stats* inserted) {
    unsigned long long* h = m->h_stats;
    if (const int rc = vmap_launch(m, vmap_params(m, pose_old), src, vmap::kRemove)) return rc;
    if (const int rc = vmap_copy_stats(m, vmap::kStWords, vmap::kStWords)) return rc;
    if (pose_new) {      // (whether the removal leaves tombstones is not known yet: revivals are counted)
        if (const int rc = vmap_launch(m, vmap_params(m, pose_new), src, vmap::kInsertRevive)) return rc;
        if (const int rc = vmap_copy_stats(m, vmap::kStWords)) return rc;
    }
    HIPC(m, hipStreamSynchronize(m->s->stream));
    const int rc_remove = vmap_close_remove(m, h + vmap::kStWords, removed);
    if (!pose_new) return rc_remove;
    const std::string err_remove = m->err;
    const int rc_insert = vmap_close_insert(m, h, inserted);
    if (rc_remove && rc_insert) m->err = err_remove + "; " + m->err;
    else if (rc_remove) m->err = err_remove;
    if (removed) removed->n_voxels = m->n_voxels;      // both statistics: the size after the call
    return std::max(rc_remove, rc_insert);
}
// a remove call, or (move) a move call: rgbd360_map_remove_* / _move_*
int vmap_edit_entry(rgbd360_map* m, const MapInput& in, const float* pose_old, const float* pose_new, bool move, rgbd360_map_edit_stats* removed,
                    rgbd360_map_stats* inserted) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;
    const int chk = vmap_check(m, in, pose_old && (!move || pose_new));
    if (chk < 0) return chk;
    vmap_fill_edit_stats(m, nullptr, removed);
    vmap_fill_stats(m, nullptr, inserted);
    if (chk == 1) return 0;
    MapSource src;
    if (const int rc = vmap_to_device(m, in, src)) return rc;
    return vmap_edit(m, src, pose_old, move ? pose_new : nullptr, removed, inserted);
}
// the census launch over the table, enqueued; its counters land in d_stats[0 .. kCnWords)
int vmap_launch_census(rgbd360_map* m) {
    HIPC(m, hipMemsetAsync(m->d_stats, 0, vmap::kCnWords * sizeof(unsigned long long), m->s->stream));
    const unsigned long long blocks = std::min<unsigned long long>((m->n_slots + 255) / 256, vmap::kCensusBlocks);
    hipLaunchKernelGGL(vmap::k_vmap_census, dim3((unsigned)blocks), dim3(256), 0, m->s->stream, m->table, m->n_slots, m->d_stats);
    HIPC(m, hipGetLastError());
    return 0;
}
// the table rebuilt into `fresh` (n_slots slots, allocated): clear and k_vmap_rehash enqueued, the failure counter in d_stats[0]
int vmap_launch_rehash(rgbd360_map* m, unsigned long long* fresh, unsigned long long n_slots) {
    const unsigned long long words = n_slots * vmap::kFields;
    HIPC(m, hipMemsetAsync(m->d_stats, 0, sizeof(unsigned long long), m->s->stream));
    hipLaunchKernelGGL(vmap::k_vmap_clear, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, m->s->stream, fresh, words);
    hipLaunchKernelGGL(vmap::k_vmap_rehash, dim3((unsigned)((m->n_slots + 255) / 256)), dim3(256), 0, m->s->stream, m->table, m->n_slots, fresh, n_slots - 1,
                       m->d_stats);
    HIPC(m, hipGetLastError());
    return 0;
}
static_assert(vmap::kCnWords <= vmap::kStWords, "the census counters live in the statistics words");

}  // namespace

extern "C" int rgbd360_map_remove_sphere(rgbd360_map* m, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type,
                                         int rows, int cols, int convention, const float pose[16], int on_device, rgbd360_map_edit_stats* stats) {
    return vmap_edit_entry(m, sphere_input(rgb, rgb_step, depth, depth_step, depth_type, rows, cols, convention, on_device), pose, nullptr, false, stats, nullptr);
}
extern "C" int rgbd360_map_remove_cloud(rgbd360_map* m, const float* xyz, const uint8_t* rgb3, long long n, const float pose[16], int on_device,
                                        rgbd360_map_edit_stats* stats) {
    return vmap_edit_entry(m, cloud_input(xyz, rgb3, n, on_device), pose, nullptr, false, stats, nullptr);
}
extern "C" int rgbd360_map_move_sphere(rgbd360_map* m, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type, int rows,
                                       int cols, int convention, const float pose_old[16], const float pose_new[16], int on_device,
                                       rgbd360_map_edit_stats* removed, rgbd360_map_stats* inserted) {
    return vmap_edit_entry(m, sphere_input(rgb, rgb_step, depth, depth_step, depth_type, rows, cols, convention, on_device), pose_old, pose_new, true, removed,
                           inserted);
}
extern "C" int rgbd360_map_move_cloud(rgbd360_map* m, const float* xyz, const uint8_t* rgb3, long long n, const float pose_old[16], const float pose_new[16],
                                      int on_device, rgbd360_map_edit_stats* removed, rgbd360_map_stats* inserted) {
    return vmap_edit_entry(m, cloud_input(xyz, rgb3, n, on_device), pose_old, pose_new, true, removed, inserted);
}

extern "C" int rgbd360_map_rehash(rgbd360_map* m, long long capacity_voxels) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;
    if (capacity_voxels < 0 || capacity_voxels > (1ll << 30)) return vmap_fail(m, -1, "capacity must be 0 (the current size) or 1 .. 2^30 voxels");
    unsigned long long n_slots = capacity_voxels ? 1 : m->n_slots;
    while (n_slots < (unsigned long long)capacity_voxels) n_slots <<= 1;
    if (n_slots < (unsigned long long)m->n_voxels) return vmap_fail(m, -1, "the capacity is below the number of occupied voxels");
    hipSetDevice(m->s->p.device);
    DevBuf<unsigned long long> fresh;
    if (fresh.ensure(n_slots * vmap::kFields) != hipSuccess) {
        (void)hipGetLastError();
        return vmap_fail(m, -103, "rgbd360_map_rehash: out of memory");
    }
    if (const int rc = vmap_launch_rehash(m, fresh, n_slots)) return rc;
    if (const int rc = vmap_read_stats(m, 1)) return rc;
    if (m->h_stats[0]) {      // (the new table goes with `fresh`)
        m->err = "rehash: voxels found no free slot within the probe bound of the new table; the map is unchanged";
        return RGBD360_MAP_FULL;
    }
    m->table = std::move(fresh);      // (the old table goes with `fresh`; the stream is idle)
    m->n_slots = n_slots;
    m->may_hold_tombstones = false;
    ++m->revision;
    vmap_drop_votes(m);      // (they are per slot)
    return 0;
}

extern "C" int rgbd360_map_census(rgbd360_map* m, rgbd360_map_census_counts* out) {
    if (!m) return -1;
    m->err.clear();
    if (!out) return vmap_fail(m, -1, "out must not be null");
    hipSetDevice(m->s->p.device);
    if (const int rc = vmap_launch_census(m)) return rc;
    if (const int rc = vmap_read_stats(m, vmap::kCnWords)) return rc;
    const unsigned long long* w = m->h_stats;
    *out = {(long long)m->n_slots, (long long)w[vmap::kCnLive], (long long)w[vmap::kCnTombstones], (long long)w[vmap::kCnPoints],
            (long long)w[vmap::kCnInconsistent]};
    return 0;
}

// measurement (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_time_edit(rgbd360_map* m, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev, size_t depth_step, int depth_type,
                                     int rows, int cols, int convention, const float pose[16], int reps, float avg_us[7]) {
    if (!m) return -1;
    m->err.clear();
    if (const int rc = vmap_refuse_level(m)) return rc;      // (it clears, fills and edits the map)
    const MapInput in = sphere_input(rgb_dev, rgb_step, depth_dev, depth_step, depth_type, rows, cols, convention, 1);
    if (const int rc = vmap_check_timed(m, in, pose, reps, avg_us)) return rc;
    MapSource src;
    if (const int rc = vmap_to_device(m, in, src)) return rc;
    const vmap::Params P = vmap_params(m, pose);
    DevBuf<unsigned long long> fresh;
    if (fresh.ensure(m->n_slots * vmap::kFields) != hipSuccess) {
        (void)hipGetLastError();
        return vmap_fail(m, -103, "out of memory");
    }
    VmapTimer timer(m, m->s->stream);
    int& rc = timer.rc;
    rgbd360_map_stats st;
    rgbd360_map_edit_stats est;
    auto close_insert = [&] {
        if (rc == 0) rc = std::min(vmap_finish_insert(m, &st), 0);
    };
    for (int r = 0; r < reps && rc == 0; ++r) {
        // the map holds the frame twice: a removal leaves every voxel live, as in a window of overlapping frames
        if ((rc = vmap_clear_dev(m)) != 0) break;
        if ((rc = vmap_launch(m, P, src, vmap::kInsert)) != 0) break;
        close_insert();
        timer.add(0, [&] { return vmap_launch(m, P, src, vmap::kInsert); });            // the claim count, populated map
        close_insert();
        timer.add(1, [&] { return vmap_launch(m, P, src, vmap::kRemove); });            // the removal kernel, same map
        if (rc == 0) rc = vmap_read_stats(m, vmap::kStWords);
        if (rc == 0) rc = std::min(vmap_close_remove(m, m->h_stats, &est), 0);
        timer.add(2, [&] { return vmap_launch(m, P, src, vmap::kInsertRevive); });      // the returning count add, populated map
        close_insert();
        if (rc == 0 && m->x_xyz.ensure(3 * (size_t)m->n_voxels + 3) != hipSuccess) rc = vmap_fail(m, -103, "out of memory");
        timer.add(3, [&] { return vmap_launch_rehash(m, fresh, m->n_slots); });        // clear of the new table + k_vmap_rehash
        timer.add(4, [&] { return vmap_launch_census(m); });
        timer.add(5, [&] { return vmap_launch_extract_scan(m); });                     // (with the clear of its counter, as in every extract call)
        // a whole move call from device memory, enqueue to synchronisation: both launches and the one wait
        timer.add(6, [&] { return std::min(vmap_edit(m, src, pose, pose, &est, &st), 0); });
    }
    return timer.finish(avg_us, 7, reps);
}
