// map_planes.h -- planar regions of the resident voxel map (voxel_map.h): connected components of the occupied voxels under the per-voxel
// normals of map_normals.h, each flat enough component an rgbd360_plane -- a PbMap of the global map, the operand that
// rgbd360_register_planes needs to place a frame in the map without an initial guess (the reference's Relocalizer360,
// Relocalizer360.h:78-93).  Part of the Frame360 translation unit, behind map_normals.h (its layer, its record) and the Frame360 host
// code whose region fit and hull it calls (region_fit_moments, apply_extent, apply_hull) and whose union-find it runs (f360::uf_union).
//
// Definition: include/rgbd360_hip.h, "planar regions of the map"; tests/map_planes_reference.py restates it.  A function
// of the voxel set and the parameters alone.  The table is never written.
//
// The label layer: 32 bytes per table slot (PlLayer below), owned by the map, built by the first call that needs it and reused while the
// map's revision word and the parameters stand.  One lane per slot in every pass over the table; slots are not compacted (at most half
// are live; a wave without a live slot ends at once).  Counters through ballots or wave sums, one integer atomic per wave and counter; no
// floating-point atomics anywhere.
//
//   k_vmap_pl_init      parent[s] = s, the per-root words cleared.
//   k_vmap_pl_link      an eligible voxel looks up its 13 neighbours of larger key -- the first probes of all 13 in flight before any is
//                       examined, as search27 does -- and joins each linked one with f360::uf_union (atomicMin; parents have the smaller
//                       slot index).
//   k_vmap_pl_compress  parent[s] = the root slot (-1: not eligible, so that no later pass needs the normal layer), and the smallest key
//                       of the region at the root slot by atomicMin, tried only where the word read is larger: the slot-independent label.
//   k_vmap_pl_count     N, P and the extent E per root (the range rule's inputs), merged per wave by region first (wave_add_by_key).
//   k_vmap_pl_roots     the roots with N >= min_voxels compacted into region ids (a wave reserves its range with one counter add), each
//                       with its key, N, E, P and the root voxel's centroid; the host sorts the few of them by key and applies the range
//                       rule before any sum is read.
//   k_vmap_pl_sums      the nine integer sums of a member into its region's row; a wave first merges the members of equal region ids
//                       (one large wall puts thousands of voxels on one accumulator: measured in DESIGN.md 3.24 with and without).
//   k_vmap_pl_scatter   the members of the planes that passed, as (u, v, key) in the plane's frame, into one contiguous list per plane.
//   k_vmap_pl_extremes  one workgroup per chunk of a list: eight waves walk it, lane k keeps the extreme of direction k; the same kernel
//                       then reduces the chunks' winners of every plane.  No atomics.
//   k_vmap_pl_labels    the shape of k_vmap_normals_extract with the label and the plane's ordinal.
#pragma once

namespace vmap {

constexpr int kPlThreads = 256, kPlExtThreads = 512;
constexpr int kPlRootWords = 8;       // per qualifying region: key, N | E << 32, P, the root centroid's bits (x | y << 32, z), three spare
constexpr int kPlMemberWords = 3;     // u and v (the bits of two doubles) and the key
constexpr unsigned long long kPlChunk = 8192;      // members a workgroup of k_vmap_pl_extremes reduces
constexpr int kPlFrameFloats = 12;    // origin, e1, e2, three spare
constexpr double kPlFix = 65536.0;    // q_k = rint((c_k - r_k) 2^16)
enum { kPlVoxels, kPlEligible, kPlLinks, kPlRegions, kPlQualify, kPlLabels, kPlWords };

// the layer: per slot the region's smallest key and point count (meaningful at a root slot), the root slot (-1: not eligible), and at a
// root slot the region's voxel count, extent and id among the qualifying regions (-1: none)
struct PlLayer {
    unsigned long long *rmin, *rpts;
    int* parent;
    unsigned *rn, *rext;
    int* rid;
};
struct PlDirs {
    short d[64][2];
};

__device__ __forceinline__ bool pl_eligible(const uint4 r, float max_voxel_curvature) {
    const NormalRec R = normal_unpack(r);
    return R.status == kClassKept && R.curvature <= max_voxel_curvature;
}
// the link predicate of two eligible voxels (normals nu, nv; centroids cu, cv): symmetric bit for bit
__device__ __forceinline__ bool pl_linked(const float nu[3], const float cu[3], const float nv[3], const float cv[3], double cos_angle, double bound) {
#pragma clang fp contract(off)
    const double ax = (double)nu[0], ay = (double)nu[1], az = (double)nu[2], bx = (double)nv[0], by = (double)nv[1], bz = (double)nv[2];
    if (!(fabs((ax * bx + ay * by) + az * bz) >= cos_angle)) return false;
    const double ex = (double)cv[0] - (double)cu[0], ey = (double)cv[1] - (double)cu[1], ez = (double)cv[2] - (double)cu[2];
    return fabs((ax * ex + ay * ey) + az * ez) <= bound && fabs((bx * ex + by * ey) + bz * ez) <= bound;
}
// neighbour c of the 13 with a larger key: positions 14 .. 26 of the nested dz / dy / dx loops (13 is the centre)
__device__ __forceinline__ void pl_cell(int c, int& dx, int& dy, int& dz) {
    const int q = 14 + c;
    dx = q % 3 - 1;
    dy = q / 3 % 3 - 1;
    dz = q / 9 - 1;
}

// W integer terms of every active lane added to row `key` of `rows` (W words per row).  merge: the lanes of equal key are summed over the
// wave first and their first lane adds once -- a loop over the distinct keys of the wave, one turn where all lanes share a region.
// Called by all 64 lanes.
template <int W>
__device__ __forceinline__ void wave_add_by_key(bool active, int key, const long long v[W], unsigned long long* __restrict__ rows, bool merge) {
    if (!merge) {
        if (active) {
#pragma unroll
            for (int q = 0; q < W; ++q) atomicAdd(rows + (size_t)key * W + q, (unsigned long long)v[q]);
        }
        return;
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int first = __builtin_ctzll(todo);
        const int k0 = __shfl(key, first);
        const bool mine = active && key == k0;
        const unsigned long long grp = __ballot(mine);
        if (__popcll(grp) == 1) {
            if (mine) {
#pragma unroll
                for (int q = 0; q < W; ++q) atomicAdd(rows + (size_t)key * W + q, (unsigned long long)v[q]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const long long t = f360::wave_sum_ll(mine ? v[q] : 0ll);
                if (lane == first) atomicAdd(rows + (size_t)k0 * W + q, (unsigned long long)t);
            }
        }
        todo &= ~grp;
    }
}

__global__ __launch_bounds__(kPlThreads) void k_vmap_pl_init(unsigned long long n_slots, PlLayer L) {
    const unsigned long long s = (unsigned long long)blockIdx.x * kPlThreads + threadIdx.x;
    if (s >= n_slots) return;
    L.rmin[s] = kEmpty;
    L.rpts[s] = 0;
    L.parent[s] = (int)s;
    L.rn[s] = 0;
    L.rext[s] = 0;
    L.rid[s] = -1;
}

__global__ __launch_bounds__(kPlThreads) void k_vmap_pl_link(const unsigned long long* __restrict__ table, unsigned long long n_slots,
                                                             const uint4* __restrict__ normals, float max_voxel_curvature, double cos_angle,
                                                             double bound, int* __restrict__ parent, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    const unsigned long long s = (unsigned long long)blockIdx.x * kPlThreads + threadIdx.x;
    const bool in = s < n_slots;
    const unsigned long long at = in ? s : 0;
    const unsigned long long* rec = table + at * kFields;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(rec);      // key, count
    const bool live = in && kc.x != kEmpty && kc.y != 0;
    const unsigned long long b_live = __ballot(live);
    if (!b_live) return;
    const NormalRec R = normal_unpack(normals[at]);
    const bool elig = live && R.status == kClassKept && R.curvature <= max_voxel_curvature;
    const unsigned long long mask = n_slots - 1;
    unsigned links = 0;
    if (elig) {
        float cu[3];
        centroid(rec, kc.y, cu);
        const long long ib[3] = {(long long)(kc.x & 0x1fffffull), (long long)((kc.x >> 21) & 0x1fffffull), (long long)(kc.x >> 42)};
        unsigned long long k0[13];
#pragma unroll
        for (int c = 0; c < 13; ++c) {
            int dx, dy, dz;
            pl_cell(c, dx, dy, dz);
            const long long nx = ib[0] + dx, ny = ib[1] + dy, nz = ib[2] + dz;
            const bool ok = nx >= 0 && nx < (1ll << 21) && ny >= 0 && ny < (1ll << 21) && nz >= 0 && nz < (1ll << 21);
            k0[c] = ok ? table[(mix64(pack_key(nx, ny, nz)) & mask) * kFields] : kEmpty;
        }
#pragma unroll
        for (int c = 0; c < 13; ++c) {
            if (k0[c] == kEmpty) continue;       // an empty first slot, or no key at all: no neighbour
            int dx, dy, dz;
            pl_cell(c, dx, dy, dz);
            const unsigned long long ck = pack_key(ib[0] + dx, ib[1] + dy, ib[2] + dz);
            unsigned probes = 0;
            const long long slot = find(table, mask, ck, mix64(ck) & mask, k0[c], probes);
            if (slot < 0) continue;
            const unsigned long long* nrec = table + (unsigned long long)slot * kFields;
            const unsigned long long cnt = nrec[1];
            if (cnt == 0) continue;              // a tombstone
            const NormalRec Rv = normal_unpack(normals[slot]);
            if (!(Rv.status == kClassKept && Rv.curvature <= max_voxel_curvature)) continue;
            float cv[3];
            centroid(nrec, cnt, cv);
            if (!pl_linked(R.n, cu, Rv.n, cv, cos_angle, bound)) continue;
            ++links;
            f360::uf_union(parent, (int)s, (int)slot);
        }
    }
    const unsigned long long b_elig = __ballot(elig);
#pragma unroll
    for (int off = 32; off; off >>= 1) links += __shfl_xor(links, off);
    if ((threadIdx.x & 63) == 0) {      // one add per wave and counter
        atomicAdd(stats + kPlVoxels, (unsigned long long)__popcll(b_live));
        if (b_elig) atomicAdd(stats + kPlEligible, (unsigned long long)__popcll(b_elig));
        if (links) atomicAdd(stats + kPlLinks, (unsigned long long)links);
    }
}

__global__ __launch_bounds__(kPlThreads) void k_vmap_pl_compress(const unsigned long long* __restrict__ table, unsigned long long n_slots,
                                                                 const uint4* __restrict__ normals, float max_voxel_curvature, PlLayer L) {
    const unsigned long long s = (unsigned long long)blockIdx.x * kPlThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = s < n_slots;
    const unsigned long long at = in ? s : 0;
    const bool elig = in && pl_eligible(normals[at], max_voxel_curvature);      // (an empty slot and a tombstone have no normal)
    int r = -1;
    if (elig) r = f360::uf_find(L.parent, (int)s);
    if (in) L.parent[s] = r;
    unsigned long long todo = __ballot(elig);
    if (!todo) return;
    const unsigned long long key = elig ? table[at * kFields] : kEmpty;
    while (todo) {       // the smallest key of each region among the wave's lanes, then one atomic per region
        const int first = __builtin_ctzll(todo);
        const int r0 = __shfl(r, first);
        const bool mine = elig && r == r0;
        const unsigned long long grp = __ballot(mine);
        unsigned long long k = mine ? key : kEmpty;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const unsigned long long o = __shfl_xor(k, off);
            k = o < k ? o : k;
        }
        // a minimum only shrinks: a word already as small makes the atomic a no-op, and a stale read only costs one
        if (lane == first && L.rmin[r0] > k) atomicMin(L.rmin + r0, k);
        todo &= ~grp;
    }
}

__global__ __launch_bounds__(kPlThreads) void k_vmap_pl_count(const unsigned long long* __restrict__ table, unsigned long long n_slots, PlLayer L) {
    const unsigned long long s = (unsigned long long)blockIdx.x * kPlThreads + threadIdx.x;
    const bool in = s < n_slots;
    const unsigned long long at = in ? s : 0;
    const int r = in ? L.parent[at] : -1;
    const bool elig = r >= 0;
    if (!__ballot(elig)) return;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(table + at * kFields);
    unsigned ext = 0;
    if (elig) {
        int32_t a[3], b[3];
        unpack_key3(kc.x, a);
        unpack_key3(L.rmin[r], b);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned d = (unsigned)(a[k] > b[k] ? a[k] - b[k] : b[k] - a[k]);
            ext = d > ext ? d : ext;
        }
    }
    // N, P and E of the region: the lanes of one region first summed (the extent: maximised) over the wave
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(elig);
    while (todo) {
        const int first = __builtin_ctzll(todo);
        const int r0 = __shfl(r, first);
        const bool mine = elig && r == r0;
        const unsigned long long grp = __ballot(mine);
        const long long pts = f360::wave_sum_ll(mine ? (long long)kc.y : 0ll);
        unsigned e = mine ? ext : 0u;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const unsigned o = __shfl_xor(e, off);
            e = o > e ? o : e;
        }
        if (lane == first) {
            atomicAdd(L.rn + r0, (unsigned)__popcll(grp));
            atomicAdd(L.rpts + r0, (unsigned long long)pts);
            if (L.rext[r0] < e) atomicMax(L.rext + r0, e);      // (a maximum only grows: a word already as large makes the atomic a no-op)
        }
        todo &= ~grp;
    }
}

__global__ __launch_bounds__(kPlThreads) void k_vmap_pl_roots(const unsigned long long* __restrict__ table, unsigned long long n_slots, PlLayer L,
                                                              unsigned min_voxels, unsigned long long cap, unsigned long long* __restrict__ roots,
                                                              unsigned long long* __restrict__ stats) {
    const unsigned long long s = (unsigned long long)blockIdx.x * kPlThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = s < n_slots;
    const unsigned long long at = in ? s : 0;
    const bool root = in && L.parent[at] == (int)at;
    const unsigned long long b_root = __ballot(root);
    if (!b_root) return;
    const unsigned n = root ? L.rn[at] : 0u;
    const bool qualifies = root && n >= min_voxels;
    const unsigned long long b_q = __ballot(qualifies);
    unsigned long long base = 0;
    if (lane == 0) {
        atomicAdd(stats + kPlRegions, (unsigned long long)__popcll(b_root));
        if (b_q) base = atomicAdd(stats + kPlQualify, (unsigned long long)__popcll(b_q));      // one add per wave
    }
    base = __shfl(base, 0);
    const unsigned long long id = base + (unsigned long long)__popcll(b_q & ((1ull << lane) - 1ull));
    if (!qualifies || id >= cap) return;
    L.rid[at] = (int)id;
    const unsigned long long mask = n_slots - 1, key = L.rmin[at], h = mix64(key) & mask;
    unsigned probes = 0;
    long long slot = find(table, mask, key, h, table[h * kFields], probes);      // the root voxel: a member, so it is there
    if (slot < 0) slot = (long long)at;
    const unsigned long long* rec = table + (unsigned long long)slot * kFields;
    float c[3];
    centroid(rec, rec[1] ? rec[1] : 1ull, c);
    unsigned long long* o = roots + id * kPlRootWords;
    o[0] = key;
    o[1] = (unsigned long long)n | ((unsigned long long)L.rext[at] << 32);
    o[2] = L.rpts[at];
    o[3] = (unsigned long long)__float_as_uint(c[0]) | ((unsigned long long)__float_as_uint(c[1]) << 32);
    o[4] = (unsigned long long)__float_as_uint(c[2]);
    o[5] = o[6] = o[7] = 0;
}

__global__ __launch_bounds__(kPlThreads) void k_vmap_pl_sums(const unsigned long long* __restrict__ table, unsigned long long n_slots, PlLayer L,
                                                             const unsigned long long* __restrict__ roots, unsigned long long* __restrict__ sums,
                                                             int merge) {
#pragma clang fp contract(off)
    const unsigned long long s = (unsigned long long)blockIdx.x * kPlThreads + threadIdx.x;
    const bool in = s < n_slots;
    const unsigned long long at = in ? s : 0;
    const int r = in ? L.parent[at] : -1;
    const int id = r >= 0 ? L.rid[r] : -1;
    const bool active = id >= 0;
    if (!__ballot(active)) return;
    long long v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (active) {
        const unsigned long long* rec = table + at * kFields;
        float c[3];
        centroid(rec, rec[1] ? rec[1] : 1ull, c);
        const unsigned long long w3 = roots[(size_t)id * kPlRootWords + 3], w4 = roots[(size_t)id * kPlRootWords + 4];
        const float rc[3] = {__uint_as_float((unsigned)w3), __uint_as_float((unsigned)(w3 >> 32)), __uint_as_float((unsigned)w4)};
        long long q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = llrint(((double)c[k] - (double)rc[k]) * kPlFix);
        v[0] = q[0], v[1] = q[1], v[2] = q[2];
        v[3] = q[0] * q[0], v[4] = q[0] * q[1], v[5] = q[0] * q[2];
        v[6] = q[1] * q[1], v[7] = q[1] * q[2], v[8] = q[2] * q[2];
    }
    wave_add_by_key<9>(active, id, v, sums, merge != 0);
}

__global__ __launch_bounds__(kPlThreads) void k_vmap_pl_scatter(const unsigned long long* __restrict__ table, unsigned long long n_slots, PlLayer L,
                                                                const int* __restrict__ plane_of, const float* __restrict__ frames,
                                                                const unsigned long long* __restrict__ offset, int* __restrict__ cursor,
                                                                unsigned long long* __restrict__ members) {
#pragma clang fp contract(off)
    const unsigned long long s = (unsigned long long)blockIdx.x * kPlThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = s < n_slots;
    const unsigned long long at = in ? s : 0;
    const int r = in ? L.parent[at] : -1;
    const int id = r >= 0 ? L.rid[r] : -1;
    const int a = id >= 0 ? plane_of[id] : -1;
    const bool active = a >= 0;
    unsigned long long todo = __ballot(active);
    if (!todo) return;
    unsigned long long place = 0;
    while (todo) {       // a wave reserves its places in a plane's list with one add per plane
        const int first = __builtin_ctzll(todo);
        const int a0 = __shfl(a, first);
        const bool mine = active && a == a0;
        const unsigned long long grp = __ballot(mine);
        int base = 0;
        if (lane == first) base = atomicAdd(cursor + a0, __popcll(grp));
        base = __shfl(base, first);
        if (mine) place = (unsigned long long)base + (unsigned long long)__popcll(grp & ((1ull << lane) - 1ull));
        todo &= ~grp;
    }
    if (!active) return;
    const unsigned long long lo = offset[a], hi = offset[a + 1];
    if (lo + place >= hi) return;      // (the list holds the region's N members: never)
    const unsigned long long* rec = table + at * kFields;
    float c[3];
    centroid(rec, rec[1] ? rec[1] : 1ull, c);
    const float* F = frames + (size_t)a * kPlFrameFloats;
    const double d0 = (double)c[0] - (double)F[0], d1 = (double)c[1] - (double)F[1], d2 = (double)c[2] - (double)F[2];
    const double u = (d0 * (double)F[3] + d1 * (double)F[4]) + d2 * (double)F[5];
    const double v = (d0 * (double)F[6] + d1 * (double)F[7]) + d2 * (double)F[8];
    unsigned long long* o = members + (lo + place) * kPlMemberWords;
    o[0] = (unsigned long long)__double_as_longlong(u);
    o[1] = (unsigned long long)__double_as_longlong(v);
    o[2] = rec[0];
}

// One workgroup per range of a member list (ranges[2 b], ranges[2 b + 1]): wave w walks members w, w + 8, ..., every lane reading the same
// member, lane k keeping the extreme of direction k -- the largest u a_k + v b_k, a tie going to the smaller key; the eight waves meet in
// LDS.  The 64 winners leave as members themselves (u, v, key), so the same kernel reduces the winners of a plane's chunks to the plane's
// extremes: a maximum with a total tie rule does not care how the list was cut.  No atomics.
__global__ __launch_bounds__(kPlExtThreads) void k_vmap_pl_extremes(const unsigned long long* __restrict__ members,
                                                                    const unsigned long long* __restrict__ ranges, unsigned long long* __restrict__ out,
                                                                    PlDirs dirs) {
#pragma clang fp contract(off)
    constexpr int kWaves = kPlExtThreads / 64;
    __shared__ double s_pr[kWaves][64], s_u[kWaves][64], s_v[kWaves][64];
    __shared__ unsigned long long s_key[kWaves][64];
    const int b = blockIdx.x, k = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double A = (double)dirs.d[k][0], B = (double)dirs.d[k][1];
    const unsigned long long lo = ranges[2 * b], hi = ranges[2 * b + 1];
    double best = -__builtin_inf(), bu = __builtin_nan(""), bv = __builtin_nan("");
    unsigned long long bkey = kEmpty;
    for (unsigned long long i = lo + w; i < hi; i += kWaves) {
        const unsigned long long* mrec = members + i * kPlMemberWords;
        const double u = __longlong_as_double((long long)mrec[0]), v = __longlong_as_double((long long)mrec[1]);
        const unsigned long long key = mrec[2];
        const double pr = u * A + v * B;
        if (pr > best || (pr == best && key < bkey)) {
            best = pr;
            bkey = key;
            bu = u;
            bv = v;
        }
    }
    s_pr[w][k] = best;
    s_key[w][k] = bkey;
    s_u[w][k] = bu;
    s_v[w][k] = bv;
    __syncthreads();
    if (w != 0) return;
    for (int q = 1; q < kWaves; ++q) {
        const double pr = s_pr[q][k];
        const unsigned long long key = s_key[q][k];
        if (pr > best || (pr == best && key < bkey)) {
            best = pr;
            bkey = key;
            bu = s_u[q][k];
            bv = s_v[q][k];
        }
    }
    unsigned long long* o = out + ((size_t)b * 64 + k) * kPlMemberWords;
    o[0] = (unsigned long long)__double_as_longlong(bu);
    o[1] = (unsigned long long)__double_as_longlong(bv);
    o[2] = bkey;
}

// the label read-out: any output may be null; records beyond max_out are counted, not written.  plane_of may be null where no region qualifies.
__global__ __launch_bounds__(256) void k_vmap_pl_labels(const unsigned long long* __restrict__ table, unsigned long long n_slots, PlLayer L,
                                                        const int* __restrict__ plane_of, long long max_out, unsigned long long* __restrict__ counter,
                                                        int32_t* __restrict__ key3, int32_t* __restrict__ label_key3, int32_t* __restrict__ plane_index) {
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long at = s < n_slots ? s : 0;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(table + at * kFields);
    const bool occupied = s < n_slots && kc.x != kEmpty && kc.y != 0;
    const unsigned long long wave = __ballot(occupied);
    unsigned long long base = 0;
    if (lane == 0 && wave) base = atomicAdd(counter, (unsigned long long)__popcll(wave));      // one add per wave
    base = __shfl(base, 0);
    const unsigned long long o = base + (unsigned long long)__popcll(wave & ((1ull << lane) - 1ull));
    if (!occupied || (long long)o >= max_out) return;
    const int r = L.parent[at];
    const int id = r >= 0 ? L.rid[r] : -1;
    if (key3) unpack_key3(kc.x, key3 + 3 * o);
    if (label_key3) unpack_key3(r >= 0 ? L.rmin[r] : kc.x, label_key3 + 3 * o);
    if (plane_index) plane_index[o] = id >= 0 && plane_of ? plane_of[id] : -1;
}

}  // namespace vmap

namespace {

static_assert(sizeof(rgbd360_map_plane_seg_params) == 32, "eight 4-byte parameters");
static_assert(sizeof(rgbd360_map_plane_seg_stats) == 6 * sizeof(long long), "six counters");
static_assert(sizeof(RGBD360_MAP_PLANE_DIRS) == sizeof(vmap::PlDirs), "the header's direction table is the kernel's");

// what every entry that takes segmentation parameters checks before anything is launched
int planes_check_params(rgbd360_map* m, const rgbd360_map_plane_seg_params* params, rgbd360_map_plane_seg_params& p) {
    if (params) p = *params;
    else rgbd360_map_default_plane_seg_params(m, &p);
    if (p.min_count < 1) return vmap_fail(m, -1, "min_count must be at least 1");
    if (p.min_support < 1 || p.min_support > 27) return vmap_fail(m, -1, "min_support must lie in 1 .. 27");
    if (!(p.max_flatness >= 0.f)) return vmap_fail(m, -1, "max_flatness must not be negative");
    if (!(p.max_voxel_curvature >= 0.f)) return vmap_fail(m, -1, "max_voxel_curvature must not be negative");
    if (!(p.cos_angle >= 0.f && p.cos_angle <= 1.f)) return vmap_fail(m, -1, "cos_angle must lie in 0 .. 1");
    if (!(p.max_offset >= 0.f)) return vmap_fail(m, -1, "max_offset must not be negative");
    if (p.min_voxels < 1) return vmap_fail(m, -1, "min_voxels must be at least 1");
    if (!(p.max_curvature >= 0.f)) return vmap_fail(m, -1, "max_curvature must not be negative");
    return 0;
}

// the range rule of a region's sums (the header): decided from N and the extent, before any sum is read
bool planes_sums_in_range(long long n_voxels, long long extent_cells, float leaf) {
    const double b = ((double)extent_cells + 2.0) * (double)leaf * vmap::kPlFix;
    return (double)n_voxels * (b * b) < 0x1p62;
}

// A region's fit from its sums (float64): the Frame360 regions' fit on the moments in metres about the root's centroid
struct MapPlaneFit {
    RegionFit f;
    double c[3], curvature;
};
MapPlaneFit planes_fit_sums(long long n_voxels, const float root_centroid[3], const long long sums[9]) {
    MapPlaneFit F;
    double mo[9];
    for (int q = 0; q < 3; ++q) mo[q] = (double)sums[q] / vmap::kPlFix;
    for (int q = 3; q < 9; ++q) mo[q] = (double)sums[q] / (vmap::kPlFix * vmap::kPlFix);
    F.f = region_fit_moments(mo, (double)n_voxels);
    for (int k = 0; k < 3; ++k) F.c[k] = (double)root_centroid[k] + F.f.c[k];
    const double tr = F.f.C[0][0] + F.f.C[1][1] + F.f.C[2][2];
    F.curvature = tr != 0 ? fabs(F.f.evals[0] / tr) : 0;
    return F;
}
// ... into a plane record without hull and colour, the normal facing `viewpoint` (null: the origin)
void planes_fill_record(const MapPlaneFit& F, long long n_points, const float* viewpoint, rgbd360_plane& P) {
    memset(&P, 0, sizeof(P));
    double v[3] = {F.f.evecs[0][0], F.f.evecs[0][1], F.f.evecs[0][2]};
    double e[3];
    for (int k = 0; k < 3; ++k) e[k] = (viewpoint ? (double)viewpoint[k] : 0.0) - F.c[k];
    if (e[0] * v[0] + e[1] * v[1] + e[2] * v[2] < 0) {
        for (int k = 0; k < 3; ++k) v[k] = -v[k];
    }
    for (int k = 0; k < 3; ++k) {
        P.centroid[k] = (float)F.c[k];
        P.normal[k] = (float)v[k];
        P.center_hull[k] = P.centroid[k];
    }
    P.d = (float)-(v[0] * F.c[0] + v[1] * F.c[1] + v[2] * F.c[2]);
    P.curvature = (float)F.curvature;
    apply_extent(P, F.f, (int)std::min<long long>(n_points, 2147483647ll));
    P.area = P.area_moment;
}

// the in-plane frame of a region's hull: the record's float32 centroid and the two in-plane eigenvectors in float32; no extremes yet
void planes_frame(const MapPlaneFit& F, VmapPlaneRec& R) {
    for (int k = 0; k < 3; ++k) {
        R.origin[k] = (float)F.c[k];
        R.e1[k] = (float)F.f.evecs[1][k];
        R.e2[k] = (float)F.f.evecs[2][k];
    }
    for (int k = 0; k < 64; ++k) R.uv[k][0] = R.uv[k][1] = NAN;
}
// The extremes of a member list on the host, operation for operation what k_vmap_pl_scatter and k_vmap_pl_extremes compute
// (rgbd360_map_plane_from_members: the record a test can build without a device)
void planes_host_extremes(VmapPlaneRec& R, const float* xyz, const int32_t* key3, long long n) {
#pragma clang fp contract(off)
    double best[64];
    unsigned long long bkey[64];
    for (int k = 0; k < 64; ++k) best[k] = -INFINITY, bkey[k] = vmap::kEmpty;
    for (long long i = 0; i < n; ++i) {
        const float* c = xyz + 3 * i;
        const unsigned long long key = vmap::pack_key((unsigned long long)(key3[3 * i] + vmap::kBias), (unsigned long long)(key3[3 * i + 1] + vmap::kBias),
                                                      (unsigned long long)(key3[3 * i + 2] + vmap::kBias));
        const double d0 = (double)c[0] - (double)R.origin[0], d1 = (double)c[1] - (double)R.origin[1], d2 = (double)c[2] - (double)R.origin[2];
        const double u = (d0 * (double)R.e1[0] + d1 * (double)R.e1[1]) + d2 * (double)R.e1[2];
        const double v = (d0 * (double)R.e2[0] + d1 * (double)R.e2[1]) + d2 * (double)R.e2[2];
        for (int k = 0; k < 64; ++k) {
            const double pr = u * (double)RGBD360_MAP_PLANE_DIRS[k][0] + v * (double)RGBD360_MAP_PLANE_DIRS[k][1];
            if (pr > best[k] || (pr == best[k] && key < bkey[k])) {
                best[k] = pr;
                bkey[k] = key;
                R.uv[k][0] = (float)u;
                R.uv[k][1] = (float)v;
            }
        }
    }
}

vmap::PlLayer planes_layer_view(const rgbd360_map* m) {
    unsigned long long* w = m->pl_layer.get();
    const size_t n = (size_t)m->n_slots;
    int* i = reinterpret_cast<int*>(w + 2 * n);
    return {w, w + n, i, reinterpret_cast<unsigned*>(i + n), reinterpret_cast<unsigned*>(i + 2 * n), i + 3 * n};
}
void planes_fill_stats(const rgbd360_map_plane_seg_stats* from, rgbd360_map_plane_seg_stats* st) {
    if (!st) return;
    if (from) *st = *from;
    else memset(st, 0, sizeof(*st));
}

// The segmentation of the map as it stands under `p`: reused while the revision word and the parameters are those it was built with,
// else rebuilt; complete when the call returns (the host stands between the passes: it sorts the roots, applies the range rule, fits the
// planes and hands the frames back).  n_voxels > 0.  tm / us: the stages under the timer (rgbd360_map_time_planes).
int planes_build(rgbd360_map* m, const rgbd360_map_plane_seg_params& p, VmapTimer* tm = nullptr, float* us = nullptr) {
    hipSetDevice(m->s->p.device);
    if (m->pl_rev == m->revision && memcmp(&m->pl_params, &p, sizeof(p)) == 0) return 0;
    rgbd360_map_normal_params np;
    np.min_count = p.min_count, np.min_support = p.min_support, np.max_flatness = p.max_flatness, np.max_shift = 0.f;
    if (const int rc = normals_layer(m, np)) return rc;
    hipStream_t stream = m->s->stream;
    m->pl_rev = 0;
    m->pl_planes.clear();
    const size_t n = (size_t)m->n_slots;
    const unsigned long long cap = (unsigned long long)(m->n_voxels / p.min_voxels) + 1;      // a qualifying region holds min_voxels voxels
    HIPC(m, m->pl_layer.ensure(4 * n));
    HIPC(m, m->pl_roots.ensure((size_t)cap * vmap::kPlRootWords));
    HIPC(m, m->pl_stats.ensure(vmap::kPlWords));
    HIPC(m, m->pl_hstats.ensure(vmap::kPlWords));
    const vmap::PlLayer L = planes_layer_view(m);
    const unsigned long long* table = m->table.get();
    const dim3 grid((unsigned)((n + vmap::kPlThreads - 1) / vmap::kPlThreads)), block(vmap::kPlThreads);
    auto stage = [&](int k, auto&& body) -> int {
        if (!tm) return body();
        tm->timed(us[k], 1, body);
        return tm->rc;
    };
    HIPC(m, hipMemsetAsync(m->pl_stats, 0, vmap::kPlWords * sizeof(unsigned long long), stream));
    if (const int rc = stage(0, [&] {
            hipLaunchKernelGGL(vmap::k_vmap_pl_init, grid, block, 0, stream, m->n_slots, L);
            return 0;
        }))
        return rc;
    if (const int rc = stage(1, [&] {
            hipLaunchKernelGGL(vmap::k_vmap_pl_link, grid, block, 0, stream, table, m->n_slots, (const uint4*)m->nm_layer.get(), p.max_voxel_curvature,
                               (double)p.cos_angle, (double)p.max_offset * (double)m->leaf, L.parent, m->pl_stats.get());
            return 0;
        }))
        return rc;
    if (const int rc = stage(2, [&] {
            hipLaunchKernelGGL(vmap::k_vmap_pl_compress, grid, block, 0, stream, table, m->n_slots, (const uint4*)m->nm_layer.get(), p.max_voxel_curvature, L);
            return 0;
        }))
        return rc;
    if (const int rc = stage(3, [&] {
            hipLaunchKernelGGL(vmap::k_vmap_pl_count, grid, block, 0, stream, table, m->n_slots, L);
            return 0;
        }))
        return rc;
    if (const int rc = stage(4, [&] {
            hipLaunchKernelGGL(vmap::k_vmap_pl_roots, grid, block, 0, stream, table, m->n_slots, L, (unsigned)p.min_voxels, cap, m->pl_roots.get(),
                               m->pl_stats.get());
            return 0;
        }))
        return rc;
    HIPC(m, hipGetLastError());
    HIPC(m, hipMemcpyAsync(m->pl_hstats, m->pl_stats, vmap::kPlWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPC(m, hipStreamSynchronize(stream));
    rgbd360_map_plane_seg_stats st = {};
    st.n_voxels = (long long)m->pl_hstats[vmap::kPlVoxels];
    st.n_eligible = (long long)m->pl_hstats[vmap::kPlEligible];
    st.n_links = (long long)m->pl_hstats[vmap::kPlLinks];
    st.n_regions = (long long)m->pl_hstats[vmap::kPlRegions];
    const size_t nq = (size_t)std::min<unsigned long long>(m->pl_hstats[vmap::kPlQualify], cap);
    std::vector<unsigned long long> roots(nq * vmap::kPlRootWords), sums(nq * 9);
    if (nq) HIPC(m, hipMemcpy(roots.data(), m->pl_roots, roots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    // the range rule, from N and the extent, before any sum exists
    for (size_t id = 0; id < nq; ++id) {
        const unsigned long long w1 = roots[id * vmap::kPlRootWords + 1];
        if (!planes_sums_in_range((long long)(w1 & 0xffffffffull), (long long)(w1 >> 32), m->leaf))
            return vmap_fail(m, -8, "region sums out of range (N ((E + 2) leaf 2^16)^2 >= 2^62)");
    }
    std::vector<int> plane_of(nq, -1);
    if (nq) {
        HIPC(m, m->pl_sums.ensure(9 * nq));
        HIPC(m, m->pl_plane_of.ensure(nq));
        HIPC(m, hipMemsetAsync(m->pl_sums, 0, 9 * nq * sizeof(unsigned long long), stream));
        const int merge = m->pl_merge_waves ? 1 : 0;
        if (const int rc = stage(5, [&] {
                hipLaunchKernelGGL(vmap::k_vmap_pl_sums, grid, block, 0, stream, table, m->n_slots, L, (const unsigned long long*)m->pl_roots.get(),
                                   m->pl_sums.get(), merge);
                return 0;
            }))
            return rc;
        HIPC(m, hipGetLastError());
        HIPC(m, hipMemcpyAsync(sums.data(), m->pl_sums, sums.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIPC(m, hipStreamSynchronize(stream));
        // the regions by root key; those flat enough are the planes
        std::vector<size_t> order(nq);
        for (size_t k = 0; k < nq; ++k) order[k] = k;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return roots[a * vmap::kPlRootWords] < roots[b * vmap::kPlRootWords]; });
        for (const size_t id : order) {
            const unsigned long long* w = &roots[id * vmap::kPlRootWords];
            VmapPlaneRec R = {};
            R.root_key = w[0];
            R.n_voxels = (long long)(w[1] & 0xffffffffull);
            R.n_points = (long long)w[2];
            const unsigned cb[3] = {(unsigned)w[3], (unsigned)(w[3] >> 32), (unsigned)w[4]};
            memcpy(R.root_centroid, cb, sizeof(cb));
            for (int q = 0; q < 9; ++q) R.sums[q] = (long long)sums[id * 9 + q];
            const MapPlaneFit F = planes_fit_sums(R.n_voxels, R.root_centroid, R.sums);
            if (!(F.curvature <= (double)p.max_curvature)) continue;
            planes_frame(F, R);
            plane_of[id] = (int)m->pl_planes.size();
            m->pl_planes.push_back(R);
            st.n_voxels_in_planes += R.n_voxels;
        }
        HIPC(m, hipMemcpyAsync(m->pl_plane_of, plane_of.data(), nq * sizeof(int), hipMemcpyHostToDevice, stream));
    }
    const size_t na = m->pl_planes.size();
    st.n_planes_available = (long long)na;
    if (na) {
        // the extremes: the planes' frames and the starts of their member lists go up, the members are scattered, a workgroup per plane reduces
        std::vector<float> frames(na * vmap::kPlFrameFloats, 0.f);
        std::vector<unsigned long long> offset(na + 1, 0);
        for (size_t a = 0; a < na; ++a) {
            const VmapPlaneRec& R = m->pl_planes[a];
            float* F = &frames[a * vmap::kPlFrameFloats];
            for (int k = 0; k < 3; ++k) F[k] = R.origin[k], F[3 + k] = R.e1[k], F[6 + k] = R.e2[k];
            offset[a + 1] = offset[a] + (unsigned long long)R.n_voxels;
        }
        HIPC(m, m->pl_frames.ensure(frames.size()));
        HIPC(m, m->pl_offset.ensure(na + 1));
        HIPC(m, m->pl_cursor.ensure(na));
        HIPC(m, m->pl_members.ensure((size_t)offset[na] * vmap::kPlMemberWords));
        // the extremes in two levels: the lists cut into chunks of kPlChunk members, then the chunks' winners of a plane
        std::vector<unsigned long long> ranges;
        std::vector<size_t> first_chunk(na + 1, 0);
        for (size_t a = 0; a < na; ++a) {
            for (unsigned long long lo = offset[a]; lo < offset[a + 1]; lo += vmap::kPlChunk) {
                ranges.push_back(lo);
                ranges.push_back(std::min(lo + vmap::kPlChunk, offset[a + 1]));
            }
            first_chunk[a + 1] = ranges.size() / 2;
        }
        const size_t n_chunks = ranges.size() / 2;
        for (size_t a = 0; a < na; ++a) {       // (behind the chunks' ranges: the planes' ranges over the winners)
            ranges.push_back(64ull * first_chunk[a]);
            ranges.push_back(64ull * first_chunk[a + 1]);
        }
        HIPC(m, m->pl_ranges.ensure(ranges.size()));
        HIPC(m, m->pl_partial.ensure(n_chunks * 64 * vmap::kPlMemberWords));
        HIPC(m, m->pl_extremes.ensure(na * 64 * vmap::kPlMemberWords));
        HIPC(m, hipMemcpyAsync(m->pl_ranges, ranges.data(), ranges.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
        HIPC(m, hipMemcpyAsync(m->pl_frames, frames.data(), frames.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        HIPC(m, hipMemcpyAsync(m->pl_offset, offset.data(), (na + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
        HIPC(m, hipMemsetAsync(m->pl_cursor, 0, na * sizeof(int), stream));
        if (const int rc = stage(6, [&] {
                hipLaunchKernelGGL(vmap::k_vmap_pl_scatter, grid, block, 0, stream, table, m->n_slots, L, (const int*)m->pl_plane_of.get(),
                                   (const float*)m->pl_frames.get(), (const unsigned long long*)m->pl_offset.get(), m->pl_cursor.get(), m->pl_members.get());
                return 0;
            }))
            return rc;
        vmap::PlDirs dirs;
        memcpy(&dirs, RGBD360_MAP_PLANE_DIRS, sizeof(dirs));
        if (const int rc = stage(7, [&] {
                hipLaunchKernelGGL(vmap::k_vmap_pl_extremes, dim3((unsigned)n_chunks), dim3(vmap::kPlExtThreads), 0, stream,
                                   (const unsigned long long*)m->pl_members.get(), (const unsigned long long*)m->pl_ranges.get(), m->pl_partial.get(), dirs);
                hipLaunchKernelGGL(vmap::k_vmap_pl_extremes, dim3((unsigned)na), dim3(vmap::kPlExtThreads), 0, stream,
                                   (const unsigned long long*)m->pl_partial.get(), (const unsigned long long*)m->pl_ranges.get() + 2 * n_chunks,
                                   m->pl_extremes.get(), dirs);
                return 0;
            }))
            return rc;
        HIPC(m, hipGetLastError());
        std::vector<unsigned long long> ext(na * 64 * vmap::kPlMemberWords);
        HIPC(m, hipMemcpyAsync(ext.data(), m->pl_extremes, ext.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIPC(m, hipStreamSynchronize(stream));       // (the uploads above left pageable memory: they are through as well)
        for (size_t a = 0; a < na; ++a)
            for (int k = 0; k < 64; ++k)
                for (int q = 0; q < 2; ++q) {
                    double w;
                    memcpy(&w, &ext[(a * 64 + k) * vmap::kPlMemberWords + q], sizeof(w));
                    m->pl_planes[a].uv[k][q] = (float)w;
                }
    } else {
        HIPC(m, hipStreamSynchronize(stream));
    }
    m->pl_host_stats = st;
    m->pl_params = p;
    m->pl_rev = m->revision;
    return 0;
}

// plane `a` of the cached list as a record: the fit from its sums, the normal towards the viewpoint, the hull of its extremes
void planes_record(const VmapPlaneRec& R, const float* viewpoint, rgbd360_plane& P) {
    planes_fill_record(planes_fit_sums(R.n_voxels, R.root_centroid, R.sums), R.n_points, viewpoint, P);
    f360::F360HullRecord H;
    for (int k = 0; k < 3; ++k) H.c[k] = R.origin[k], H.e1[k] = R.e1[k], H.e2[k] = R.e2[k];
    H.n = 64;
    memcpy(H.uv, R.uv, sizeof(R.uv));
    apply_hull(P, H);
}

}  // namespace

extern "C" void rgbd360_map_default_plane_seg_params(const rgbd360_map* m, rgbd360_map_plane_seg_params* p) {
    if (!p) return;
    (void)m;
    p->min_count = 1;              // the three of rgbd360_map_default_normal_params
    p->min_support = 5;
    p->max_flatness = 0.05f;
    p->max_voxel_curvature = INFINITY;
    p->cos_angle = 0.9961947f;     // cos 5 deg
    p->max_offset = 0.5f;
    p->min_voxels = 50;
    p->max_curvature = 0.0013f;
}

extern "C" int rgbd360_map_planes(rgbd360_map* m, const rgbd360_map_plane_seg_params* params, const float* viewpoint, int max_planes,
                                  rgbd360_plane* planes_out, int32_t* root_key3_out, int* n_planes_out, rgbd360_map_plane_seg_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_plane_seg_params p;
    if (const int rc = planes_check_params(m, params, p)) return rc;
    if (max_planes < 0) return vmap_fail(m, -1, "max_planes must not be negative");
    for (int k = 0; k < 3 && viewpoint; ++k)
        if (!std::isfinite(viewpoint[k])) return vmap_fail(m, -1, "the viewpoint must be finite");
    if (m->n_voxels == 0) {
        planes_fill_stats(nullptr, stats);
        if (n_planes_out) *n_planes_out = 0;
        return 0;
    }
    if (const int rc = planes_build(m, p)) return rc;
    const size_t na = m->pl_planes.size();
    std::vector<size_t> keep(na);
    for (size_t a = 0; a < na; ++a) keep[a] = a;
    if (na > (size_t)max_planes) {      // the largest N, ties to the smaller root key; then root-key order again
        std::sort(keep.begin(), keep.end(), [&](size_t a, size_t b) {
            const VmapPlaneRec &A = m->pl_planes[a], &B = m->pl_planes[b];
            return A.n_voxels != B.n_voxels ? A.n_voxels > B.n_voxels : A.root_key < B.root_key;
        });
        keep.resize((size_t)max_planes);
        std::sort(keep.begin(), keep.end());
    }
    for (size_t o = 0; o < keep.size(); ++o) {
        const VmapPlaneRec& R = m->pl_planes[keep[o]];
        if (planes_out) {
            planes_record(R, viewpoint, planes_out[o]);
            planes_out[o].root = (int)o;
        }
        if (root_key3_out) vmap::unpack_key3(R.root_key, root_key3_out + 3 * o);
    }
    if (n_planes_out) *n_planes_out = (int)keep.size();
    planes_fill_stats(&m->pl_host_stats, stats);
    return 0;
}

extern "C" long long rgbd360_map_plane_labels(rgbd360_map* m, const rgbd360_map_plane_seg_params* params, long long max_out, int32_t* key3,
                                              int32_t* label_key3, int32_t* plane_index) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_plane_seg_params p;
    if (const int rc = planes_check_params(m, params, p)) return rc;
    if (max_out < 0) return vmap_fail(m, -1, "max_out must not be negative");
    if (m->n_voxels == 0) return 0;
    if (const int rc = planes_build(m, p)) return rc;
    const size_t n = std::min((size_t)m->n_voxels, (size_t)max_out);
    if (n == 0 || (!key3 && !label_key3 && !plane_index)) return m->n_voxels;
    hipStream_t stream = m->s->stream;
    // the records staged on the device, seven words each: key3, label_key3, plane_index
    HIPC(m, m->pl_stage.ensure(7 * n));
    int32_t* sg = m->pl_stage.get();
    unsigned long long* counter = m->pl_stats + vmap::kPlLabels;
    HIPC(m, hipMemsetAsync(counter, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(vmap::k_vmap_pl_labels, dim3((unsigned)((m->n_slots + 255) / 256)), dim3(256), 0, stream, (const unsigned long long*)m->table.get(),
                       m->n_slots, planes_layer_view(m), (const int*)m->pl_plane_of.get(), (long long)n, counter, key3 ? sg : nullptr, label_key3 ? sg + 3 * n : nullptr, plane_index ? sg + 6 * n : nullptr);
    HIPC(m, hipGetLastError());
    if (key3) HIPC(m, hipMemcpyAsync(key3, sg, 3 * n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (label_key3) HIPC(m, hipMemcpyAsync(label_key3, sg + 3 * n, 3 * n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (plane_index) HIPC(m, hipMemcpyAsync(plane_index, sg + 6 * n, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIPC(m, hipStreamSynchronize(stream));
    return m->n_voxels;
}

extern "C" size_t rgbd360_map_plane_bytes(const rgbd360_map* m) {
    if (!m) return 0;
    return (m->pl_layer.capacity() + m->pl_roots.capacity() + m->pl_sums.capacity() + m->pl_stats.capacity() + m->pl_offset.capacity() +
            m->pl_members.capacity() + m->pl_ranges.capacity() + m->pl_partial.capacity() + m->pl_extremes.capacity()) * sizeof(unsigned long long) +
           (m->pl_plane_of.capacity() + m->pl_cursor.capacity() + m->pl_stage.capacity()) * sizeof(int) +
           m->pl_frames.capacity() * sizeof(float);
}

extern "C" int rgbd360_map_release_planes(rgbd360_map* m) {
    if (!m) return -1;
    m->err.clear();
    hipSetDevice(m->s->p.device);
    HIPC(m, hipStreamSynchronize(m->s->stream));
    m->pl_layer.release(), m->pl_roots.release(), m->pl_sums.release(), m->pl_stats.release(), m->pl_offset.release(), m->pl_members.release();
    m->pl_plane_of.release(), m->pl_cursor.release(), m->pl_stage.release(), m->pl_frames.release(), m->pl_extremes.release(), m->pl_ranges.release(), m->pl_partial.release();
    m->pl_planes.clear();
    m->pl_rev = 0;
    return 0;
}

// host only (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_plane_from_sums(long long n_voxels, long long n_points, const float root_centroid[3], const long long sums[9],
                                           const float viewpoint[3], rgbd360_plane* plane) {
    if (!root_centroid || !sums || !plane || n_voxels < 1) return -1;
    planes_fill_record(planes_fit_sums(n_voxels, root_centroid, sums), n_points, viewpoint, *plane);
    return 0;
}
extern "C" int rgbd360_map_plane_from_members(long long n_voxels, long long n_points, const float root_centroid[3], const long long sums[9],
                                              const float* member_xyz, const int32_t* member_key3, const float viewpoint[3], rgbd360_plane* plane) {
    if (!root_centroid || !sums || !plane || !member_xyz || !member_key3 || n_voxels < 1) return -1;
    VmapPlaneRec R = {};
    R.n_voxels = n_voxels, R.n_points = n_points;
    memcpy(R.root_centroid, root_centroid, sizeof(R.root_centroid));
    memcpy(R.sums, sums, sizeof(R.sums));
    planes_frame(planes_fit_sums(n_voxels, root_centroid, sums), R);
    planes_host_extremes(R, member_xyz, member_key3, n_voxels);
    planes_record(R, viewpoint, *plane);
    return 0;
}
extern "C" int rgbd360_map_plane_sums_in_range(long long n_voxels, long long extent_cells, float leaf) {
    return planes_sums_in_range(n_voxels, extent_cells, leaf) ? 1 : 0;
}

// measurement (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_time_planes(rgbd360_map* m, const rgbd360_map_plane_seg_params* params, int reps, int merge_waves, float* stage_us,
                                       rgbd360_map_plane_seg_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_plane_seg_params p;
    if (const int rc = planes_check_params(m, params, p)) return rc;
    if (reps < 1 || !stage_us || m->n_voxels == 0) return vmap_fail(m, -1, "bad arguments");
    m->pl_merge_waves = merge_waves != 0;
    m->pl_rev = 0;
    int rc = planes_build(m, p);      // once untimed: code and buffers there
    {
        VmapTimer timer(m, m->s->stream);
        if (rc == 0) rc = timer.rc;
        for (int r = 0; r < reps && rc == 0; ++r) {
            for (int k = 0; k < 8; ++k) stage_us[8 * r + k] = 0.f;
            m->pl_rev = 0;
            rc = planes_build(m, p, &timer, stage_us + 8 * r);
        }
    }
    m->pl_merge_waves = true;
    m->pl_rev = rc == 0 ? m->pl_rev : 0;
    if (rc) {
        (void)hipGetLastError();
        return rc;
    }
    planes_fill_stats(&m->pl_host_stats, stats);
    return 0;
}
