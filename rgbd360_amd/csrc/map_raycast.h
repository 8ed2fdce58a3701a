// map_raycast.h -- ray casting through the resident voxel map (voxel_map.h): the first occupied voxel along each ray of a list, or of every
// pixel of the dense alignment's full-sphere panorama at a pose.  Where map_render.h splats centroids into pixels, this walks the grid:
// the model image of frame-to-model alignment as a per-pixel first hit, any view as a list of rays, line-of-sight checks.
// Part of the Frame360 translation unit (rgbd360_frame360.hip includes it behind voxel_map.h, map_edit.h and map_normals.h).
// The surface cast (rgbd360_map_raycast_surface*) is the same kernel and the same host entries with SURFACE / a RaySurface: the traversal
// and the hit decision below unchanged, then per hit the normal of the voxel and the depth on its plane (vmap::surface_step, map_normals.h).
//
// Definition (include/rgbd360_hip.h, "ray casting through the map"; tests/map_raycast_reference.py restates it).  All
// traversal arithmetic is float64 + - x / with contraction off; o, d, the centroid and inv_leaf enter as the doubles of their float32 values.
//   1 ray         origin o, direction d (float32 triples, world); the point at t >= 0 is o + t d, t in units of |d|.  Not finite, or d = 0:
//                 status "bad ray", nothing traversed.
//   2 grid        g_k = o_k inv_leaf, u_k = d_k inv_leaf (both products exact), r_k = 1 / u_k; the time of the ray at the cell boundary b
//                 of axis k (the plane between cells b - 1 and b) is T_k(b) = (b - g_k) r_k: two roundings, a function of b alone -- no
//                 running sum, so the time of a boundary does not depend on how the ray came there.  u_k = 0: T_k = +inf.
//   3 clip        the box of the live voxels, cells lo_k .. hi_k (integer key bounds over the slots with count > 0): t0 = max(0, near_k),
//                 t1 = min(far_k) over the axes with u_k != 0, near / far the smaller / larger of T_k(lo_k), T_k(hi_k + 1); an axis with
//                 u_k = 0 misses unless lo_k <= g_k < hi_k + 1.  t0 > t1: status "misses the box", zero steps.
//   4 start       cell i_k = floor(g_k + t0 u_k) clamped to lo_k .. hi_k; t_in = t0.
//   5 per cell    t_in > t_max: status "t_max".  max_steps cells visited: status "max_steps".  Else the cell counts as a step;
//                 t_out = min_k T_k(next boundary of axis k), on equal times the LOWEST axis index.  Candidate: the slot of the cell is
//                 live with count >= min_count (tombstones and empty slots are air).  c = the read-out's centroid (vmap::centroid),
//                 s = (((c_x - o_x) d_x + (c_y - o_y) d_y) + (c_z - o_z) d_z) / ((d_x^2 + d_y^2) + d_z^2), t_hit = min(max(s, t_in), t_out).
//                 Rejected when t_hit < t_min, or when ((e_x^2 + e_y^2) + e_z^2) inv_leaf^2 > max_offset^2, e_k = (c_k - o_k) - s d_k.
//                 Else: status "hit".
//   6 advance     the axis of t_out steps by the sign of u_k; a cell outside lo .. hi: status "left the box" (the key range |i| < 2^20
//                 contains the box).  t_in = t_out.
//   7 outputs     t = (float)t_hit, key3, count, rgb3 (the read-out's integer division), status; zeros on a miss.  Exact integer counters.
//
// The coarse layer: bricks of 8^3 cells, a hash table brick key -> 512-bit mask of the live cells, and the live-key bounds, built by two
// scans of the voxel table (k_vmap_layer_keys claims the bricks the way the voxel table claims slots and takes the bounds with integer
// min / max atomics; the host reads the brick count and sizes the masks; k_vmap_layer_masks sets the bits with integer atomicOr).  Kernel
// boundaries are the only synchronisation.  The layer belongs to the map and is rebuilt only when the map's revision word has moved (the
// writing entries bump it on the host).  The layered traversal looks the brick up once per brick entered; in an absent brick it jumps to
// the cell behind the brick's exit face -- the first of the three exit-boundary times, lowest axis on ties, and on the other two axes
// every boundary whose (time, axis) sorts before it, which is exactly the order in which step 5 would have crossed them; the cells jumped
// over are counted as steps -- and in a present brick it probes the voxel table only where the bit is set.  Where a limit (t_max,
// max_steps) could fall inside the jump it walks the cells instead.  Outputs and counters are those of the plain traversal, bit for
// bit, except n_lookups (voxel-table lookups: every cell for the plain form, live cells only for the layered one).
//
// One lane per ray; a wave runs until its longest ray ends.  cast_ray is host-device and takes the tables through a Grid, so that the
// same text can be run against a host-side map.  What happens at a candidate is a compile-time policy: FirstHit, the ray cast (the
// candidate that passes ends the ray), or one that is handed every candidate and lets the walk go on (map_carve.h: the line of sight
// of a measurement).  The first-hit instantiation is the code it was before the policy (same registers, no scratch: DESIGN.md 3.22).
#pragma once
#include <limits>

#include "map_table.h"

namespace vmap {

constexpr int kRayThreads = 256;
enum { kRayMissBox, kRayHit, kRayLeftBox, kRayTMax, kRayMaxSteps, kRayBad };      // the status of a ray (rgbd360_hip.h: RGBD360_RAY_*)
enum { kRsRays, kRsHits, kRsMissBox, kRsLeftBox, kRsTMax, kRsMaxSteps, kRsBad, kRsSteps, kRsLookups, kRsWords };      // rgbd360_map_raycast_stats in its order
enum { kLyLo = 0, kLyHi = 3, kLyBricks = 6, kLyWords = 8 };      // the layer's scan words (uint32): biased min, biased max, bricks claimed

// the brick of a cell (unbiased indices): the three 18-bit brick indices packed like a key
__host__ __device__ inline unsigned long long brick_key(int ix, int iy, int iz) {
    return ((unsigned long long)((iz + kBias) >> 3) << 36) | ((unsigned long long)((iy + kBias) >> 3) << 18) | (unsigned long long)((ix + kBias) >> 3);
}

struct RayParams {
    unsigned long long min_count;
    double t_min, t_max, off2_max;       // off2_max = max_offset^2
    long long max_steps;
    float inv_leaf;
    int lo[3], hi[3];                    // the live box, unbiased cell indices
};
struct RayResult {
    int status;
    double t;
    int cell[3];
    const unsigned long long* rec;       // the slot of the hit
    long long steps, lookups;
};

// What a traversal does with a candidate (a live cell of count >= min_count, step 5).  FirstHit: the ray cast -- the candidate that passes
// t_min and max_offset ends the ray.  A policy with kStops = false (map_carve.h: the through-votes of a line of sight) is handed every
// candidate -- its slot, t_hit, |d|^2 and the squared offset in leaves -- and the walk goes on to t_max, the box or max_steps.
struct FirstHit {
    static constexpr bool kStops = true;
    __host__ __device__ void cell(const unsigned long long*, double, double, double) {}
};

// Steps 1-7 for one ray.  Grid: voxel(key) -> the slot's eight words or null; brick(brick key) -> the brick's eight mask words or null.
// (No array is indexed by a run-time axis: the selects keep i, T in registers.)
template <bool LAYER, class Grid, class Policy>
__host__ __device__ inline void cast_ray(const Grid& G, const RayParams& P, const float o[3], const float d[3], RayResult& H, Policy& policy) {
#pragma clang fp contract(off)
    const double kInf = __builtin_inf();
    H.status = kRayBad;
    H.t = 0.0;
    H.cell[0] = H.cell[1] = H.cell[2] = 0;
    H.rec = nullptr;
    H.steps = H.lookups = 0;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) finite = finite && __builtin_isfinite(o[k]) && __builtin_isfinite(d[k]);
    if (!finite || (d[0] == 0.f && d[1] == 0.f && d[2] == 0.f)) return;
    const double inv = (double)P.inv_leaf;
    double g[3], u[3], r[3];
    int st[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g[k] = (double)o[k] * inv;
        u[k] = (double)d[k] * inv;
        st[k] = u[k] > 0.0 ? 1 : u[k] < 0.0 ? -1 : 0;
        r[k] = st[k] ? 1.0 / u[k] : 0.0;
    }
    // 3 clip
    double t0 = 0.0, t1 = kInf;
    bool meets = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lo = (double)P.lo[k], hi1 = (double)(P.hi[k] + 1);
        if (st[k] == 0) {
            if (g[k] < lo || g[k] >= hi1) meets = false;
        } else {
            const double ta = (lo - g[k]) * r[k], tc = (hi1 - g[k]) * r[k];
            const double nr = ta < tc ? ta : tc, fr = ta < tc ? tc : ta;
            if (nr > t0) t0 = nr;
            if (fr < t1) t1 = fr;
        }
    }
    if (!meets || t0 > t1) {
        H.status = kRayMissBox;
        return;
    }
    // 4 start
    int i[3];
    double T[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double p = __builtin_floor(g[k] + t0 * u[k]);
        p = p < (double)P.lo[k] ? (double)P.lo[k] : p;
        p = p > (double)P.hi[k] ? (double)P.hi[k] : p;
        i[k] = (int)p;
        T[k] = st[k] ? ((double)(i[k] + (st[k] > 0 ? 1 : 0)) - g[k]) * r[k] : kInf;
    }
    const double dd = ((double)d[0] * (double)d[0] + (double)d[1] * (double)d[1]) + (double)d[2] * (double)d[2];
    double t_in = t0;
    long long steps = 0, lookups = 0;
    unsigned long long cur_brick = kEmpty;
    const unsigned long long* bm = nullptr;
    int status;
    for (;;) {
        if (t_in > P.t_max) {
            status = kRayTMax;
            break;
        }
        if (steps >= P.max_steps) {
            status = kRayMaxSteps;
            break;
        }
        ++steps;
        int a = T[1] < T[0] ? 1 : 0;
        if (T[2] < (a ? T[1] : T[0])) a = 2;
        const double t_out = a == 0 ? T[0] : a == 1 ? T[1] : T[2];
        bool probe = true;
        if (LAYER) {
            const unsigned long long bk = brick_key(i[0], i[1], i[2]);
            if (bk != cur_brick) {
                cur_brick = bk;
                bm = G.brick(bk);
            }
            if (bm) {
                probe = (bm[(i[2] + kBias) & 7] >> ((((i[1] + kBias) & 7) << 3) | ((i[0] + kBias) & 7))) & 1ull;
            } else {
                probe = false;
                // the exit of (brick intersected with box): per axis the boundary that leaves it and its time
                int B[3];
                double TB[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int c0 = (((i[k] + kBias) >> 3) << 3) - kBias;
                    const int up = c0 + 8 < P.hi[k] + 1 ? c0 + 8 : P.hi[k] + 1, dn = c0 > P.lo[k] ? c0 : P.lo[k];
                    B[k] = st[k] > 0 ? up : dn;
                    TB[k] = st[k] ? ((double)B[k] - g[k]) * r[k] : kInf;
                }
                int e = TB[1] < TB[0] ? 1 : 0;
                if (TB[2] < (e ? TB[1] : TB[0])) e = 2;
                const double tE = e == 0 ? TB[0] : e == 1 ? TB[1] : TB[2];
                int ni[3];
                long long crossed = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    int n = i[k];
                    if (k == e) {
                        n = st[k] > 0 ? B[k] : B[k] - 1;
                    } else if (st[k]) {
                        const int last = st[k] > 0 ? B[k] - 1 : B[k];
                        while (n != last) {      // (at most seven boundaries)
                            const double tt = ((double)(n + (st[k] > 0 ? 1 : 0)) - g[k]) * r[k];
                            if (!(tt < tE || (tt == tE && k < e))) break;
                            n += st[k];
                        }
                    }
                    ni[k] = n;
                    crossed += n > i[k] ? n - i[k] : i[k] - n;
                }
                if (tE <= P.t_max && steps + crossed <= P.max_steps) {      // no limit falls inside the jump
                    steps += crossed - 1;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        i[k] = ni[k];
                        T[k] = st[k] ? ((double)(i[k] + (st[k] > 0 ? 1 : 0)) - g[k]) * r[k] : kInf;
                    }
                    const int ie = e == 0 ? i[0] : e == 1 ? i[1] : i[2], le = e == 0 ? P.lo[0] : e == 1 ? P.lo[1] : P.lo[2],
                              he = e == 0 ? P.hi[0] : e == 1 ? P.hi[1] : P.hi[2];
                    if (ie < le || ie > he) {
                        status = kRayLeftBox;
                        break;
                    }
                    t_in = tE;
                    continue;
                }
            }
        }
        if (probe) {
            ++lookups;
            const unsigned long long* rec =
                G.voxel(pack_key((unsigned long long)(i[0] + kBias), (unsigned long long)(i[1] + kBias), (unsigned long long)(i[2] + kBias)));
            const unsigned long long cnt = rec ? rec[1] : 0;
            if (cnt != 0 && cnt >= P.min_count) {
                float c[3];
                centroid(rec, cnt, c);
                const double e0 = (double)c[0] - (double)o[0], e1 = (double)c[1] - (double)o[1], e2 = (double)c[2] - (double)o[2];
                const double s = ((e0 * (double)d[0] + e1 * (double)d[1]) + e2 * (double)d[2]) / dd;
                double th = s > t_in ? s : t_in;
                th = th < t_out ? th : t_out;
                if (!Policy::kStops) {
                    const double f0 = e0 - s * (double)d[0], f1 = e1 - s * (double)d[1], f2 = e2 - s * (double)d[2];
                    policy.cell(rec, th, dd, ((f0 * f0 + f1 * f1) + f2 * f2) * (inv * inv));
                } else if (th >= P.t_min) {
                    const double f0 = e0 - s * (double)d[0], f1 = e1 - s * (double)d[1], f2 = e2 - s * (double)d[2];
                    const double off2 = ((f0 * f0 + f1 * f1) + f2 * f2) * (inv * inv);
                    if (!(off2 > P.off2_max)) {
                        H.t = th;
                        H.rec = rec;
                        H.cell[0] = i[0], H.cell[1] = i[1], H.cell[2] = i[2];
                        status = kRayHit;
                        break;
                    }
                }
            }
        }
        // 6 advance
        bool out = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k == a) {
                i[k] += st[k];
                out = i[k] < P.lo[k] || i[k] > P.hi[k];
                T[k] = ((double)(i[k] + (st[k] > 0 ? 1 : 0)) - g[k]) * r[k];
            }
        }
        if (out) {
            status = kRayLeftBox;
            break;
        }
        t_in = t_out;
    }
    H.status = status;
    H.steps = steps;
    H.lookups = lookups;
}
template <bool LAYER, class Grid>
__host__ __device__ inline void cast_ray(const Grid& G, const RayParams& P, const float o[3], const float d[3], RayResult& H) {
    FirstHit first_hit;
    cast_ray<LAYER>(G, P, o, d, H, first_hit);
}

#if !defined(RGBD360_RAYCAST_CORE_ONLY)

// the two tables on the device
struct DevGrid {
    const unsigned long long* table;
    unsigned long long mask;
    const unsigned long long* bkeys;         // brick table: key per slot, ~0 = empty ...
    unsigned long long bmask;
    const uint32_t* bidx;                    // ... the brick's number ...
    const unsigned long long* masks;         // ... and per brick number eight words: word = z in the brick, bit = 8 y + x
    __device__ __forceinline__ const unsigned long long* voxel(unsigned long long key) const {
        const unsigned long long first = mix64(key) & mask;
        unsigned probes = 0;
        const long long slot = find(table, mask, key, first, table[first * kFields], probes);
        return slot < 0 ? nullptr : table + (unsigned long long)slot * kFields;
    }
    __device__ __forceinline__ const unsigned long long* brick(unsigned long long bk) const {
        unsigned long long slot = mix64(bk) & bmask;
        for (unsigned long long p = 0; p <= bmask; ++p) {      // (the table is at most half full: an empty slot ends every run)
            const unsigned long long k0 = bkeys[slot];
            if (k0 == bk) return masks + 8ull * bidx[slot];
            if (k0 == kEmpty) return nullptr;
            slot = (slot + 1) & bmask;
        }
        return nullptr;
    }
};

// the layer's first scan, one lane per slot: the live-key bounds (one min / max per wave and axis) and the bricks claimed and numbered
__global__ __launch_bounds__(256) void k_vmap_layer_keys(const unsigned long long* __restrict__ table, unsigned long long n_slots,
                                                         unsigned long long* __restrict__ bkeys, unsigned long long bmask, uint32_t* __restrict__ bidx,
                                                         unsigned* __restrict__ words) {
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(table + (s < n_slots ? s : 0) * kFields);
    const bool live = s < n_slots && kc.x != kEmpty && kc.y != 0;
    if (!__ballot(live)) return;
    unsigned lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned b = (unsigned)((kc.x >> (21 * k)) & 0x1fffffull);
        lo[k] = live ? b : 0xffffffffu;
        hi[k] = live ? b : 0u;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            lo[k] = min(lo[k], (unsigned)__shfl_xor((int)lo[k], off));
            hi[k] = max(hi[k], (unsigned)__shfl_xor((int)hi[k], off));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin(words + kLyLo + k, lo[k]);
            atomicMax(words + kLyHi + k, hi[k]);
        }
    }
    if (!live) return;
    int32_t c[3];
    unpack_key3(kc.x, c);
    const unsigned long long bk = brick_key(c[0], c[1], c[2]);
    unsigned long long slot = mix64(bk) & bmask;
    for (unsigned long long p = 0; p <= bmask; ++p) {
        unsigned long long k0 = __hip_atomic_load(bkeys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k0 == kEmpty) {
            k0 = atomicCAS(bkeys + slot, kEmpty, bk);
            if (k0 == kEmpty) {      // claimed: the brick's number (read by the next launch only)
                bidx[slot] = atomicAdd(words + kLyBricks, 1u);
                return;
            }
        }
        if (k0 == bk) return;
        slot = (slot + 1) & bmask;
    }
}
// ... and the second: every live slot sets its bit
__global__ __launch_bounds__(256) void k_vmap_layer_masks(const unsigned long long* __restrict__ table, unsigned long long n_slots, DevGrid G,
                                                          unsigned long long* __restrict__ masks) {
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_slots) return;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(table + s * kFields);
    if (kc.x == kEmpty || kc.y == 0) return;
    int32_t c[3];
    unpack_key3(kc.x, c);
    const unsigned long long* bm = G.brick(brick_key(c[0], c[1], c[2]));
    if (!bm) return;
    atomicOr(masks + (bm - G.masks) + ((c[2] + kBias) & 7), 1ull << ((((c[1] + kBias) & 7) << 3) | ((c[0] + kBias) & 7)));
}

struct RayJob {
    DevGrid G;
    RayParams P;
    long long n;
    const float *origins, *dirs;                         // a list of rays
    int cols;                                            // a panorama: pixel = row * cols + column ...
    const float *sin_theta, *cos_theta, *sin_phi, *cos_phi;      // ... its angle tables ...
    float pose[16];                                      // ... and the pose, column-major
    float* t;                                            // outputs, any may be null
    int32_t *key3, *count;
    uint8_t* rgb3;
    int32_t* status;
    unsigned long long* stats;                           // kRsWords counters; the surface cast: one more, the rays whose plane depth was taken
    const uint4* normals;                                // the surface cast (SURFACE): the normal layer (map_normals.h), a record per slot ...
    double shift2_max;                                   // ... max_shift^2 ...
    float* normal;                                       // ... and its normal output, may be null
};

// SURFACE: the surface cast.  The traversal and the hit decision are the plain cast's; a hit whose voxel has a normal gets it, facing the
// ray's origin, and the depth of the plane through the voxel's centroid where vmap::surface_step takes it.
template <bool LAYER, bool SPHERE, bool SURFACE>
__global__ __launch_bounds__(kRayThreads) void k_vmap_raycast(RayJob J) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * kRayThreads + threadIdx.x;
    const bool in = idx < J.n;
    const size_t ii = in ? (size_t)idx : 0;
    float o[3], d[3];
    if (SPHERE) {
        // the dense alignment's source point at depth 1 (sphere_point, convention 2), rotated: every product and sum rounded on its own
        const int r = (int)(ii / (size_t)J.cols), c = (int)(ii - (size_t)r * J.cols);
        const float sp = J.sin_phi[r], cp = J.cos_phi[r], st = J.sin_theta[c], ct = J.cos_theta[c];
        const float fx = sp, fy = (-cp) * st, fz = (-cp) * ct;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            d[k] = (J.pose[k] * fx + J.pose[k + 4] * fy) + J.pose[k + 8] * fz;
            o[k] = J.pose[12 + k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = J.origins[3 * ii + k];
            d[k] = J.dirs[3 * ii + k];
        }
    }
    RayResult H;
    H.status = -1;
    H.t = 0.0;
    H.rec = nullptr;
    H.steps = H.lookups = 0;
    H.cell[0] = H.cell[1] = H.cell[2] = 0;
    if (in) cast_ray<LAYER>(J.G, J.P, o, d, H);
    const bool hit = H.status == kRayHit;
    unsigned long long cnt = 0, col[3] = {0, 0, 0};
    if (hit) {
        cnt = H.rec[1];
#pragma unroll
        for (int k = 0; k < 3; ++k) col[k] = H.rec[5 + k] / cnt;
    }
    double t = H.t;
    float nrm[3] = {0.f, 0.f, 0.f};
    bool on_plane = false;
    if (SURFACE && hit) {
        float c[3];
        centroid(H.rec, cnt, c);
        on_plane = surface_step(J.normals[(H.rec - J.G.table) / kFields], c, o, d, J.P.t_min, (double)J.P.inv_leaf, J.shift2_max, nrm, t);
    }
    if (J.stats) {
        unsigned long long steps = (unsigned long long)H.steps, lookups = (unsigned long long)H.lookups;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            steps += __shfl_xor(steps, off);
            lookups += __shfl_xor(lookups, off);
        }
        unsigned long long b[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) b[q] = __ballot(H.status == q);
        const unsigned long long b_in = __ballot(in), b_plane = SURFACE ? __ballot(on_plane) : 0ull;
        if ((threadIdx.x & 63) == 0 && b_in) {      // one add per wave and counter
            if (SURFACE && b_plane) atomicAdd(J.stats + kRsWords, (unsigned long long)__popcll(b_plane));
            atomicAdd(J.stats + kRsRays, (unsigned long long)__popcll(b_in));
            if (b[kRayHit]) atomicAdd(J.stats + kRsHits, (unsigned long long)__popcll(b[kRayHit]));
            if (b[kRayMissBox]) atomicAdd(J.stats + kRsMissBox, (unsigned long long)__popcll(b[kRayMissBox]));
            if (b[kRayLeftBox]) atomicAdd(J.stats + kRsLeftBox, (unsigned long long)__popcll(b[kRayLeftBox]));
            if (b[kRayTMax]) atomicAdd(J.stats + kRsTMax, (unsigned long long)__popcll(b[kRayTMax]));
            if (b[kRayMaxSteps]) atomicAdd(J.stats + kRsMaxSteps, (unsigned long long)__popcll(b[kRayMaxSteps]));
            if (b[kRayBad]) atomicAdd(J.stats + kRsBad, (unsigned long long)__popcll(b[kRayBad]));
            if (steps) atomicAdd(J.stats + kRsSteps, steps);
            if (lookups) atomicAdd(J.stats + kRsLookups, lookups);
        }
    }
    if (!in) return;
    if (J.t) J.t[ii] = hit ? (float)t : 0.f;
    if (SURFACE && J.normal) {
#pragma unroll
        for (int k = 0; k < 3; ++k) J.normal[3 * ii + k] = nrm[k];
    }
    if (J.key3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) J.key3[3 * ii + k] = hit ? H.cell[k] : 0;
    }
    if (J.count) J.count[ii] = (int32_t)cnt;
    if (J.rgb3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) J.rgb3[3 * ii + k] = (uint8_t)col[k];
    }
    if (J.status) J.status[ii] = H.status;
}

#endif  // RGBD360_RAYCAST_CORE_ONLY
}  // namespace vmap

#if !defined(RGBD360_RAYCAST_CORE_ONLY)
namespace {

static_assert(sizeof(rgbd360_map_raycast_stats) == vmap::kRsWords * sizeof(unsigned long long), "the statistics are the counters in their order");
static_assert(RGBD360_RAY_MISS_BOX == vmap::kRayMissBox && RGBD360_RAY_HIT == vmap::kRayHit && RGBD360_RAY_LEFT_BOX == vmap::kRayLeftBox &&
                  RGBD360_RAY_T_MAX == vmap::kRayTMax && RGBD360_RAY_MAX_STEPS == vmap::kRayMaxSteps && RGBD360_RAY_BAD == vmap::kRayBad,
              "the header's status values");

// what a ray cast checks of its parameters before anything is launched
int ray_check_params(rgbd360_map* m, const rgbd360_map_raycast_params* params, rgbd360_map_raycast_params& p) {
    if (params) p = *params;
    else rgbd360_map_default_raycast_params(m, &p);
    if (p.min_count < 1) return vmap_fail(m, -1, "min_count must be at least 1");
    if (!(p.t_min >= 0.f) || !std::isfinite(p.t_min)) return vmap_fail(m, -1, "t_min must be finite and not negative");
    if (!(p.t_max >= 0.f)) return vmap_fail(m, -1, "t_max must not be negative");
    if (!(p.max_offset >= 0.f)) return vmap_fail(m, -1, "max_offset must not be negative");
    if (p.max_steps < 1 || p.max_steps > (1 << 23)) return vmap_fail(m, -1, "max_steps must lie in 1 .. 2^23");
    return 0;
}
// What the surface entries (rgbd360_map_raycast_surface*) add to a cast; a null RaySurface is the plain cast.  normal and n_on_plane are
// host or device memory as the entry's other outputs and its statistics are.
struct RaySurface {
    const rgbd360_map_normal_params* params;
    float* normal;
    long long* n_on_plane;
};
int ray_check_surface(rgbd360_map* m, const RaySurface* sf, rgbd360_map_normal_params& np) { return sf ? normal_check_params(m, sf->params, np) : 0; }

// The coarse layer and the live-key bounds of the map as it stands: rebuilt when the map has been written since (the revision word).
// The call waits for the first scan (the brick count sizes the masks).  n_voxels > 0.
int ray_layer(rgbd360_map* m) {
    if (m->rc_rev == m->revision) return 0;
    hipStream_t stream = m->s->stream;
    unsigned long long bslots = 64;
    while (bslots < 2ull * (unsigned long long)m->n_voxels) bslots <<= 1;      // at most half full whatever the bricks hold
    HIPC(m, m->rc_bkeys.ensure(bslots));
    HIPC(m, m->rc_bidx.ensure(bslots));
    HIPC(m, m->rc_words.ensure(vmap::kLyWords));
    HIPC(m, m->rc_hwords.ensure(vmap::kLyWords));
    HIPC(m, hipMemsetAsync(m->rc_bkeys, 0xff, bslots * sizeof(unsigned long long), stream));
    HIPC(m, hipMemsetAsync(m->rc_words, 0xff, 3 * sizeof(unsigned), stream));
    HIPC(m, hipMemsetAsync(m->rc_words + vmap::kLyHi, 0, (vmap::kLyWords - vmap::kLyHi) * sizeof(unsigned), stream));
    const dim3 scan((unsigned)((m->n_slots + 255) / 256));
    hipLaunchKernelGGL(vmap::k_vmap_layer_keys, scan, dim3(256), 0, stream, m->table, m->n_slots, m->rc_bkeys, bslots - 1, m->rc_bidx, m->rc_words);
    HIPC(m, hipGetLastError());
    HIPC(m, hipMemcpyAsync(m->rc_hwords, m->rc_words, vmap::kLyWords * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    HIPC(m, hipStreamSynchronize(stream));
    m->rc_bslots = bslots;
    m->rc_bricks = m->rc_hwords[vmap::kLyBricks];
    for (int k = 0; k < 3; ++k) {
        m->rc_lo[k] = (int)m->rc_hwords[vmap::kLyLo + k] - vmap::kBias;
        m->rc_hi[k] = (int)m->rc_hwords[vmap::kLyHi + k] - vmap::kBias;
    }
    if (m->rc_bricks == 0) {      // no live slot: a box no ray meets
        for (int k = 0; k < 3; ++k) m->rc_lo[k] = 0, m->rc_hi[k] = -1;
    }
    HIPC(m, m->rc_masks.ensure(8 * (size_t)m->rc_bricks + 8));
    HIPC(m, hipMemsetAsync(m->rc_masks, 0, 8 * (size_t)m->rc_bricks * sizeof(unsigned long long), stream));
    const vmap::DevGrid G = {m->table, m->n_slots - 1, m->rc_bkeys, bslots - 1, m->rc_bidx, m->rc_masks};
    hipLaunchKernelGGL(vmap::k_vmap_layer_masks, scan, dim3(256), 0, stream, m->table, m->n_slots, G, m->rc_masks);
    HIPC(m, hipGetLastError());
    m->rc_rev = m->revision;
    return 0;
}
size_t ray_layer_bytes(const rgbd360_map* m) {
    return m->rc_rev == m->revision ? (size_t)m->rc_bslots * 12 + (size_t)m->rc_bricks * 64 : 0;
}

// the job of a checked call but for its rays and outputs
vmap::RayJob ray_job(const rgbd360_map* m, const rgbd360_map_raycast_params& p) {
    vmap::RayJob J = {};
    J.G = {m->table, m->n_slots - 1, m->rc_bkeys, m->rc_bslots - 1, m->rc_bidx, m->rc_masks};
    J.P.min_count = (unsigned long long)p.min_count;
    J.P.t_min = (double)p.t_min;
    J.P.t_max = (double)p.t_max;
    J.P.off2_max = (double)p.max_offset * (double)p.max_offset;
    J.P.max_steps = p.max_steps;
    J.P.inv_leaf = m->inv_leaf;
    for (int k = 0; k < 3; ++k) J.P.lo[k] = m->rc_lo[k], J.P.hi[k] = m->rc_hi[k];
    J.stats = m->rc_stats;
    return J;
}
// ... of a surface cast: also the normal layer (ray_prepare has built it) and max_shift
void ray_surface_job(const rgbd360_map* m, vmap::RayJob& J, const rgbd360_map_normal_params& np) {
    J.normals = m->nm_layer;
    J.shift2_max = (double)np.max_shift * (double)np.max_shift;
}
// the kernel over the job, enqueued behind the clear of its counters; plain: the one-level traversal; surface: the surface cast
int ray_launch(rgbd360_map* m, const vmap::RayJob& J, bool sphere, bool plain, bool surface = false) {
    HIPC(m, hipMemsetAsync(m->rc_stats, 0, (vmap::kRsWords + 1) * sizeof(unsigned long long), m->s->stream));
    const dim3 grid((unsigned)((J.n + vmap::kRayThreads - 1) / vmap::kRayThreads)), block(vmap::kRayThreads);
    with_choice<1, 0>(plain, [&](auto L) {
        with_choice<0, 1>(sphere, [&](auto S) {
            with_choice<0, 1>(surface, [&](auto F) {
                hipLaunchKernelGGL((vmap::k_vmap_raycast<decltype(L)::value != 0, decltype(S)::value != 0, decltype(F)::value != 0>), grid, block, 0,
                                   m->s->stream, J);
            });
        });
    });
    HIPC(m, hipGetLastError());
    return 0;
}
void ray_fill_stats(const unsigned long long* w, rgbd360_map_raycast_stats* st) {
    if (!st) return;
    long long* out = &st->n_rays;
    for (int k = 0; k < vmap::kRsWords; ++k) out[k] = w ? (long long)w[k] : 0;
}

// What a panorama call checks before anything is launched (the render's checks); 1: rows cols == 0.  Then the angle tables of the pixel
// grid on the device: the dense alignment's float32 angles (RPI.h:4556-4571), their sine and cosine taken in double and rounded to
// float32, so that the directions do not hang on a C library's sinf.
int ray_sphere_check(rgbd360_map* m, int rows, int cols, const float* pose) {
    if (!pose) return vmap_fail(m, -1, "pose must not be null");
    if (rows < 0 || cols < 0) return vmap_fail(m, -1, "bad image size");
    if (rows == 0 || cols == 0) return 1;
    if (rows < 2 || cols < 8) return vmap_fail(m, -1, "image too small");
    if ((long long)rows * cols >= (1ll << 24) || rows >= (1 << 15) || cols >= (1 << 15)) return vmap_fail(m, -1, "image too large (< 16 Mpx, both sides < 32768)");
    return 0;
}
int ray_sphere_tables(rgbd360_map* m, int rows, int cols) {
    if (m->rc_tab_rows == rows && m->rc_tab_cols == cols) return 0;
    const size_t ntab = (size_t)2 * cols + 2 * rows;
    std::vector<float> tab(ntab);
    float *st = tab.data(), *ct = st + cols, *sp = ct + cols, *cp = sp + rows;
    const float angle_res = 2 * kPI / cols;
    const float half_nRows = 0.5 * rows - 0.5;
    for (int c = 0; c < cols; ++c) {
        const float theta = c * angle_res;
        st[c] = (float)sin((double)theta);
        ct[c] = (float)cos((double)theta);
    }
    for (int r = 0; r < rows; ++r) {
        const float phi = (half_nRows - r) * angle_res;
        sp[r] = (float)sin((double)phi);
        cp[r] = (float)cos((double)phi);
    }
    HIPC(m, m->rc_tab.ensure(ntab));
    m->rc_tab_rows = m->rc_tab_cols = 0;
    HIPC(m, hipMemcpyAsync(m->rc_tab, tab.data(), ntab * sizeof(float), hipMemcpyHostToDevice, m->s->stream));
    HIPC(m, hipStreamSynchronize(m->s->stream));      // `tab` (pageable) must outlive the copy
    m->rc_tab_rows = rows, m->rc_tab_cols = cols;
    return 0;
}
void ray_sphere_job(const rgbd360_map* m, vmap::RayJob& J, int rows, int cols, const float* pose) {
    J.n = (long long)rows * cols;
    J.cols = cols;
    const float* tab = m->rc_tab;
    J.sin_theta = tab, J.cos_theta = tab + cols, J.sin_phi = tab + 2 * cols, J.cos_phi = tab + 2 * cols + rows;
    memcpy(J.pose, pose, sizeof(J.pose));
}
// the buffers every cast needs (the counters and, behind them, the surface cast's n_on_plane), the coarse layer and, for a surface cast
// (np), the normal layer
int ray_prepare(rgbd360_map* m, const rgbd360_map_normal_params* np = nullptr) {
    hipSetDevice(m->s->p.device);
    HIPC(m, m->rc_stats.ensure(vmap::kRsWords + 1));
    HIPC(m, m->rc_hstats.ensure(vmap::kRsWords + 1));
    if (const int rc = ray_layer(m)) return rc;
    return np ? normals_layer(m, *np) : 0;
}

// rgbd360_map_raycast and, with sf, rgbd360_map_raycast_surface
int ray_cast_list(rgbd360_map* m, long long n, const float* origins, const float* dirs, int on_device, const rgbd360_map_raycast_params* params, float* t,
                  int32_t* key3, int32_t* count, uint8_t* rgb3, int32_t* status, rgbd360_map_raycast_stats* stats, const RaySurface* sf) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_raycast_params p;
    rgbd360_map_normal_params np;
    if (const int rc = ray_check_params(m, params, p)) return rc;
    if (const int rc = ray_check_surface(m, sf, np)) return rc;
    if (n < 0 || n >= (1ll << 31)) return vmap_fail(m, -1, "bad ray count");
    if (n > 0 && (!origins || !dirs)) return vmap_fail(m, -1, "origins and dirs must not be null");
    ray_fill_stats(nullptr, stats);
    if (sf && sf->n_on_plane) *sf->n_on_plane = 0;
    if (n == 0) return 0;
    hipSetDevice(m->s->p.device);
    hipStream_t stream = m->s->stream;
    const size_t N = (size_t)n;
    float* normal = sf ? sf->normal : nullptr;
    if (m->n_voxels == 0) {      // nothing to hit: zero-filled outputs (status 0: the ray meets no box), no kernel
        if (on_device) {
            if (t) HIPC(m, hipMemsetAsync(t, 0, N * sizeof(float), stream));
            if (normal) HIPC(m, hipMemsetAsync(normal, 0, N * 3 * sizeof(float), stream));
            if (key3) HIPC(m, hipMemsetAsync(key3, 0, N * 3 * sizeof(int32_t), stream));
            if (count) HIPC(m, hipMemsetAsync(count, 0, N * sizeof(int32_t), stream));
            if (rgb3) HIPC(m, hipMemsetAsync(rgb3, 0, N * 3, stream));
            if (status) HIPC(m, hipMemsetAsync(status, 0, N * sizeof(int32_t), stream));
            HIPC(m, hipStreamSynchronize(stream));
        } else {
            if (t) memset(t, 0, N * sizeof(float));
            if (normal) memset(normal, 0, N * 3 * sizeof(float));
            if (key3) memset(key3, 0, N * 3 * sizeof(int32_t));
            if (count) memset(count, 0, N * sizeof(int32_t));
            if (rgb3) memset(rgb3, 0, N * 3);
            if (status) memset(status, 0, N * sizeof(int32_t));
        }
        return 0;
    }
    if (const int rc = ray_prepare(m, sf ? &np : nullptr)) return rc;
    vmap::RayJob J = ray_job(m, p);
    if (sf) ray_surface_job(m, J, np);
    J.n = n;
    if (on_device) {
        J.origins = origins, J.dirs = dirs;
        J.t = t, J.key3 = key3, J.count = count, J.rgb3 = rgb3, J.status = status, J.normal = normal;
    } else {
        // the rays up, the outputs staged: t, count, status, key3, normal (4-byte arrays first), then rgb3
        HIPC(m, m->rc_rays.ensure(6 * N));
        HIPC(m, m->rc_stage.ensure(39 * N));
        HIPC(m, hipMemcpyAsync(m->rc_rays, origins, 3 * N * sizeof(float), hipMemcpyHostToDevice, stream));
        HIPC(m, hipMemcpyAsync(m->rc_rays + 3 * N, dirs, 3 * N * sizeof(float), hipMemcpyHostToDevice, stream));
        uint8_t* sg = m->rc_stage;
        J.origins = m->rc_rays, J.dirs = m->rc_rays + 3 * N;
        J.t = t ? reinterpret_cast<float*>(sg) : nullptr;
        J.count = count ? reinterpret_cast<int32_t*>(sg + 4 * N) : nullptr;
        J.status = status ? reinterpret_cast<int32_t*>(sg + 8 * N) : nullptr;
        J.key3 = key3 ? reinterpret_cast<int32_t*>(sg + 12 * N) : nullptr;
        J.normal = normal ? reinterpret_cast<float*>(sg + 24 * N) : nullptr;
        J.rgb3 = rgb3 ? sg + 36 * N : nullptr;
    }
    if (const int rc = ray_launch(m, J, false, m->rc_plain, sf != nullptr)) return rc;
    if (!on_device) {
        if (t) HIPC(m, hipMemcpyAsync(t, J.t, N * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (count) HIPC(m, hipMemcpyAsync(count, J.count, N * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        if (status) HIPC(m, hipMemcpyAsync(status, J.status, N * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        if (key3) HIPC(m, hipMemcpyAsync(key3, J.key3, N * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        if (normal) HIPC(m, hipMemcpyAsync(normal, J.normal, N * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (rgb3) HIPC(m, hipMemcpyAsync(rgb3, J.rgb3, N * 3, hipMemcpyDeviceToHost, stream));
    }
    HIPC(m, hipMemcpyAsync(m->rc_hstats, m->rc_stats, (vmap::kRsWords + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPC(m, hipStreamSynchronize(stream));
    ray_fill_stats(m->rc_hstats, stats);
    if (sf && sf->n_on_plane) *sf->n_on_plane = (long long)m->rc_hstats[vmap::kRsWords];
    return 0;
}

// rgbd360_map_raycast_sphere and, with sf, rgbd360_map_raycast_surface_sphere
int ray_cast_sphere(rgbd360_map* m, int rows, int cols, const float* pose, const rgbd360_map_raycast_params* params, float* depth, uint8_t* rgb, int32_t* count,
                    int32_t* key3, rgbd360_map_raycast_stats* stats, const RaySurface* sf) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_raycast_params p;
    rgbd360_map_normal_params np;
    if (const int rc = ray_check_params(m, params, p)) return rc;
    if (const int rc = ray_check_surface(m, sf, np)) return rc;
    const int chk = ray_sphere_check(m, rows, cols, pose);
    if (chk < 0) return chk;
    ray_fill_stats(nullptr, stats);
    if (sf && sf->n_on_plane) *sf->n_on_plane = 0;
    if (chk == 1) return 0;
    const size_t n = (size_t)rows * cols;
    float* normal = sf ? sf->normal : nullptr;
    if (m->n_voxels == 0) {
        if (depth) memset(depth, 0, n * sizeof(float));
        if (normal) memset(normal, 0, n * 3 * sizeof(float));
        if (rgb) memset(rgb, 0, n * 3);
        if (count) memset(count, 0, n * sizeof(int32_t));
        if (key3) memset(key3, 0, n * 3 * sizeof(int32_t));
        return 0;
    }
    if (const int rc = ray_prepare(m, sf ? &np : nullptr)) return rc;
    if (const int rc = ray_sphere_tables(m, rows, cols)) return rc;
    hipStream_t stream = m->s->stream;
    HIPC(m, m->rc_stage.ensure(39 * n));
    uint8_t* sg = m->rc_stage;
    vmap::RayJob J = ray_job(m, p);
    if (sf) ray_surface_job(m, J, np);
    ray_sphere_job(m, J, rows, cols, pose);
    J.t = depth ? reinterpret_cast<float*>(sg) : nullptr;
    J.count = count ? reinterpret_cast<int32_t*>(sg + 4 * n) : nullptr;
    J.key3 = key3 ? reinterpret_cast<int32_t*>(sg + 12 * n) : nullptr;
    J.normal = normal ? reinterpret_cast<float*>(sg + 24 * n) : nullptr;
    J.rgb3 = rgb ? sg + 36 * n : nullptr;
    if (const int rc = ray_launch(m, J, true, m->rc_plain, sf != nullptr)) return rc;
    if (depth) HIPC(m, hipMemcpyAsync(depth, J.t, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (normal) HIPC(m, hipMemcpyAsync(normal, J.normal, n * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (rgb) HIPC(m, hipMemcpyAsync(rgb, J.rgb3, n * 3, hipMemcpyDeviceToHost, stream));
    if (count) HIPC(m, hipMemcpyAsync(count, J.count, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (key3) HIPC(m, hipMemcpyAsync(key3, J.key3, n * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIPC(m, hipMemcpyAsync(m->rc_hstats, m->rc_stats, (vmap::kRsWords + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPC(m, hipStreamSynchronize(stream));
    ray_fill_stats(m->rc_hstats, stats);
    if (sf && sf->n_on_plane) *sf->n_on_plane = (long long)m->rc_hstats[vmap::kRsWords];
    return 0;
}

// rgbd360_map_raycast_sphere_dev and, with sf, rgbd360_map_raycast_surface_sphere_dev
int ray_cast_sphere_dev(rgbd360_map* m, int rows, int cols, const float* pose, const rgbd360_map_raycast_params* params, float* depth_dev, uint8_t* rgb_dev,
                        int32_t* count_dev, int32_t* key3_dev, rgbd360_map_raycast_stats* stats_dev, const RaySurface* sf) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_raycast_params p;
    rgbd360_map_normal_params np;
    if (const int rc = ray_check_params(m, params, p)) return rc;
    if (const int rc = ray_check_surface(m, sf, np)) return rc;
    const int chk = ray_sphere_check(m, rows, cols, pose);
    if (chk < 0) return chk;
    hipSetDevice(m->s->p.device);
    hipStream_t stream = m->s->stream;
    float* normal_dev = sf ? sf->normal : nullptr;
    long long* on_plane_dev = sf ? sf->n_on_plane : nullptr;
    if (chk == 1 || m->n_voxels == 0) {      // nothing to hit: the outputs are cleared on the stream, no kernel
        const size_t n = chk == 1 ? 0 : (size_t)rows * cols;
        if (depth_dev && n) HIPC(m, hipMemsetAsync(depth_dev, 0, n * sizeof(float), stream));
        if (normal_dev && n) HIPC(m, hipMemsetAsync(normal_dev, 0, n * 3 * sizeof(float), stream));
        if (rgb_dev && n) HIPC(m, hipMemsetAsync(rgb_dev, 0, n * 3, stream));
        if (count_dev && n) HIPC(m, hipMemsetAsync(count_dev, 0, n * sizeof(int32_t), stream));
        if (key3_dev && n) HIPC(m, hipMemsetAsync(key3_dev, 0, n * 3 * sizeof(int32_t), stream));
        if (stats_dev) HIPC(m, hipMemsetAsync(stats_dev, 0, sizeof(rgbd360_map_raycast_stats), stream));
        if (on_plane_dev) HIPC(m, hipMemsetAsync(on_plane_dev, 0, sizeof(long long), stream));
        return 0;
    }
    if (const int rc = ray_prepare(m, sf ? &np : nullptr)) return rc;
    if (const int rc = ray_sphere_tables(m, rows, cols)) return rc;
    vmap::RayJob J = ray_job(m, p);
    if (sf) ray_surface_job(m, J, np);
    ray_sphere_job(m, J, rows, cols, pose);
    J.t = depth_dev, J.rgb3 = rgb_dev, J.count = count_dev, J.key3 = key3_dev, J.normal = normal_dev;
    if (const int rc = ray_launch(m, J, true, m->rc_plain, sf != nullptr)) return rc;
    if (stats_dev) HIPC(m, hipMemcpyAsync(stats_dev, m->rc_stats, sizeof(rgbd360_map_raycast_stats), hipMemcpyDeviceToDevice, stream));
    if (on_plane_dev) HIPC(m, hipMemcpyAsync(on_plane_dev, m->rc_stats + vmap::kRsWords, sizeof(long long), hipMemcpyDeviceToDevice, stream));
    return 0;
}

}  // namespace

extern "C" void rgbd360_map_default_raycast_params(const rgbd360_map* m, rgbd360_map_raycast_params* p) {
    if (!p) return;
    p->min_count = 1;
    p->t_min = m ? m->leaf : 0.05f;
    p->t_max = std::numeric_limits<float>::infinity();
    p->max_offset = std::numeric_limits<float>::infinity();
    p->max_steps = 8192;
}

extern "C" int rgbd360_map_raycast(rgbd360_map* m, long long n, const float* origins, const float* dirs, int on_device, const rgbd360_map_raycast_params* params,
                                   float* t, int32_t* key3, int32_t* count, uint8_t* rgb3, int32_t* status, rgbd360_map_raycast_stats* stats) {
    return ray_cast_list(m, n, origins, dirs, on_device, params, t, key3, count, rgb3, status, stats, nullptr);
}
extern "C" int rgbd360_map_raycast_sphere(rgbd360_map* m, int rows, int cols, const float pose[16], const rgbd360_map_raycast_params* params, float* depth,
                                          uint8_t* rgb, int32_t* count, int32_t* key3, rgbd360_map_raycast_stats* stats) {
    return ray_cast_sphere(m, rows, cols, pose, params, depth, rgb, count, key3, stats, nullptr);
}
extern "C" int rgbd360_map_raycast_sphere_dev(rgbd360_map* m, int rows, int cols, const float pose[16], const rgbd360_map_raycast_params* params,
                                              float* depth_dev, uint8_t* rgb_dev, int32_t* count_dev, int32_t* key3_dev, rgbd360_map_raycast_stats* stats_dev) {
    return ray_cast_sphere_dev(m, rows, cols, pose, params, depth_dev, rgb_dev, count_dev, key3_dev, stats_dev, nullptr);
}

// the surface cast: the same rays, checks and outputs, with the normal of each hit and the depth on its plane (map_normals.h)
extern "C" int rgbd360_map_raycast_surface(rgbd360_map* m, long long n, const float* origins, const float* dirs, int on_device,
                                           const rgbd360_map_raycast_params* ray_params, const rgbd360_map_normal_params* normal_params, float* t, float* normal,
                                           int32_t* key3, int32_t* count, uint8_t* rgb3, int32_t* status, long long* n_on_plane,
                                           rgbd360_map_raycast_stats* stats) {
    const RaySurface sf = {normal_params, normal, n_on_plane};
    return ray_cast_list(m, n, origins, dirs, on_device, ray_params, t, key3, count, rgb3, status, stats, &sf);
}
extern "C" int rgbd360_map_raycast_surface_sphere(rgbd360_map* m, int rows, int cols, const float pose[16], const rgbd360_map_raycast_params* ray_params,
                                                  const rgbd360_map_normal_params* normal_params, float* depth, float* normal, uint8_t* rgb, int32_t* count,
                                                  int32_t* key3, long long* n_on_plane, rgbd360_map_raycast_stats* stats) {
    const RaySurface sf = {normal_params, normal, n_on_plane};
    return ray_cast_sphere(m, rows, cols, pose, ray_params, depth, rgb, count, key3, stats, &sf);
}
extern "C" int rgbd360_map_raycast_surface_sphere_dev(rgbd360_map* m, int rows, int cols, const float pose[16], const rgbd360_map_raycast_params* ray_params,
                                                      const rgbd360_map_normal_params* normal_params, float* depth_dev, float* normal_dev, uint8_t* rgb_dev,
                                                      int32_t* count_dev, int32_t* key3_dev, long long* n_on_plane_dev, rgbd360_map_raycast_stats* stats_dev) {
    const RaySurface sf = {normal_params, normal_dev, n_on_plane_dev};
    return ray_cast_sphere_dev(m, rows, cols, pose, ray_params, depth_dev, rgb_dev, count_dev, key3_dev, stats_dev, &sf);
}

// measurement and the traversal switch (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_raycast_set_plain(rgbd360_map* m, int plain) {
    if (!m) return -1;
    m->err.clear();
    m->rc_plain = plain != 0;
    return 0;
}

extern "C" int rgbd360_map_time_raycast(rgbd360_map* m, long long n, const float* origins_dev, const float* dirs_dev, int rows, int cols, const float pose[16],
                                        const rgbd360_map_raycast_params* params, int plain, int reps, float* build_us, float* cast_us, float* scan_us,
                                        rgbd360_map_raycast_stats* stats, long long* layer_bytes) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_raycast_params p;
    if (const int rc = ray_check_params(m, params, p)) return rc;
    const bool sphere = origins_dev == nullptr;
    if (sphere) {
        if (ray_sphere_check(m, rows, cols, pose) != 0) return vmap_fail(m, -1, "bad arguments");
    } else if (n < 1 || n >= (1ll << 31) || !dirs_dev) {
        return vmap_fail(m, -1, "bad arguments");
    }
    if (reps < 1 || !build_us || !cast_us || m->n_voxels == 0) return vmap_fail(m, -1, "bad arguments");
    if (const int rc = ray_prepare(m)) return rc;
    const size_t N = sphere ? (size_t)rows * cols : (size_t)n;
    if (sphere) {
        if (const int rc = ray_sphere_tables(m, rows, cols)) return rc;
    }
    HIPC(m, m->rc_stage.ensure(27 * N));
    HIPC(m, m->x_xyz.ensure(3 * (size_t)m->n_voxels + 3));
    uint8_t* sg = m->rc_stage;
    VmapTimer timer(m, m->s->stream);
    for (int r = 0; r < reps && timer.rc == 0; ++r) {
        timer.timed(build_us[r], 1, [&] {       // both scans with their clears and the read-back between them
            m->rc_rev = 0;
            return ray_layer(m);
        });
        vmap::RayJob J = ray_job(m, p);
        if (sphere) {
            ray_sphere_job(m, J, rows, cols, pose);
        } else {
            J.n = n;
            J.origins = origins_dev, J.dirs = dirs_dev;
            J.status = reinterpret_cast<int32_t*>(sg + 8 * N);
        }
        J.t = reinterpret_cast<float*>(sg);
        J.count = reinterpret_cast<int32_t*>(sg + 4 * N);
        J.key3 = reinterpret_cast<int32_t*>(sg + 12 * N);
        J.rgb3 = sg + 24 * N;
        timer.timed(cast_us[r], 1, [&] { return ray_launch(m, J, sphere, plain != 0); });
        if (scan_us) timer.timed(scan_us[r], 1, [&] { return vmap_launch_extract_scan(m); });
    }
    if (timer.rc) {
        (void)hipGetLastError();
        return timer.rc;
    }
    HIPC(m, hipMemcpyAsync(m->rc_hstats, m->rc_stats, vmap::kRsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->s->stream));
    HIPC(m, hipStreamSynchronize(m->s->stream));
    ray_fill_stats(m->rc_hstats, stats);
    if (layer_bytes) *layer_bytes = (long long)ray_layer_bytes(m);
    return 0;
}
#endif  // RGBD360_RAYCAST_CORE_ONLY
