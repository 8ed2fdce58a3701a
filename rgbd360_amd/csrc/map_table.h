// map_table.h -- the voxel map's table as both device translation units see it: the slot layout, the hash, the read-only lookup, and
// the view through which rgbd360_api.hip (map_render.h: the map rendered as a spherical frame, which needs the dense alignment's warp)
// reaches a map that rgbd360_frame360.hip owns (voxel_map.h).  Like f360_state.h, the seam carries plain pointers and numbers: neither
// unit sees the other's structs or kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct rgbd360_map;

namespace vmap {

constexpr unsigned long long kMaxProbes = 2048;             // of one key in the HBM table (voxel_map.h, the head comment: probe bound)
constexpr int kFields = 8;                                  // 64-bit words per slot: key, count, Sx, Sy, Sz, Sr, Sg, Sb
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kBias = 1 << 20;                              // |i_k| <= 4096 / 0.004 * (1 + 2^-23) < 2^20
constexpr double kFix = 1048576.0;

__host__ __device__ inline unsigned long long mix64(unsigned long long k) {      // (the 64-bit finaliser of MurmurHash3)
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// a key: the three biased 21-bit indices, i_z, i_y, i_x from the top; and the unbiased indices (i_x, i_y, i_z) back out of it
__host__ __device__ inline unsigned long long pack_key(unsigned long long ix, unsigned long long iy, unsigned long long iz) { return (iz << 42) | (iy << 21) | ix; }
__host__ __device__ inline void unpack_key3(unsigned long long key, int32_t out[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (int32_t)((key >> (21 * k)) & 0x1fffffull) - kBias;
}
// the read-out's centroid of the slot `rec`, which holds `count` points
__host__ __device__ __forceinline__ void centroid(const unsigned long long* rec, unsigned long long count, float c[3]) {
#pragma clang fp contract(off)
    const double den = (double)count * kFix;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (float)((double)(long long)rec[2 + k] / den);
}

// the slot of `key` from its first probe on (slot, k0 = the key word there), read only; -1: not in the table
__device__ __forceinline__ long long find(const unsigned long long* __restrict__ table, unsigned long long mask, unsigned long long key, unsigned long long slot,
                                          unsigned long long k0, unsigned& probes) {
    const unsigned long long n_probes = mask < kMaxProbes ? mask + 1 : kMaxProbes;
    for (unsigned long long p = 1;; ++p) {
        if (k0 == key) return (long long)slot;
        if (k0 == kEmpty || p >= n_probes) return -1;
        slot = (slot + 1) & mask;
        k0 = table[slot * kFields];
        ++probes;
    }
}

// What a render works on.  The planes and the staging belong to the map: they grow on demand and go with rgbd360_map_destroy.
enum { kRnVoxels, kRnBelowMin, kRnNear, kRnSplatted, kRnPixels, kRnAtomics, kRnWords };      // rgbd360_map_render_stats in its order, then the
                                                                                             // atomics the depth pass issued (measurement)
struct RenderView {
    int device;
    hipStream_t stream;
    const unsigned long long* table;
    unsigned long long n_slots;
    float leaf;
    long long n_voxels;
    uint32_t* plane_dist;                // one word per pixel: the smallest dist bits that landed
    unsigned long long* plane_key;       // one word per pixel: the smallest key among the voxels of that dist
    unsigned long long* stats;           // kRnWords counters in device memory
    unsigned long long* stats_host;      // ... and their pinned copy
    uint8_t* stage;                      // the host entry's outputs on the device: 23 bytes per pixel (depth, count, key3, rgb)
};

}  // namespace vmap

// rgbd360_frame360.hip (voxel_map.h).  map_view: the table and the map's numbers as they are, nothing allocated.
// map_render_view: also the planes for n_pixels pixels and, with `stage`, the staging; 0 or a HIP error code (the map's error is set).
void rgbd360_map_view(const rgbd360_map* m, vmap::RenderView* v);
int rgbd360_map_render_view(rgbd360_map* m, size_t n_pixels, bool stage, vmap::RenderView* v);
int rgbd360_map_set_error(rgbd360_map* m, int code, const char* msg);      // returns code; (0, "") clears the error as every entry does
// measurement: microseconds per launch of k_vmap_extract over the table (xyz only), the cost of merely scanning it
int rgbd360_map_time_extract_scan(rgbd360_map* m, int reps, float* avg_us);
