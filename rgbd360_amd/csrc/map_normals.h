// map_normals.h -- surface normals of the resident voxel map (voxel_map.h): one normal per voxel, fitted to the centroids of the 27 cells
// around it, kept resident like the ray cast's coarse layer, and its two consumers: the read-out with normals (here) and the ray cast
// that returns the surface (map_raycast.h, which follows this header: vmap::surface_step below is its plane depth).  Part of the Frame360
// translation unit, behind map_align.h and map_align_plane.h, whose candidate search and plane fit it calls.
//
// Definition (include/rgbd360_hip.h, "surface normals of the map"; tests/map_normals_reference.py restates it).  Per
// voxel v with count >= min_count: w = the read-out's float32 centroid of v; steps 2-3 of the point-to-plane definition
// (map_align_plane.h) with v's own key as the centre and w as the point -- vmap::search27<PlaneSupport>, the covariance of
// PlaneTail (map_align_plane.h), vmap::plane_fit; status NONE (below min_count) / OK / UNSUPPORTED (m < min_support) / NONPLANAR = vmap::kClass*;
// n32_k = (float)n_k, negated as a whole unless its component of largest magnitude (the earliest on a tie) is positive; curvature
// (float)(l0 / c2), c2 the covariance's trace, 0 when c2 is not positive; normal zero unless OK, curvature zero unless OK or NONPLANAR.
// A function of the voxel set and the three parameters alone.
//
// The layer: one 16-byte record per table slot (NormalRec below), owned by the map, built by the first call that needs it and reused
// while the map's revision word and the three parameters stand (the pattern of rc_rev).  The table is never written.
//
//   k_vmap_normals           one lane per slot; a live voxel runs search27 with its own key and centroid (the first probes of all 27 cells
//                            in flight before any is looked at), then plane_fit.  Slots are not compacted first: at most half are live,
//                            and the dead lanes of a wave wait for its live ones; a wave without a live slot stores its zeros and ends.
//                            Counters through ballots, one integer atomic per wave and counter; no floating-point atomics.
//   k_vmap_normals_extract   the shape of k_vmap_extract (a wave reserves its output range with one counter add) with the record of the
//                            slot and the viewpoint's sign.
#pragma once

namespace vmap {

constexpr int kNormalThreads = 256;
enum { kNmVoxels, kNmBelowMin, kNmUnsupported, kNmNonplanar, kNmNormals, kNmExtract, kNmWords };      // rgbd360_map_normal_stats in its order, then
                                                                                                      // the read-out's record counter

// A record of the layer: the bits of n32 (x, y, z) and of the curvature.  An OK normal has unit length, so its words can not all be small:
// a record whose y and z words are zero and whose x word is at most 3 holds no normal, and that x word is the status (NONE, UNSUPPORTED
// or NONPLANAR; OK is never written there).
struct NormalRec {
    int status;
    float n[3], curvature;
};
__device__ __forceinline__ uint4 normal_pack(int status, const float n[3], float curvature) {
    const bool ok = status == kClassKept;
    return make_uint4(ok ? __float_as_uint(n[0]) : (unsigned)status, ok ? __float_as_uint(n[1]) : 0u, ok ? __float_as_uint(n[2]) : 0u,
                      __float_as_uint(curvature));
}
__device__ __forceinline__ NormalRec normal_unpack(const uint4 r) {
    NormalRec R;
    const bool ok = r.x > 3u || r.y != 0u || r.z != 0u;
    R.status = ok ? (int)kClassKept : (int)r.x;
    R.n[0] = ok ? __uint_as_float(r.x) : 0.f;
    R.n[1] = ok ? __uint_as_float(r.y) : 0.f;
    R.n[2] = ok ? __uint_as_float(r.z) : 0.f;
    R.curvature = __uint_as_float(r.w);
    return R;
}

__global__ __launch_bounds__(kNormalThreads) void k_vmap_normals(const unsigned long long* __restrict__ table, unsigned long long n_slots,
                                                                 unsigned long long min_count, unsigned min_support, double max_flatness,
                                                                 uint4* __restrict__ layer, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    const unsigned long long s = (unsigned long long)blockIdx.x * kNormalThreads + threadIdx.x;
    const bool in = s < n_slots;
    const unsigned long long* rec = table + (in ? s : 0) * kFields;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(rec);      // key, count
    const bool live = in && kc.x != kEmpty && kc.y != 0;                  // (count 0: a tombstone)
    const unsigned long long b_live = __ballot(live);
    float n32[3] = {0.f, 0.f, 0.f}, curvature = 0.f;
    int status = kClassNone;
    if (!b_live) {
        if (in) layer[s] = normal_pack(status, n32, curvature);
        return;
    }
    const bool fit = live && kc.y >= min_count;
    if (fit) {
        float w[3];
        centroid(rec, kc.y, w);
        unsigned n_probes = 0;
        const Match<PlaneSupport> mt = search27<PlaneSupport>(table, n_slots - 1, min_count, kc.x, w, n_probes);
        const PlaneSupport& sp = mt.support;
        if (sp.m < min_support) {
            status = kClassUnsupported;
        } else {
            const double dm = (double)sp.m;
            const double mx = sp.se[0] / dm, my = sp.se[1] / dm, mz = sp.se[2] / dm;
            const double cov[6] = {sp.see[0] / dm - mx * mx, sp.see[1] / dm - mx * my, sp.see[2] / dm - mx * mz,
                                   sp.see[3] / dm - my * my, sp.see[4] / dm - my * mz, sp.see[5] / dm - mz * mz};
            double nrm[3], l0, l1;
            const bool planar = plane_fit(cov, max_flatness, nrm, l0, l1);
            const double c2 = (cov[0] + cov[3]) + cov[5];
            curvature = c2 > 0.0 ? (float)(l0 / c2) : 0.f;
            status = planar ? kClassKept : kClassNonplanar;
            if (planar) {
#pragma unroll
                for (int k = 0; k < 3; ++k) n32[k] = (float)nrm[k];
                // the canonical sign: the component of largest magnitude, the earliest on a tie, is positive
                float big = n32[0];
                if (fabsf(n32[1]) > fabsf(big)) big = n32[1];
                if (fabsf(n32[2]) > fabsf(big)) big = n32[2];
                if (big < 0.f) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) n32[k] = -n32[k];
                }
            }
        }
    }
    const unsigned long long b_below = __ballot(live && !fit), b_uns = __ballot(status == kClassUnsupported),
                             b_non = __ballot(status == kClassNonplanar), b_ok = __ballot(status == kClassKept);
    if ((threadIdx.x & 63) == 0) {      // one add per wave and counter
        atomicAdd(stats + kNmVoxels, (unsigned long long)__popcll(b_live));
        if (b_below) atomicAdd(stats + kNmBelowMin, (unsigned long long)__popcll(b_below));
        if (b_uns) atomicAdd(stats + kNmUnsupported, (unsigned long long)__popcll(b_uns));
        if (b_non) atomicAdd(stats + kNmNonplanar, (unsigned long long)__popcll(b_non));
        if (b_ok) atomicAdd(stats + kNmNormals, (unsigned long long)__popcll(b_ok));
    }
    if (in) layer[s] = normal_pack(status, n32, curvature);
}

// the read-out with normals: any output may be null; records beyond max_out are counted, not written
struct NormalOut {
    float *xyz, *normal, *curvature;
    int32_t *status, *count, *key3;
};
struct NormalView {
    float v[3];
    int has;
};
__global__ __launch_bounds__(256) void k_vmap_normals_extract(const unsigned long long* __restrict__ table, unsigned long long n_slots,
                                                              const uint4* __restrict__ layer, long long max_out, unsigned long long* __restrict__ counter,
                                                              NormalView view, NormalOut O) {
#pragma clang fp contract(off)
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long at = s < n_slots ? s : 0;
    const unsigned long long* rec = table + at * kFields;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(rec);
    const bool occupied = s < n_slots && kc.x != kEmpty && kc.y != 0;
    const unsigned long long wave = __ballot(occupied);
    unsigned long long base = 0;
    if (lane == 0 && wave) base = atomicAdd(counter, (unsigned long long)__popcll(wave));      // one add per wave
    base = __shfl(base, 0);
    const unsigned long long o = base + (unsigned long long)__popcll(wave & ((1ull << lane) - 1ull));
    if (!occupied || (long long)o >= max_out) return;
    float w[3];
    centroid(rec, kc.y, w);
    NormalRec R = normal_unpack(layer[at]);
    if (view.has && R.status == kClassKept) {      // towards the viewpoint
        const double ex = (double)view.v[0] - (double)w[0], ey = (double)view.v[1] - (double)w[1], ez = (double)view.v[2] - (double)w[2];
        if (((double)R.n[0] * ex + (double)R.n[1] * ey) + (double)R.n[2] * ez < 0.0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) R.n[k] = -R.n[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (O.xyz) O.xyz[3 * o + k] = w[k];
        if (O.normal) O.normal[3 * o + k] = R.n[k];
    }
    if (O.curvature) O.curvature[o] = R.curvature;
    if (O.status) O.status[o] = R.status;
    if (O.count) O.count[o] = (int32_t)kc.y;
    if (O.key3) unpack_key3(kc.x, O.key3 + 3 * o);
}

// The surface of a hit (the surface cast, map_raycast.h): `r` the layer's record of the hit voxel, c its centroid, o and d the ray.
// n_out: n32 facing the ray's origin, zero unless the voxel is OK.  True, and t = the ray's depth on the plane through c, iff the voxel is
// OK, q = n . d != 0, t_p >= t_min and the plane point lies within max_shift leaves of c (shift2_max = max_shift^2); the depth is not
// clamped to the cell.
__device__ __forceinline__ bool surface_step(const uint4 r, const float c[3], const float o[3], const float d[3], double t_min, double inv_leaf,
                                             double shift2_max, float n_out[3], double& t) {
#pragma clang fp contract(off)
    const NormalRec R = normal_unpack(r);
    n_out[0] = n_out[1] = n_out[2] = 0.f;
    if (R.status != kClassKept) return false;
    const double nx = (double)R.n[0], ny = (double)R.n[1], nz = (double)R.n[2];
    const double q = (nx * (double)d[0] + ny * (double)d[1]) + nz * (double)d[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) n_out[k] = q > 0.0 ? -R.n[k] : R.n[k];
    if (!(q != 0.0)) return false;
    const double tp = ((nx * ((double)c[0] - (double)o[0]) + ny * ((double)c[1] - (double)o[1])) + nz * ((double)c[2] - (double)o[2])) / q;
    const double f0 = ((double)o[0] + tp * (double)d[0]) - (double)c[0], f1 = ((double)o[1] + tp * (double)d[1]) - (double)c[1],
                 f2 = ((double)o[2] + tp * (double)d[2]) - (double)c[2];
    if (!(tp >= t_min) || !(((f0 * f0 + f1 * f1) + f2 * f2) * (inv_leaf * inv_leaf) <= shift2_max)) return false;
    t = tp;
    return true;
}

}  // namespace vmap

namespace {

static_assert(sizeof(rgbd360_map_normal_stats) == vmap::kNmExtract * sizeof(unsigned long long), "the statistics are the counters in their order");
static_assert(sizeof(rgbd360_map_normal_params) == 16, "four 4-byte parameters");
static_assert(RGBD360_NORMAL_NONE == vmap::kClassNone && RGBD360_NORMAL_OK == vmap::kClassKept && RGBD360_NORMAL_UNSUPPORTED == vmap::kClassUnsupported &&
                  RGBD360_NORMAL_NONPLANAR == vmap::kClassNonplanar,
              "the header's status values");

// what every entry that takes normal parameters checks before anything is launched
int normal_check_params(rgbd360_map* m, const rgbd360_map_normal_params* params, rgbd360_map_normal_params& p) {
    if (params) p = *params;
    else rgbd360_map_default_normal_params(m, &p);
    if (p.min_count < 1) return vmap_fail(m, -1, "min_count must be at least 1");
    if (p.min_support < 1 || p.min_support > 27) return vmap_fail(m, -1, "min_support must lie in 1 .. 27");
    if (!(p.max_flatness >= 0.f)) return vmap_fail(m, -1, "max_flatness must not be negative");
    if (!(p.max_shift >= 0.f)) return vmap_fail(m, -1, "max_shift must not be negative");
    return 0;
}

// The layer of the map as it stands under the three fit parameters of `p`: reused while the revision word and the parameters are those
// it was built with, else rebuilt -- one launch behind the clear of its counters, enqueued on the stream; nothing waits.  n_voxels > 0.
int normals_layer(rgbd360_map* m, const rgbd360_map_normal_params& p) {
    hipSetDevice(m->s->p.device);
    if (m->nm_rev == m->revision && m->nm_min_count == p.min_count && m->nm_min_support == p.min_support &&
        memcmp(&m->nm_max_flatness, &p.max_flatness, sizeof(float)) == 0)
        return 0;
    hipStream_t stream = m->s->stream;
    m->nm_rev = 0;
    HIPC(m, m->nm_layer.ensure((size_t)m->n_slots));
    HIPC(m, m->nm_stats.ensure(vmap::kNmWords));
    HIPC(m, m->nm_hstats.ensure(vmap::kNmWords));
    HIPC(m, hipMemsetAsync(m->nm_stats, 0, vmap::kNmWords * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(vmap::k_vmap_normals, dim3((unsigned)((m->n_slots + vmap::kNormalThreads - 1) / vmap::kNormalThreads)), dim3(vmap::kNormalThreads), 0,
                       stream, (const unsigned long long*)m->table.get(), m->n_slots, (unsigned long long)p.min_count, (unsigned)p.min_support,
                       (double)p.max_flatness, m->nm_layer.get(), m->nm_stats.get());
    HIPC(m, hipGetLastError());
    m->nm_rev = m->revision;
    m->nm_min_count = p.min_count, m->nm_min_support = p.min_support, m->nm_max_flatness = p.max_flatness;
    return 0;
}
void normal_fill_stats(const unsigned long long* w, rgbd360_map_normal_stats* st) {
    if (!st) return;
    long long* out = &st->n_voxels;
    for (int k = 0; k < vmap::kNmExtract; ++k) out[k] = w ? (long long)w[k] : 0;
}
// what both read-outs check: the parameters, max_out and the viewpoint
int normals_check(rgbd360_map* m, const rgbd360_map_normal_params* params, const float* viewpoint, long long max_out, rgbd360_map_normal_params& p,
                  vmap::NormalView& view) {
    if (const int rc = normal_check_params(m, params, p)) return rc;
    if (max_out < 0) return vmap_fail(m, -1, "max_out must not be negative");
    view = {{0.f, 0.f, 0.f}, viewpoint ? 1 : 0};
    for (int k = 0; k < 3 && viewpoint; ++k) {
        if (!std::isfinite(viewpoint[k])) return vmap_fail(m, -1, "the viewpoint must be finite");
        view.v[k] = viewpoint[k];
    }
    return 0;
}
int normals_launch_extract(rgbd360_map* m, long long max_out, const vmap::NormalView& view, const vmap::NormalOut& O) {
    unsigned long long* counter = m->nm_stats + vmap::kNmExtract;
    HIPC(m, hipMemsetAsync(counter, 0, sizeof(unsigned long long), m->s->stream));
    hipLaunchKernelGGL(vmap::k_vmap_normals_extract, dim3((unsigned)((m->n_slots + 255) / 256)), dim3(256), 0, m->s->stream,
                       (const unsigned long long*)m->table.get(), m->n_slots, (const uint4*)m->nm_layer.get(), max_out, counter, view, O);
    HIPC(m, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" void rgbd360_map_default_normal_params(const rgbd360_map* m, rgbd360_map_normal_params* p) {
    if (!p) return;
    (void)m;
    p->min_count = 1;            // the three of rgbd360_map_default_align_plane_params
    p->min_support = 5;
    p->max_flatness = 0.05f;
    p->max_shift = 2.0f;
}

extern "C" long long rgbd360_map_normals_dev(rgbd360_map* m, const rgbd360_map_normal_params* params, const float* viewpoint, long long max_out, float* xyz_dev,
                                             float* normal_dev, float* curvature_dev, int32_t* status_dev, int32_t* count_dev, int32_t* key3_dev,
                                             rgbd360_map_normal_stats* stats_dev) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_normal_params p;
    vmap::NormalView view;
    if (const int rc = normals_check(m, params, viewpoint, max_out, p, view)) return rc;
    hipSetDevice(m->s->p.device);
    if (m->n_voxels == 0) {
        if (stats_dev) HIPC(m, hipMemsetAsync(stats_dev, 0, sizeof(rgbd360_map_normal_stats), m->s->stream));
        return 0;
    }
    if (const int rc = normals_layer(m, p)) return rc;
    if (max_out > 0) {
        if (const int rc = normals_launch_extract(m, max_out, view, {xyz_dev, normal_dev, curvature_dev, status_dev, count_dev, key3_dev})) return rc;
    }
    if (stats_dev) HIPC(m, hipMemcpyAsync(stats_dev, m->nm_stats, sizeof(rgbd360_map_normal_stats), hipMemcpyDeviceToDevice, m->s->stream));
    return m->n_voxels;
}

extern "C" long long rgbd360_map_normals(rgbd360_map* m, const rgbd360_map_normal_params* params, const float* viewpoint, long long max_out, float* xyz,
                                         float* normal, float* curvature, int32_t* status, int32_t* count, int32_t* key3, rgbd360_map_normal_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_normal_params p;
    vmap::NormalView view;
    if (const int rc = normals_check(m, params, viewpoint, max_out, p, view)) return rc;
    normal_fill_stats(nullptr, stats);
    if (m->n_voxels == 0) return 0;
    if (const int rc = normals_layer(m, p)) return rc;
    hipStream_t stream = m->s->stream;
    const size_t n = std::min((size_t)m->n_voxels, (size_t)max_out);
    if (n) {
        // the records staged on the device, 48 bytes each: xyz, normal, key3 (three words each), curvature, status, count
        HIPC(m, m->nm_stage.ensure(48 * n));
        float* sg = reinterpret_cast<float*>(m->nm_stage.get());
        const vmap::NormalOut O = {xyz ? sg : nullptr,
                                   normal ? sg + 3 * n : nullptr,
                                   curvature ? sg + 9 * n : nullptr,
                                   status ? reinterpret_cast<int32_t*>(sg + 10 * n) : nullptr,
                                   count ? reinterpret_cast<int32_t*>(sg + 11 * n) : nullptr,
                                   key3 ? reinterpret_cast<int32_t*>(sg + 6 * n) : nullptr};
        if (const int rc = normals_launch_extract(m, (long long)n, view, O)) return rc;
        if (xyz) HIPC(m, hipMemcpyAsync(xyz, O.xyz, 3 * n * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (normal) HIPC(m, hipMemcpyAsync(normal, O.normal, 3 * n * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (key3) HIPC(m, hipMemcpyAsync(key3, O.key3, 3 * n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        if (curvature) HIPC(m, hipMemcpyAsync(curvature, O.curvature, n * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (status) HIPC(m, hipMemcpyAsync(status, O.status, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        if (count) HIPC(m, hipMemcpyAsync(count, O.count, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    }
    HIPC(m, hipMemcpyAsync(m->nm_hstats, m->nm_stats, vmap::kNmWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPC(m, hipStreamSynchronize(stream));
    normal_fill_stats(m->nm_hstats, stats);
    return m->n_voxels;
}

// measurement (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_time_normals(rgbd360_map* m, const rgbd360_map_normal_params* params, int reps, float* build_us, float* scan_us,
                                        rgbd360_map_normal_stats* stats, long long* layer_bytes) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_normal_params p;
    if (const int rc = normal_check_params(m, params, p)) return rc;
    if (reps < 1 || !build_us || m->n_voxels == 0) return vmap_fail(m, -1, "bad arguments");
    if (const int rc = normals_layer(m, p)) return rc;      // once untimed: code and buffers there
    if (scan_us) HIPC(m, m->x_xyz.ensure(3 * (size_t)m->n_voxels + 3));
    VmapTimer timer(m, m->s->stream);
    for (int r = 0; r < reps && timer.rc == 0; ++r) {
        timer.timed(build_us[r], 1, [&] {       // the launch with the clear of its counters
            m->nm_rev = 0;
            return normals_layer(m, p);
        });
        if (scan_us) timer.timed(scan_us[r], 1, [&] { return vmap_launch_extract_scan(m); });
    }
    if (timer.rc) {
        (void)hipGetLastError();
        return timer.rc;
    }
    HIPC(m, hipMemcpyAsync(m->nm_hstats, m->nm_stats, vmap::kNmWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->s->stream));
    HIPC(m, hipStreamSynchronize(m->s->stream));
    normal_fill_stats(m->nm_hstats, stats);
    if (layer_bytes) *layer_bytes = (long long)(m->n_slots * sizeof(uint4));
    return 0;
}
