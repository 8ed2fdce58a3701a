// map_colour.h -- the colour of the resident voxel map (voxel_map.h) as an alignment can use it: one intensity per voxel and its gradient
// on the voxel's tangent plane, fitted to the intensities of the voxels in the 27 cells around it, kept resident like the normal layer, and
// its two consumers: the read-out (here) and coloured ICP (map_align_colour.h, which follows this header).  Part of the Frame360
// translation unit, behind map_normals.h, whose layer gives the tangent plane.
//
// Definition (include/rgbd360_hip.h, "colour of the map"; tests/map_colour_reference.py restates it in numpy).  Float64
// with + - x / sqrt only, every operation rounded on its own, in the order written: the host, the device and numpy give the same bits.
//   intensity   of a slot with `count` points and colour sums Sr, Sg, Sb: Y = 4899 Sr + 9617 Sg + 1868 Sb in int64 (the dense path's gray
//               weights, their sum 2^14), I64 = (double)Y / (((double)count 16384) 255), a number in [0, 1].  A voxel's I = (float)I64; a
//               source point's is I64 of its three bytes with count 1, kept as a double.
//   status      NONE: count < min_count.  NO_NORMAL: the voxel's record in the normal layer of (min_count, min_support, max_flatness) is
//               not OK.  Otherwise the fit: OK or NO_GRADIENT.
//   basis       n = the doubles of the float32 normal; k = the axis of smallest |n_k|, the lowest index on a tie; t = e_k x n (k = 0:
//               (0, -n_z, n_y); 1: (n_z, 0, -n_x); 2: (-n_y, n_x, 0)), u = t / sqrt((t_x t_x + t_y t_y) + t_z t_z), v = n x u.
//   fit         over the voxels with count >= min_count of the 27 cells other than the voxel itself, in vmap::search27's cell order:
//               r = the float32 difference of the read-out's centroids (neighbour - voxel), widened; a = (r_x u_x + r_y u_y) + r_z u_z,
//               b likewise with v, delta = (double)I_nb - (double)I; the sums m, Saa += a a, Sab += a b, Sbb += b b, Sad += a delta,
//               Sbd += b delta.  NO_GRADIENT when m < min_gradient_support or not det > min_spread (tr tr), det = Saa Sbb - Sab Sab,
//               tr = Saa + Sbb.  Else du = (Sad Sbb - Sbd Sab) / det, dv = (Saa Sbd - Sab Sad) / det, d_k = (float)(du u_k + dv v_k).
//               d is zero unless the status is OK.
// A function of the voxel set, its colour sums and the five parameters alone.  A map fed without colours has I = 0 and d = 0 everywhere
// (every fit gives du = dv = 0): there is no flag that tells.
//
// The layer: one 16-byte record per table slot (colour_pack below), owned by the map, built by the first call that needs it -- behind the
// normal layer it reads -- and reused while the map's revision word and the five parameters stand.  The table is never written.
//
//   k_vmap_colour_layer     the shape of k_vmap_normals: one lane per slot; a voxel with an OK normal walks the 27 cells of its own key
//                           as vmap::search27 does (colour_neighbours below: the same first probes in flight, cell order, vmap::find and
//                           centroid), the five sums riding in the candidate loop, then the 2 x 2 solve.  The walk is written out here
//                           and not hooked into search27: the fit needs the candidate's record and a state to start from, and either
//                           hook changed the machine code of the evaluation kernels that share search27.  Counters
//                           through ballots, one integer atomic per wave and counter.
//   k_vmap_colour_extract   the shape of k_vmap_normals_extract with the record of the slot.
#pragma once

namespace vmap {

enum { kColNone = 0, kColOk = 1, kColNoNormal = 2, kColNoGradient = 3 };
enum { kClVoxels, kClBelowMin, kClNoNormal, kClNoGradient, kClGradients, kClExtract, kClWords };      // rgbd360_map_colour_stats in its order, then
                                                                                                      // the read-out's record counter

// I64 of the definition
__host__ __device__ inline double intensity64(long long sr, long long sg, long long sb, unsigned long long count) {
#pragma clang fp contract(off)
    const long long Y = 4899ll * sr + 9617ll * sg + 1868ll * sb;
    return (double)Y / (((double)count * 16384.0) * 255.0);
}
__host__ __device__ inline float slot_intensity(const unsigned long long* rec, unsigned long long count) {
    return (float)intensity64((long long)rec[5], (long long)rec[6], (long long)rec[7], count);
}

// The fit of one voxel: init with its float32 normal and intensity, add per neighbour, solve.  The function the kernel runs and the host
// entry rgbd360_map_colour_gradient compiles.
struct ColourFit {
    double u[3], v[3], I;
    double saa, sab, sbb, sad, sbd;
    unsigned m;
    __host__ __device__ inline void init(const float n32[3], float I32) {
#pragma clang fp contract(off)
        const double n0 = (double)n32[0], n1 = (double)n32[1], n2 = (double)n32[2];
        const double a0 = n0 < 0.0 ? -n0 : n0, a1 = n1 < 0.0 ? -n1 : n1, a2 = n2 < 0.0 ? -n2 : n2;
        int k = 0;
        double least = a0;
        if (a1 < least) k = 1, least = a1;
        if (a2 < least) k = 2;
        const double t0 = k == 0 ? 0.0 : k == 1 ? n2 : -n1, t1 = k == 0 ? -n2 : k == 1 ? 0.0 : n0, t2 = k == 0 ? n1 : k == 1 ? -n0 : 0.0;
        const double len = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
        u[0] = t0 / len, u[1] = t1 / len, u[2] = t2 / len;
        v[0] = n1 * u[2] - n2 * u[1];
        v[1] = n2 * u[0] - n0 * u[2];
        v[2] = n0 * u[1] - n1 * u[0];
        I = (double)I32;
        saa = sab = sbb = sad = sbd = 0.0;
        m = 0;
    }
    __host__ __device__ inline void add(const float r[3], float I_nb) {
#pragma clang fp contract(off)
        const double rx = (double)r[0], ry = (double)r[1], rz = (double)r[2];
        const double a = (rx * u[0] + ry * u[1]) + rz * u[2], b = (rx * v[0] + ry * v[1]) + rz * v[2], delta = (double)I_nb - I;
        m += 1u;
        saa += a * a;
        sab += a * b;
        sbb += b * b;
        sad += a * delta;
        sbd += b * delta;
    }
    __host__ __device__ inline int solve(unsigned min_gradient_support, double min_spread, float d[3]) const {
#pragma clang fp contract(off)
        d[0] = d[1] = d[2] = 0.f;
        if (m < min_gradient_support) return kColNoGradient;
        const double tr = saa + sbb, det = saa * sbb - sab * sab;
        if (!(det > min_spread * (tr * tr))) return kColNoGradient;
        const double du = (sad * sbb - sbd * sab) / det, dv = (saa * sbd - sab * sad) / det;
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = (float)(du * u[k] + dv * v[k]);
        return kColOk;
    }
};

// The neighbours of the layer build: vmap::search27's walk over the 27 cells of `key` -- its first probes in flight before any is looked
// at, its cell order, vmap::find, count >= min_count, the read-out's centroid -- with what search27's Support does not get to see: the
// candidate's record (its colour sums) and a fit that starts from the voxel's own basis.  Every candidate but the voxel's own slot goes
// into the fit.
__device__ __forceinline__ void colour_neighbours(ColourFit& fit, const unsigned long long* __restrict__ table, unsigned long long mask,
                                                  unsigned long long min_count, unsigned long long key, const unsigned long long* self, const float w[3]) {
#pragma clang fp contract(off)
    const long long ib[3] = {(long long)(key & 0x1fffffull), (long long)((key >> 21) & 0x1fffffull), (long long)(key >> 42)};
    unsigned long long k0[27];
    unsigned n_probes = 0;
#pragma unroll
    for (int c = 0; c < 27; ++c) {
        int dx, dy, dz;
        icp_cell(c, dx, dy, dz);
        const long long nx = ib[0] + dx, ny = ib[1] + dy, nz = ib[2] + dz;
        const bool ok = nx >= 0 && nx < (1ll << 21) && ny >= 0 && ny < (1ll << 21) && nz >= 0 && nz < (1ll << 21);
        k0[c] = ok ? table[(mix64(pack_key(nx, ny, nz)) & mask) * kFields] : kEmpty;
    }
#pragma unroll
    for (int c = 0; c < 27; ++c) {
        if (k0[c] == kEmpty) continue;
        int dx, dy, dz;
        icp_cell(c, dx, dy, dz);
        const unsigned long long ck = pack_key(ib[0] + dx, ib[1] + dy, ib[2] + dz);
        const long long slot = find(table, mask, ck, mix64(ck) & mask, k0[c], n_probes);
        if (slot < 0) continue;
        const unsigned long long* rec = table + (unsigned long long)slot * kFields;
        const unsigned long long cnt = rec[1];
        if (cnt < min_count || cnt == 0 || rec == self) continue;
        float cf[3];
        centroid(rec, cnt, cf);
        const float r[3] = {cf[0] - w[0], cf[1] - w[1], cf[2] - w[2]};
        fit.add(r, slot_intensity(rec, cnt));
    }
}

// A record of the layer, 16 bytes: the bits of I with the status in the two top bits (I lies in [0, 1]: its sign and its top exponent
// bit are never set), then the bits of d.
struct ColourRec {
    int status;
    float I, d[3];
};
__device__ __forceinline__ uint4 colour_pack(int status, float I, const float d[3]) {
    return make_uint4(__float_as_uint(I) | ((unsigned)status << 30), __float_as_uint(d[0]), __float_as_uint(d[1]), __float_as_uint(d[2]));
}
__device__ __forceinline__ ColourRec colour_unpack(const uint4 r) {
    ColourRec R;
    R.status = (int)(r.x >> 30);
    R.I = __uint_as_float(r.x & 0x3fffffffu);
    R.d[0] = __uint_as_float(r.y);
    R.d[1] = __uint_as_float(r.z);
    R.d[2] = __uint_as_float(r.w);
    return R;
}

__global__ __launch_bounds__(kNormalThreads) void k_vmap_colour_layer(const unsigned long long* __restrict__ table, unsigned long long n_slots,
                                                                      unsigned long long min_count, const uint4* __restrict__ normals,
                                                                      unsigned min_gradient_support, double min_spread, uint4* __restrict__ layer,
                                                                      unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    const unsigned long long s = (unsigned long long)blockIdx.x * kNormalThreads + threadIdx.x;
    const bool in = s < n_slots;
    const unsigned long long at = in ? s : 0;
    const unsigned long long* rec = table + at * kFields;
    const ulonglong2 kc = *reinterpret_cast<const ulonglong2*>(rec);      // key, count
    const bool live = in && kc.x != kEmpty && kc.y != 0;                  // (count 0: a tombstone)
    const unsigned long long b_live = __ballot(live);
    float I = 0.f, d[3] = {0.f, 0.f, 0.f};
    int status = kColNone;
    if (!b_live) {
        if (in) layer[s] = colour_pack(status, I, d);
        return;
    }
    const bool fit = live && kc.y >= min_count;
    if (live) I = slot_intensity(rec, kc.y);
    if (fit) {
        const NormalRec nr = normal_unpack(normals[at]);
        if (nr.status != kClassKept) {
            status = kColNoNormal;
        } else {
            float w[3];
            centroid(rec, kc.y, w);
            ColourFit fit;
            fit.init(nr.n, I);
            colour_neighbours(fit, table, n_slots - 1, min_count, kc.x, rec, w);
            status = fit.solve(min_gradient_support, min_spread, d);
        }
    }
    const unsigned long long b_below = __ballot(live && !fit), b_nn = __ballot(status == kColNoNormal), b_ng = __ballot(status == kColNoGradient),
                             b_ok = __ballot(status == kColOk);
    if ((threadIdx.x & 63) == 0) {      // one add per wave and counter
        atomicAdd(stats + kClVoxels, (unsigned long long)__popcll(b_live));
        if (b_below) atomicAdd(stats + kClBelowMin, (unsigned long long)__popcll(b_below));
        if (b_nn) atomicAdd(stats + kClNoNormal, (unsigned long long)__popcll(b_nn));
        if (b_ng) atomicAdd(stats + kClNoGradient, (unsigned long long)__popcll(b_ng));
        if (b_ok) atomicAdd(stats + kClGradients, (unsigned long long)__popcll(b_ok));
    }
    if (in) layer[s] = colour_pack(status, I, d);
}

// the read-out: any output may be null; records beyond max_out are counted, not written
struct ColourOut {
    float *xyz, *intensity, *gradient;
    int32_t *status, *count, *key3;
};
__global__ __launch_bounds__(256) void k_vmap_colour_extract(const unsigned long long* __restrict__ table, unsigned long long n_slots,
                                                             const uint4* __restrict__ layer, long long max_out, unsigned long long* __restrict__ counter,
                                                             ColourOut O) {
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
    const ColourRec R = colour_unpack(layer[at]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (O.xyz) O.xyz[3 * o + k] = w[k];
        if (O.gradient) O.gradient[3 * o + k] = R.d[k];
    }
    if (O.intensity) O.intensity[o] = R.I;
    if (O.status) O.status[o] = R.status;
    if (O.count) O.count[o] = (int32_t)kc.y;
    if (O.key3) unpack_key3(kc.x, O.key3 + 3 * o);
}

}  // namespace vmap

namespace {

static_assert(sizeof(rgbd360_map_colour_stats) == vmap::kClExtract * sizeof(unsigned long long), "the statistics are the counters in their order");
static_assert(sizeof(rgbd360_map_colour_params) == 20, "five 4-byte parameters");
static_assert(RGBD360_COLOUR_NONE == vmap::kColNone && RGBD360_COLOUR_OK == vmap::kColOk && RGBD360_COLOUR_NO_NORMAL == vmap::kColNoNormal &&
                  RGBD360_COLOUR_NO_GRADIENT == vmap::kColNoGradient,
              "the header's status values");

// what every entry that takes colour parameters checks before anything is launched
int colour_check_params(rgbd360_map* m, const rgbd360_map_colour_params* params, rgbd360_map_colour_params& p) {
    if (params) p = *params;
    else rgbd360_map_default_colour_params(m, &p);
    if (p.min_count < 1) return vmap_fail(m, -1, "min_count must be at least 1");
    if (p.min_support < 1 || p.min_support > 27) return vmap_fail(m, -1, "min_support must lie in 1 .. 27");
    if (!(p.max_flatness >= 0.f)) return vmap_fail(m, -1, "max_flatness must not be negative");
    if (p.min_gradient_support < 1 || p.min_gradient_support > 26) return vmap_fail(m, -1, "min_gradient_support must lie in 1 .. 26");
    if (!(p.min_spread >= 0.f)) return vmap_fail(m, -1, "min_spread must not be negative");
    return 0;
}

// The colour layer of the map as it stands under `p`, behind the normal layer of its first three parameters (built or reused as every
// consumer of that layer does): reused while the revision word and the five parameters are those it was built with, else rebuilt -- one
// launch behind the clear of its counters, enqueued on the stream; nothing waits.  n_voxels > 0.
int colour_layer(rgbd360_map* m, const rgbd360_map_colour_params& p) {
    const rgbd360_map_normal_params np = {p.min_count, p.min_support, p.max_flatness, 0.f};
    if (const int rc = normals_layer(m, np)) return rc;
    if (m->cl_rev == m->revision && memcmp(&m->cl_params, &p, sizeof(p)) == 0) return 0;
    hipStream_t stream = m->s->stream;
    m->cl_rev = 0;
    HIPC(m, m->cl_layer.ensure((size_t)m->n_slots));
    HIPC(m, m->cl_stats.ensure(vmap::kClWords));
    HIPC(m, m->cl_hstats.ensure(vmap::kClWords));
    HIPC(m, hipMemsetAsync(m->cl_stats, 0, vmap::kClWords * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(vmap::k_vmap_colour_layer, dim3((unsigned)((m->n_slots + vmap::kNormalThreads - 1) / vmap::kNormalThreads)),
                       dim3(vmap::kNormalThreads), 0, stream, (const unsigned long long*)m->table.get(), m->n_slots, (unsigned long long)p.min_count,
                       (const uint4*)m->nm_layer.get(), (unsigned)p.min_gradient_support, (double)p.min_spread, m->cl_layer.get(), m->cl_stats.get());
    HIPC(m, hipGetLastError());
    m->cl_rev = m->revision;
    m->cl_params = p;
    return 0;
}
void colour_fill_stats(const unsigned long long* w, rgbd360_map_colour_stats* st) {
    if (!st) return;
    long long* out = &st->n_voxels;
    for (int k = 0; k < vmap::kClExtract; ++k) out[k] = w ? (long long)w[k] : 0;
}
int colour_launch_extract(rgbd360_map* m, long long max_out, const vmap::ColourOut& O) {
    unsigned long long* counter = m->cl_stats + vmap::kClExtract;
    HIPC(m, hipMemsetAsync(counter, 0, sizeof(unsigned long long), m->s->stream));
    hipLaunchKernelGGL(vmap::k_vmap_colour_extract, dim3((unsigned)((m->n_slots + 255) / 256)), dim3(256), 0, m->s->stream,
                       (const unsigned long long*)m->table.get(), m->n_slots, (const uint4*)m->cl_layer.get(), max_out, counter, O);
    HIPC(m, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" void rgbd360_map_default_colour_params(const rgbd360_map* m, rgbd360_map_colour_params* p) {
    if (!p) return;
    (void)m;
    p->min_count = 1;            // the three of rgbd360_map_default_normal_params
    p->min_support = 5;
    p->max_flatness = 0.05f;
    p->min_gradient_support = 4;
    p->min_spread = 0.01f;       // (the smaller tangential spread at least a tenth of the larger)
}

extern "C" long long rgbd360_map_colours_dev(rgbd360_map* m, const rgbd360_map_colour_params* params, long long max_out, float* xyz_dev, float* intensity_dev,
                                             float* gradient_dev, int32_t* status_dev, int32_t* count_dev, int32_t* key3_dev,
                                             rgbd360_map_colour_stats* stats_dev) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_colour_params p;
    if (const int rc = colour_check_params(m, params, p)) return rc;
    if (max_out < 0) return vmap_fail(m, -1, "max_out must not be negative");
    hipSetDevice(m->s->p.device);
    if (m->n_voxels == 0) {
        if (stats_dev) HIPC(m, hipMemsetAsync(stats_dev, 0, sizeof(rgbd360_map_colour_stats), m->s->stream));
        return 0;
    }
    if (const int rc = colour_layer(m, p)) return rc;
    if (max_out > 0) {
        if (const int rc = colour_launch_extract(m, max_out, {xyz_dev, intensity_dev, gradient_dev, status_dev, count_dev, key3_dev})) return rc;
    }
    if (stats_dev) HIPC(m, hipMemcpyAsync(stats_dev, m->cl_stats, sizeof(rgbd360_map_colour_stats), hipMemcpyDeviceToDevice, m->s->stream));
    return m->n_voxels;
}

extern "C" long long rgbd360_map_colours(rgbd360_map* m, const rgbd360_map_colour_params* params, long long max_out, float* xyz, float* intensity,
                                         float* gradient, int32_t* status, int32_t* count, int32_t* key3, rgbd360_map_colour_stats* stats) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_colour_params p;
    if (const int rc = colour_check_params(m, params, p)) return rc;
    if (max_out < 0) return vmap_fail(m, -1, "max_out must not be negative");
    colour_fill_stats(nullptr, stats);
    if (m->n_voxels == 0) return 0;
    hipSetDevice(m->s->p.device);
    if (const int rc = colour_layer(m, p)) return rc;
    hipStream_t stream = m->s->stream;
    const size_t n = (size_t)m->n_voxels, n_out = std::min(n, (size_t)max_out);
    // the whole map unsorted (the first max_out of the SORTED map are wanted), 48 bytes a record: xyz, gradient, key3 (three words each),
    // intensity, status, count; then the order of the keys on the host, as rgbd360_map_extract does
    std::vector<float> h(n_out ? 12 * n : 0);
    if (n_out) {
        HIPC(m, m->cl_stage.ensure(48 * n));
        float* sg = reinterpret_cast<float*>(m->cl_stage.get());
        const vmap::ColourOut O = {sg, sg + 9 * n, sg + 3 * n, reinterpret_cast<int32_t*>(sg + 10 * n), reinterpret_cast<int32_t*>(sg + 11 * n),
                                   reinterpret_cast<int32_t*>(sg + 6 * n)};
        if (const int rc = colour_launch_extract(m, (long long)n, O)) return rc;
        HIPC(m, hipMemcpyAsync(h.data(), sg, 48 * n, hipMemcpyDeviceToHost, stream));
    }
    HIPC(m, hipMemcpyAsync(m->cl_hstats, m->cl_stats, vmap::kClWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPC(m, hipStreamSynchronize(stream));
    colour_fill_stats(m->cl_hstats, stats);
    if (!n_out) return m->n_voxels;
    const int32_t* hk = reinterpret_cast<const int32_t*>(h.data() + 6 * n);
    std::vector<size_t> order(n);
    for (size_t k = 0; k < n; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {      // (i_z, i_y, i_x) ascending
        for (int q = 2; q >= 0; --q)
            if (hk[3 * a + q] != hk[3 * b + q]) return hk[3 * a + q] < hk[3 * b + q];
        return false;
    });
    for (size_t o = 0; o < n_out; ++o) {
        const size_t k = order[o];
        for (int q = 0; q < 3; ++q) {
            if (xyz) xyz[3 * o + q] = h[3 * k + q];
            if (gradient) gradient[3 * o + q] = h[3 * n + 3 * k + q];
            if (key3) key3[3 * o + q] = hk[3 * k + q];
        }
        if (intensity) intensity[o] = h[9 * n + k];
        if (status) status[o] = reinterpret_cast<const int32_t*>(h.data())[10 * n + k];
        if (count) count[o] = reinterpret_cast<const int32_t*>(h.data())[11 * n + k];
    }
    return m->n_voxels;
}

extern "C" size_t rgbd360_map_colour_bytes(const rgbd360_map* m) { return m ? m->cl_layer.capacity() * sizeof(uint4) : 0; }
extern "C" int rgbd360_map_release_colours(rgbd360_map* m) {
    if (!m) return -1;
    m->err.clear();
    hipSetDevice(m->s->p.device);
    HIPC(m, hipStreamSynchronize(m->s->stream));
    m->cl_layer.release();
    m->cl_stage.release();
    m->cl_rev = 0;
    return 0;
}

// measurement and tests (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_colour_gradient(const float normal[3], float intensity, int m, const float* r, const float* intensity_nb, int min_gradient_support,
                                           float min_spread, float gradient[3]) {
    if (!normal || !gradient || m < 0 || (m > 0 && (!r || !intensity_nb))) return -1;
    vmap::ColourFit fit;
    fit.init(normal, intensity);
    for (int j = 0; j < m; ++j) fit.add(r + 3 * j, intensity_nb[j]);
    return fit.solve((unsigned)std::max(min_gradient_support, 0), (double)min_spread, gradient);
}
extern "C" double rgbd360_map_colour_intensity(long long sr, long long sg, long long sb, long long count) {
    return count > 0 ? vmap::intensity64(sr, sg, sb, (unsigned long long)count) : 0.0;
}

extern "C" int rgbd360_map_time_colours(rgbd360_map* m, const rgbd360_map_colour_params* params, int reps, float* build_us, float* normals_us, float* scan_us,
                                        rgbd360_map_colour_stats* stats, long long* layer_bytes) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_map_colour_params p;
    if (const int rc = colour_check_params(m, params, p)) return rc;
    if (reps < 1 || !build_us || m->n_voxels == 0) return vmap_fail(m, -1, "bad arguments");
    hipSetDevice(m->s->p.device);
    if (const int rc = colour_layer(m, p)) return rc;       // once untimed: code and buffers there, the normal layer built
    if (scan_us) HIPC(m, m->x_xyz.ensure(3 * (size_t)m->n_voxels + 3));
    const rgbd360_map_normal_params np = {p.min_count, p.min_support, p.max_flatness, 0.f};
    VmapTimer timer(m, m->s->stream);
    for (int r = 0; r < reps && timer.rc == 0; ++r) {
        if (normals_us) timer.timed(normals_us[r], 1, [&] {      // the normal layer's launch with the clear of its counters
            m->nm_rev = 0;
            return normals_layer(m, np);
        });
        timer.timed(build_us[r], 1, [&] {       // this layer's (the normal layer stands)
            m->cl_rev = 0;
            return colour_layer(m, p);
        });
        if (scan_us) timer.timed(scan_us[r], 1, [&] { return vmap_launch_extract_scan(m); });
    }
    if (timer.rc) {
        (void)hipGetLastError();
        return timer.rc;
    }
    HIPC(m, hipMemcpyAsync(m->cl_hstats, m->cl_stats, vmap::kClWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->s->stream));
    HIPC(m, hipStreamSynchronize(m->s->stream));
    colour_fill_stats(m->cl_hstats, stats);
    if (layer_bytes) *layer_bytes = (long long)(m->n_slots * sizeof(uint4));
    return 0;
}
