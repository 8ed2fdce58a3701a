// map_align_gicp.h -- generalized ICP (Segal, Haehnel, Thrun: plane-to-plane) of a posed sphere frame, of a cloud with normals, or of
// another voxel map against the resident voxel map: the cost of every cloud ICP call site of the reference
// (pcl::GeneralizedIterativeClosestPoint on two voxel-filtered clouds: OdometryRGBD360.cpp:98-114, 210-222, RegisterPairRGBD360.cpp:111-118,
// MethodsRegisterRGBD360.cpp:294-320, OdometryKeyFrame360.cpp:124-140) with the map as its target.  Part of the Frame360 translation
// unit, behind map_normals.h: the target's covariance model is the map's resident per-voxel normal (normals_layer), the match, the row
// sum and the loop are map_align.h's.  Here: the weight of a match, the evaluation's tail (GicpTail), the row's description (GicpMethod)
// and the host's (GicpIcp).
//
// Definition (include/rgbd360_hip.h, "generalized ICP against the map"; tests/map_align_gicp_reference.py restates it in
// numpy).  Per source point at the current pose T = [R | t], float64 with + - x / sqrt only, no contraction:
//   1 match: steps 1-4 of map_align.h, bit for bit (vmap::classify, vmap::search27<NoSupport>, kept iff d2 <= max_dist^2); e = the
//     float32 w - c of the match, widened.
//   2 target covariance: C_B = I - s nb nb^T, s = 1 - epsilon, nb the doubles of the matched voxel's float32 normal, where
//     use_target_normals is set and the voxel's record in the normal layer is OK; else C_B = I.
//   3 source covariance: C_A = I - s na na^T, na = R n^, n^ = n / sqrt(n.n), where a normal array was passed and the point's normal is
//     finite and not zero; else C_A = 0 (the source point is a point).
//   4 weight: M = (C_B + C_A)^-1 by cofactors (vmap::gicp_weight below, the function the host entry rgbd360_map_gicp_weight compiles).
//   5 terms: J = [I | -[w]x]; H += J^T M J (21 terms), g += J^T M e (6), cost += e^T M e, ee += e.e.
//   6 38 float64 words per workgroup row (kGicpWords), the rows added in ascending order; no floating-point atomics.
//   7 H and g straight from the row, cast to float32, gn::step with lambda 0, the stop tests and statuses of map_align.h.
// No normals on either side is point-to-point (M = I exactly), target normals alone point-to-plane with weight 1 / epsilon along the
// normal and 1 across it, normals on both sides plane-to-plane; a pair without a planar side degrades to point-to-point instead of
// dropping out, which is what map_align_plane.h does with corners and edges.
//
//   k_vmap_eval<GicpMethod, SRC>  map_align.h's evaluation on this row, the table and the layer read-only.  No plane fit in the loop: per
//                      kept point ONE 16-byte read of the matched slot's record in the normal layer (the slot rides in search27's Match)
//                      and, with a normal array, 12 bytes of the source (GicpTail).
//   k_vmap_icp_solve<GicpMethod>  map_align.h's solve kernel on this row.
#pragma once

namespace vmap {

// a partial row: n, the 21 upper-triangle terms of sum J^T M J (row by row), sum J^T M e (6), sum e^T M e, sum e.e, then the counters
// n_valid, n_box_rejected, n_out_of_range, n_target_planes, n_source_planes, n_plane_pairs, probes, points searched (all doubles: exact
// integers)
constexpr int kGicpWords = 38;
enum { kGcN = 0, kGcH = 1, kGcG = 22, kGcCost = 28, kGcEE = 29, kGcValid = 30, kGcBox = 31, kGcRange = 32, kGcTarget = 33, kGcSource = 34, kGcPairs = 35,
       kGcProbes = 36, kGcSearched = 37 };
enum { kGicpKept = 1, kGicpTarget = 2, kGicpSource = 4 };      // the bits of a point's class byte

// Steps 2-4: the weight M (upper triangle 00, 01, 02, 11, 12, 22) of a match.  nb: the target voxel's normal (has_b: it has one); na: the
// source point's normal as it was passed (has_a: an array was passed), taken iff its three floats are finite and it is not zero; pose:
// column-major, its rotation turns na into the world.  Returns kGicpTarget | kGicpSource as the two sides were used.  Float64, every
// operation rounded on its own: the host, the device and a restatement in any IEEE arithmetic give the same bits.  C_B + C_A has
// eigenvalues of at least epsilon for epsilon in (0, 1]: there is no failure branch.
__host__ __device__ inline int gicp_weight(const double nb[3], bool has_b, const float na[3], bool has_a, const float pose[16], float epsilon, double M[6]) {
#pragma clang fp contract(off)
    const double s = 1.0 - (double)epsilon;
    double cb[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0}, ca[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (has_b) {
        cb[0] = 1.0 - s * (nb[0] * nb[0]);
        cb[1] = 0.0 - s * (nb[0] * nb[1]);
        cb[2] = 0.0 - s * (nb[0] * nb[2]);
        cb[3] = 1.0 - s * (nb[1] * nb[1]);
        cb[4] = 0.0 - s * (nb[1] * nb[2]);
        cb[5] = 1.0 - s * (nb[2] * nb[2]);
    }
    bool has_source = false;
    if (has_a && __builtin_isfinite(na[0]) && __builtin_isfinite(na[1]) && __builtin_isfinite(na[2])) {
        const double nx = (double)na[0], ny = (double)na[1], nz = (double)na[2];
        const double q = (nx * nx + ny * ny) + nz * nz;
        if (q > 0.0) {
            has_source = true;
            const double len = sqrt(q);
            const double hx = nx / len, hy = ny / len, hz = nz / len;
            double r[3];
            for (int k = 0; k < 3; ++k) r[k] = ((double)pose[k] * hx + (double)pose[k + 4] * hy) + (double)pose[k + 8] * hz;
            ca[0] = 1.0 - s * (r[0] * r[0]);
            ca[1] = 0.0 - s * (r[0] * r[1]);
            ca[2] = 0.0 - s * (r[0] * r[2]);
            ca[3] = 1.0 - s * (r[1] * r[1]);
            ca[4] = 0.0 - s * (r[1] * r[2]);
            ca[5] = 1.0 - s * (r[2] * r[2]);
        }
    }
    const double a00 = cb[0] + ca[0], a01 = cb[1] + ca[1], a02 = cb[2] + ca[2], a11 = cb[3] + ca[3], a12 = cb[4] + ca[4], a22 = cb[5] + ca[5];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    M[0] = c00 / det;
    M[1] = c01 / det;
    M[2] = c02 / det;
    M[3] = c11 / det;
    M[4] = c12 / det;
    M[5] = c22 / det;
    return (has_b ? kGicpTarget : 0) | (has_source ? kGicpSource : 0);
}

// what the evaluation takes beyond EvalCommon.  normal: the source's normals by the point's index (a cloud's), or null; layer: the map's
// normal records by slot, or null (no target normals are used).  The per-point outputs (tests; either may be null): mc_out seven doubles
// per point (M00 M01 M02 M11 M12 M22 and the cost e^T M e; zeros without a kept match), class_out one byte per point (kGicpKept |
// kGicpTarget | kGicpSource).
struct GicpArgs {
    const float* normal;
    const uint4* layer;
    float epsilon;
    double* mc_out;
    uint8_t* class_out;
};
// generalized ICP's tail: steps 2-5 of the definition; W: the weight policy (map_align.h)
template <class W>
struct GicpTailT : PointsOnly {
    double acc[kGcEE + 1];           // n, H (21), g (6), e^T M e, e.e
    W wt;
    unsigned n_target = 0, n_source = 0, n_pairs = 0;
    int pclass;                      // of the point added last, for store(): its class, weight and cost
    double M[6], cost;
    __device__ __forceinline__ GicpTailT() {
#pragma unroll
        for (int q = 0; q <= kGcEE; ++q) acc[q] = 0.0;
    }
    template <class Args>
    __device__ __forceinline__ void add(long long index, const float pose[16], const float w[3], const Match<NoSupport>& mt, bool kept, const Args& args) {
#pragma clang fp contract(off)
        wt.clear();
        pclass = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) M[q] = 0.0;
        cost = 0.0;
        if (kept) {
            double nb[3] = {0.0, 0.0, 0.0};
            bool has_b = false;
            if (args.layer) {        // the one 16-byte read
                const NormalRec rec = normal_unpack(args.layer[mt.best_slot]);
                has_b = rec.status == kClassKept;
#pragma unroll
                for (int q = 0; q < 3; ++q) nb[q] = (double)rec.n[q];
            }
            float na[3] = {0.f, 0.f, 0.f};
            if (args.normal) {
#pragma unroll
                for (int q = 0; q < 3; ++q) na[q] = args.normal[3 * index + q];
            }
            const int used = gicp_weight(nb, has_b, na, args.normal != nullptr, pose, args.epsilon, M);
            pclass = kGicpKept | used;
            n_target += used & kGicpTarget ? 1u : 0u;
            n_source += used & kGicpSource ? 1u : 0u;
            n_pairs += used == (kGicpTarget | kGicpSource) ? 1u : 0u;
            const double m00 = M[0], m01 = M[1], m02 = M[2], m11 = M[3], m12 = M[4], m22 = M[5];
            const double wx = w[0], wy = w[1], wz = w[2], ex = mt.be[0], ey = mt.be[1], ez = mt.be[2];
            // q = M e; m_3..5 = M u_3..5 with u_3 = (0, -wz, wy), u_4 = (wz, 0, -wx), u_5 = (-wy, wx, 0): the columns of -[w]x
            const double qx = (m00 * ex + m01 * ey) + m02 * ez, qy = (m01 * ex + m11 * ey) + m12 * ez, qz = (m02 * ex + m12 * ey) + m22 * ez;
            const double m3[3] = {wy * m02 - wz * m01, wy * m12 - wz * m11, wy * m22 - wz * m12};
            const double m4[3] = {wz * m00 - wx * m02, wz * m01 - wx * m12, wz * m02 - wx * m22};
            const double m5[3] = {wx * m01 - wy * m00, wx * m11 - wy * m01, wx * m12 - wy * m02};
            cost = (ex * qx + ey * qy) + ez * qz;
            const auto s = [&] { return cost; };
            wt.set(s, args);
            acc[kGcN] += wt(1.0);
            double* H = acc + kGcH;  // rows 0 .. 5 of the upper triangle
            H[0] += wt(m00), H[1] += wt(m01), H[2] += wt(m02), H[3] += wt(m3[0]), H[4] += wt(m4[0]), H[5] += wt(m5[0]);
            H[6] += wt(m11), H[7] += wt(m12), H[8] += wt(m3[1]), H[9] += wt(m4[1]), H[10] += wt(m5[1]);
            H[11] += wt(m22), H[12] += wt(m3[2]), H[13] += wt(m4[2]), H[14] += wt(m5[2]);
            H[15] += wt(wy * m3[2] - wz * m3[1]), H[16] += wt(wy * m4[2] - wz * m4[1]), H[17] += wt(wy * m5[2] - wz * m5[1]);
            H[18] += wt(wz * m4[0] - wx * m4[2]), H[19] += wt(wz * m5[0] - wx * m5[2]);
            H[20] += wt(wx * m5[1] - wy * m5[0]);
            acc[kGcG] += wt(qx);
            acc[kGcG + 1] += wt(qy);
            acc[kGcG + 2] += wt(qz);
            acc[kGcG + 3] += wt(wy * qz - wz * qy);
            acc[kGcG + 4] += wt(wz * qx - wx * qz);
            acc[kGcG + 5] += wt(wx * qy - wy * qx);
            acc[kGcCost] += wt.rho(s);
            acc[kGcEE] += (ex * ex + ey * ey) + ez * ez;
        }
    }
    template <class Args>
    __device__ __forceinline__ void store(long long index, const Args& args) const {
        wt.store(index, args);
        if (args.mc_out) {
#pragma unroll
            for (int q = 0; q < 6; ++q) args.mc_out[7 * index + q] = M[q];
            args.mc_out[7 * index + 6] = cost;
        }
        if (args.class_out) args.class_out[index] = (uint8_t)pclass;
    }
    __device__ __forceinline__ void row(double* out) const {
#pragma unroll
        for (int q = 0; q <= kGcEE; ++q) out[q] = acc[q];
        out[kGcTarget] = (double)n_target;
        out[kGcSource] = (double)n_source;
        out[kGcPairs] = (double)n_pairs;
        wt.row(out + kGicpWords);
    }
};
using GicpTail = GicpTailT<UnitWeight>;

struct GicpMethod {
    static constexpr int kWords = kGicpWords, kN = kGcN, kSumSq = kGcCost, kCounters = kGcValid, kProbes = kGcProbes, kSearched = kGcSearched;
    __host__ __device__ static void assemble(const double* s, float* H, float* g) { plane_assemble(s, H, g); }      // (the plane row's places)
    using Support = NoSupport;
    using Args = GicpArgs;
    using Tail = GicpTail;
    template <class W>
    using TailT = GicpTailT<W>;
};
static_assert(kGcValid + 1 == kGcBox && kGcValid + 2 == kGcRange, "the three counters of every method lead the row's counters");
static_assert(kGcH == kPlH && kGcG == kPlG, "H and g lie where plane_assemble reads them");
static_assert(kGicpWords <= kIcpMaxWords, "the buffers of a map hold the widest row");

}  // namespace vmap

namespace {

static_assert(sizeof(rgbd360_map_align_gicp_params) == 40 && sizeof(rgbd360_map_align_gicp_result) == 256, "the header's structs");

struct GicpIcp : vmap::GicpMethod {
    using Row = vmap::GicpMethod;
    static constexpr int kMethod = RGBD360_MAP_METHOD_GICP;
    using Params = rgbd360_map_align_gicp_params;
    using Result = rgbd360_map_align_gicp_result;
    struct Out {
        int32_t* key3 = nullptr;
        float* d2 = nullptr;
        double* weight_cost = nullptr;
        uint8_t* cls = nullptr;
    };
    static int check(rgbd360_map* m, const Params* params, IcpJob& job) {
        Params p;
        if (params) p = *params;
        else rgbd360_map_default_align_gicp_params(m, &p);
        const rgbd360_map_align_params shared = {p.max_dist, p.max_iters, p.eps, p.min_count, p.min_matches};
        if (const int rc = icp_check_params(m, &shared, job.p)) return rc;
        if (!(p.epsilon > 0.f && p.epsilon <= 1.f)) return vmap_fail(m, -1, "epsilon must lie in (0, 1]");
        if (p.min_support < 1 || p.min_support > 27) return vmap_fail(m, -1, "min_support must lie in 1 .. 27");
        if (!(p.max_flatness >= 0.f)) return vmap_fail(m, -1, "max_flatness must not be negative");
        job.min_support = p.min_support;
        job.max_flatness = p.max_flatness;
        job.epsilon = p.epsilon;
        job.use_target_normals = p.use_target_normals != 0;
        return 0;
    }
    // the map's normal layer under this call's parameters, built or reused as the surface cast does (normals_layer: a comparison on the
    // host while the map's revision and the parameters stand), ahead of the kernel on the stream
    static int eval_args(rgbd360_map* m, const IcpJob& job, const Out& o, Args& a) {
        const uint4* layer = nullptr;
        if (job.use_target_normals && m->n_voxels > 0) {
            const rgbd360_map_normal_params np = {job.p.min_count, job.min_support, job.max_flatness, 0.f};
            if (const int rc = normals_layer(m, np)) return rc;
            layer = m->nm_layer.get();
        }
        a = {job.src.cloud ? job.normal : nullptr, layer, job.epsilon, o.weight_cost, o.cls};
        return 0;
    }
    static void fill_extra(const double* row, double n, Result* res) {      // (n: the kept matches)
        res->n_target_planes = (long long)row[vmap::kGcTarget];
        res->n_source_planes = (long long)row[vmap::kGcSource];
        res->n_plane_pairs = (long long)row[vmap::kGcPairs];
        res->fitness_point = n > 0.0 ? row[vmap::kGcEE] / n : 0.0;
    }
};

MapInput gicp_cloud_input(const float* xyz, const float* normal, long long n, int on_device) {
    MapInput in = cloud_input(xyz, nullptr, n, on_device);
    in.normal = n > 0 ? normal : nullptr;
    return in;
}
}  // namespace

extern "C" void rgbd360_map_default_align_gicp_params(const rgbd360_map* m, rgbd360_map_align_gicp_params* p) {
    if (!p) return;
    rgbd360_map_align_plane_params plane;
    rgbd360_map_default_align_plane_params(m, &plane);
    memset(p, 0, sizeof(*p));
    p->max_dist = plane.max_dist;
    p->max_iters = plane.max_iters;
    p->eps = plane.eps;
    p->min_count = plane.min_count;
    p->min_matches = plane.min_matches;
    p->epsilon = 1e-3f;          // PCL's gicp_epsilon_
    p->use_target_normals = 1;
    p->min_support = plane.min_support;
    p->max_flatness = plane.max_flatness;
}

extern "C" int rgbd360_map_align_gicp_sphere(rgbd360_map* m, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                             const float guess[16], int on_device, const rgbd360_map_align_gicp_params* params, float pose_out[16],
                                             rgbd360_map_align_gicp_result* result) {
    return icp_by_setting<GicpIcp>(m, [&](auto M) {
        return icp_align<typename decltype(M)::type>(m, sphere_input(nullptr, 0, depth, depth_step, depth_type, rows, cols, convention, on_device), guess, params,
                                                     pose_out, result);
    });
}
extern "C" int rgbd360_map_align_gicp_cloud(rgbd360_map* m, const float* xyz, const float* normal, long long n, const float guess[16], int on_device,
                                            const rgbd360_map_align_gicp_params* params, float pose_out[16], rgbd360_map_align_gicp_result* result) {
    return icp_by_setting<GicpIcp>(m, [&](auto M) {
        return icp_align<typename decltype(M)::type>(m, gicp_cloud_input(xyz, normal, n, on_device), guess, params, pose_out, result);
    });
}

// measurement and tests (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_gicp_weight(const double nb[3], int has_b, const float na[3], int has_a, const float pose[16], float epsilon, double M[6]) {
    if (!pose || !M || (has_b && !nb) || (has_a && !na)) return -1;
    const double zero[3] = {0.0, 0.0, 0.0};
    const float zerof[3] = {0.f, 0.f, 0.f};
    return vmap::gicp_weight(has_b ? nb : zero, has_b != 0, has_a ? na : zerof, has_a != 0, pose, epsilon, M);
}

extern "C" int rgbd360_map_align_gicp_eval(rgbd360_map* m, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                           const float* xyz, const float* normal, long long n, const float pose[16], int on_device,
                                           const rgbd360_map_align_gicp_params* params, double row[30], long long counters[6], int32_t* key3_dev,
                                           float* d2_dev, double* weight_cost_dev, uint8_t* class_dev) {
    if (!m) return -1;
    m->err.clear();
    if (!pose) return vmap_fail(m, -1, "pose must not be null");
    MapInput in = icp_eval_input(depth, depth_step, depth_type, rows, cols, convention, xyz, n, on_device);
    if (in.cloud && n > 0) in.normal = normal;
    return icp_eval<GicpIcp>(m, in, pose, params, row, counters, {key3_dev, d2_dev, weight_cost_dev, class_dev});
}

extern "C" int rgbd360_map_time_align_gicp(rgbd360_map* m, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                           const float pose[16], const rgbd360_map_align_gicp_params* params, int reps, float avg_us[5], double* probes) {
    if (!m) return -1;
    m->err.clear();
    const MapInput in = sphere_input(nullptr, 0, depth_dev, depth_step, depth_type, rows, cols, convention, 1);
    if (const int rc = vmap_check_timed(m, in, pose, reps, avg_us)) return rc;
    IcpJob job;
    if (const int rc = GicpIcp::check(m, params, job)) return rc;
    if (const int rc = icp_prepare(m, in, job)) return rc;
    const vmap::Params P = vmap_params(m, pose);
    VmapTimer timer(m, m->s->stream);        // made last
    if (timer.rc) return timer.rc;
    int& rc = timer.rc;
    // the point-to-point and point-to-plane kernels first, on the same frame, map and buffers, then this method's, whose state stays behind
    rc = icp_launch_init<PointIcp>(m, pose);
    if (rc == 0) rc = icp_launch_eval<PointIcp>(m, job, P, 1, {});      // once untimed: code and tables loaded
    timer.timed(avg_us[1], reps, [&] { return icp_launch_eval<PointIcp>(m, job, P, 1, {}); });
    if (rc == 0) rc = icp_launch_init<PlaneIcp>(m, pose);
    if (rc == 0) rc = icp_launch_eval<PlaneIcp>(m, job, P, 1, {});
    timer.timed(avg_us[2], reps, [&] { return icp_launch_eval<PlaneIcp>(m, job, P, 1, {}); });
    if (rc == 0) rc = icp_launch_init<GicpIcp>(m, pose);
    if (rc == 0) rc = icp_launch_eval<GicpIcp>(m, job, P, 1, {});       // (and the normal layer built)
    timer.timed(avg_us[0], reps, [&] { return icp_launch_eval<GicpIcp>(m, job, P, 1, {}); });
    timer.timed(avg_us[3], reps, [&] { return icp_launch_solve<GicpIcp>(m, job, 1); });
    if (rc == 0 && probes) rc = icp_read_probes<GicpIcp>(m, probes);
    if (const int failed = timer.finish(avg_us, 0, reps)) return failed;
    return icp_time_whole<GicpIcp>(m, job, pose, reps, avg_us[4]);
}
