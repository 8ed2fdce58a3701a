// map_align_plane.h -- point-to-plane ICP of a posed sphere frame, or of a cloud, against the resident voxel map: the plane cost the
// reference's call sites actually use (pcl::GeneralizedIterativeClosestPoint, a plane-to-plane cost: OdometryRGBD360.cpp:98-114, 210-222,
// RegisterPairRGBD360.cpp:111-118, MethodsRegisterRGBD360.cpp:294-320) with the map as its target.  Part of the Frame360 translation unit,
// behind map_align.h, which holds what the methods share: the lookup (vmap::find, icp_cell), the loop's state and kernels, the host
// driver (icp_align<M> and icp_eval<M> on a MapInput) and the trace.  Here: the plane fit, the evaluation's tail (PlaneTail), the row's description (PlaneMethod) and the host's (PlaneIcp).
//
// Definition (include/rgbd360_hip.h, "point-to-plane ICP of a frame against the map"; tests/map_align_plane_reference.py
// restates it in numpy).  Per source point at the current pose:
//   1 candidates and match: steps 1-4 of map_align.h, bit for bit (the same key and d2 per point): eval_tile's, whatever the method.
//   2 support: over ALL m candidates e_j = (double)w - (double)c_j, sum e (3) and sum e e^T (6) in float64 in the cells' order;
//     e_mean = sum e / m (= w - mu, mu the mean centroid), C = sum e e^T / m - e_mean e_mean^T.  A kept point with m < min_support is
//     counted in n_unsupported.
//   3 plane: vmap::plane_fit below -- the smallest eigenvalue of C by Newton's method on the characteristic polynomial from 0, its vector
//     from the largest cross product of two rows of C - l0 I, the middle eigenvalue from the deflated quadratic; planar iff the cross
//     product is not zero, l1 > 0 and l0 <= max_flatness l1, else the point is counted in n_nonplanar (room corners and edges).
//   4 r = n . e_mean, J = [n ; w x n] in float64.
//   5 37 float64 sums per workgroup row (kPlaneWords), the rows added in ascending order; no floating-point atomics.
//   6 H and g straight from the row, cast to float32, gn::step with lambda 0, the stop tests and statuses of map_align.h.
// The map stores no normals and insertion is unchanged: the plane comes from the centroids the lookup has already loaded.
//
//   k_vmap_eval<PlaneMethod, SRC>  map_align.h's evaluation on this row: the nine support sums ride in the candidate loop as search27's
//                       PlaneSupport, the plane fit runs once per kept point with enough support (PlaneTail).
//   k_vmap_icp_solve<PlaneMethod>  map_align.h's solve kernel on this row.
#pragma once

namespace vmap {

// a partial row: n, the 21 upper-triangle terms of sum J J^T (row by row), sum J r (6), sum r r, sum e_match . e_match, then the counters
// n_valid, n_box_rejected, n_out_of_range, n_unsupported, n_nonplanar, probes, points searched (all doubles: exact integers)
constexpr int kPlaneWords = 37;
enum { kPlN = 0, kPlH = 1, kPlG = 22, kPlRR = 28, kPlEE = 29, kPlValid = 30, kPlBox = 31, kPlRange = 32, kPlUnsupported = 33, kPlNonplanar = 34,
       kPlProbes = 35, kPlSearched = 36 };
enum { kClassNone = 0, kClassKept = 1, kClassUnsupported = 2, kClassNonplanar = 3 };

// The plane of a support: a = the upper triangle (00, 01, 02, 11, 12, 22) of the covariance C.  n: the unit eigenvector of the smallest
// eigenvalue l0; true iff the support is planar.  Float64 with + - x / sqrt only, every operation rounded on its own: the host, the device
// and a restatement in any IEEE arithmetic give the same bits.  (The Newton iteration and the cross-product eigenvector are those of
// k_f360_slot_frames, frame360_kernels.h, which keeps its own copy: DESIGN.md 3.13.)
__host__ __device__ inline bool plane_fit(const double a[6], double max_flatness, double n[3], double& l0_out, double& l1_out) {
#pragma clang fp contract(off)
    const double a00 = a[0], a01 = a[1], a02 = a[2], a11 = a[3], a12 = a[4], a22 = a[5];
    // f(l) = l^3 - c2 l^2 + c1 l - c0
    const double c2 = (a00 + a11) + a22;
    const double c1 = ((a00 * a11 - a01 * a01) + (a00 * a22 - a02 * a02)) + (a11 * a22 - a12 * a12);
    const double c0 = (a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a12 * a02)) + a02 * (a01 * a12 - a11 * a02);
    double l = 0.0;
    for (int it = 0; it < 12; ++it) {
        const double f = ((l - c2) * l + c1) * l - c0, df = (3.0 * l - 2.0 * c2) * l + c1;
        if (!(df > 0.0)) break;
        const double step = f / df;
        l = l - step;
        if ((step < 0.0 ? -step : step) <= 1e-15 * c2) break;
    }
    const double r0[3] = {a00 - l, a01, a02}, r1[3] = {a01, a11 - l, a12}, r2[3] = {a02, a12, a22 - l};
    const double n01[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
    const double n02[3] = {r0[1] * r2[2] - r0[2] * r2[1], r0[2] * r2[0] - r0[0] * r2[2], r0[0] * r2[1] - r0[1] * r2[0]};
    const double n12[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    const double q01 = (n01[0] * n01[0] + n01[1] * n01[1]) + n01[2] * n01[2];
    const double q02 = (n02[0] * n02[0] + n02[1] * n02[1]) + n02[2] * n02[2];
    const double q12 = (n12[0] * n12[0] + n12[1] * n12[1]) + n12[2] * n12[2];
    double qq = q01;
    n[0] = n01[0], n[1] = n01[1], n[2] = n01[2];
    if (q02 > qq) qq = q02, n[0] = n02[0], n[1] = n02[1], n[2] = n02[2];
    if (q12 > qq) qq = q12, n[0] = n12[0], n[1] = n12[1], n[2] = n12[2];
    // the middle eigenvalue: the smaller root of the quadratic left when l0 is divided out
    const double s = c2 - l, p = c1 - l * s;
    const double disc = s * s - 4.0 * p;
    const double l1 = 0.5 * (s - sqrt(disc > 0.0 ? disc : 0.0));
    l0_out = l;
    l1_out = l1;
    if (!(qq > 0.0)) {
        n[0] = n[1] = n[2] = 0.0;
        return false;
    }
    const double len = sqrt(qq);
    n[0] = n[0] / len;
    n[1] = n[1] / len;
    n[2] = n[2] / len;
    return l1 > 0.0 && l <= max_flatness * l1;
}

// the support of a point (step 2 of the definition): over every candidate of vmap::search27, in the cells' order, the difference in double
struct PlaneSupport {
    double se[3] = {0.0, 0.0, 0.0}, see[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned m = 0;
    __device__ __forceinline__ void add(const float w[3], const float cf[3]) {
#pragma clang fp contract(off)
        const double ex = (double)w[0] - (double)cf[0], ey = (double)w[1] - (double)cf[1], ez = (double)w[2] - (double)cf[2];
        m += 1u;
        se[0] += ex;
        se[1] += ey;
        se[2] += ez;
        see[0] += ex * ex;
        see[1] += ex * ey;
        see[2] += ex * ez;
        see[3] += ey * ey;
        see[4] += ey * ez;
        see[5] += ez * ez;
    }
};

// what the evaluation takes beyond EvalCommon; the per-point outputs (tests; either may be null): nr_out four doubles per point (the
// normal and r; zeros unless the class is kept), class_out one byte per point (key3: the key of the kept MATCH whatever the point's class)
struct PlaneArgs {
    unsigned min_support;
    double max_flatness;
    double* nr_out;
    uint8_t* class_out;
};
// point-to-plane's tail: steps 2-5 of the definition on the support search27 carried; W: the weight policy (map_align.h)
template <class W>
struct PlaneTailT : PointsOnly {
    double acc[kPlRR + 2];           // n, H (21), g (6), r r, e.e
    W wt;
    unsigned n_unsupported = 0, n_nonplanar = 0;
    int pclass;                      // of the point added last, for store(): its class, normal and r
    double nrm[3], r;
    __device__ __forceinline__ PlaneTailT() {
#pragma unroll
        for (int q = 0; q < kPlRR + 2; ++q) acc[q] = 0.0;
    }
    template <class Args>
    __device__ __forceinline__ void add(long long, const float*, const float w[3], const Match<PlaneSupport>& mt, bool kept, const Args& args) {
#pragma clang fp contract(off)
        const PlaneSupport& sp = mt.support;
        wt.clear();
        pclass = kClassNone;
        nrm[0] = nrm[1] = nrm[2] = 0.0, r = 0.0;
        if (kept && sp.m < args.min_support) {
            pclass = kClassUnsupported;
            n_unsupported += 1u;
        } else if (kept) {
            const double dm = (double)sp.m;
            const double mx = sp.se[0] / dm, my = sp.se[1] / dm, mz = sp.se[2] / dm;
            const double cov[6] = {sp.see[0] / dm - mx * mx, sp.see[1] / dm - mx * my, sp.see[2] / dm - mx * mz,
                                   sp.see[3] / dm - my * my, sp.see[4] / dm - my * mz, sp.see[5] / dm - mz * mz};
            double l0, l1;
            if (plane_fit(cov, args.max_flatness, nrm, l0, l1)) {
                pclass = kClassKept;
                r = (nrm[0] * mx + nrm[1] * my) + nrm[2] * mz;
                const double wx = w[0], wy = w[1], wz = w[2];
                const double J[6] = {nrm[0], nrm[1], nrm[2], wy * nrm[2] - wz * nrm[1], wz * nrm[0] - wx * nrm[2], wx * nrm[1] - wy * nrm[0]};
                const double ex = mt.be[0], ey = mt.be[1], ez = mt.be[2];
                const auto s = [&] { return r * r; };
                wt.set(s, args);
                acc[kPlN] += wt(1.0);
                int h = kPlH;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
#pragma unroll
                    for (int b = a; b < 6; ++b) acc[h++] += wt(J[a] * J[b]);
                }
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[kPlG + a] += wt(J[a] * r);
                acc[kPlRR] += wt.rho(s);
                acc[kPlEE] += (ex * ex + ey * ey) + ez * ez;
            } else {
                pclass = kClassNonplanar;
                n_nonplanar += 1u;
                nrm[0] = nrm[1] = nrm[2] = 0.0;
            }
        }
    }
    template <class Args>
    __device__ __forceinline__ void store(long long index, const Args& args) const {
        wt.store(index, args);
        if (args.nr_out) {
            args.nr_out[4 * index] = nrm[0];
            args.nr_out[4 * index + 1] = nrm[1];
            args.nr_out[4 * index + 2] = nrm[2];
            args.nr_out[4 * index + 3] = r;
        }
        if (args.class_out) args.class_out[index] = (uint8_t)pclass;
    }
    __device__ __forceinline__ void row(double* out) const {
#pragma unroll
        for (int q = 0; q < kPlRR + 2; ++q) out[q] = acc[q];
        out[kPlUnsupported] = (double)n_unsupported;
        out[kPlNonplanar] = (double)n_nonplanar;
        wt.row(out + kPlaneWords);
    }
};
using PlaneTail = PlaneTailT<UnitWeight>;

// H (column-major, symmetric) and g from the row
__host__ __device__ inline void plane_assemble(const double* s, float* H, float* g) {
    int h = kPlH;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++h) H[b * 6 + a] = H[a * 6 + b] = (float)s[h];
    for (int k = 0; k < 6; ++k) g[k] = (float)s[kPlG + k];
}

struct PlaneMethod {
    static constexpr int kWords = kPlaneWords, kN = kPlN, kSumSq = kPlRR, kCounters = kPlValid, kProbes = kPlProbes, kSearched = kPlSearched;
    __host__ __device__ static void assemble(const double* s, float* H, float* g) { plane_assemble(s, H, g); }
    using Support = PlaneSupport;
    using Args = PlaneArgs;
    using Tail = PlaneTail;
    template <class W>
    using TailT = PlaneTailT<W>;
};
static_assert(kPlValid + 1 == kPlBox && kPlValid + 2 == kPlRange, "the three counters of every method lead the row's counters");
static_assert(kPlaneWords <= kIcpMaxWords, "the buffers of a map hold the widest row");

}  // namespace vmap

namespace {

struct PlaneIcp : vmap::PlaneMethod {
    using Row = vmap::PlaneMethod;
    static constexpr int kMethod = RGBD360_MAP_METHOD_PLANE;
    using Params = rgbd360_map_align_plane_params;
    using Result = rgbd360_map_align_plane_result;
    struct Out {                 // (the key of the kept MATCH whatever the point's class)
        int32_t* key3 = nullptr;
        float* d2 = nullptr;
        double* normal_r = nullptr;
        uint8_t* cls = nullptr;
    };
    static int check(rgbd360_map* m, const Params* params, IcpJob& job) {
        Params p;
        if (params) p = *params;
        else rgbd360_map_default_align_plane_params(m, &p);
        const rgbd360_map_align_params shared = {p.max_dist, p.max_iters, p.eps, p.min_count, p.min_matches};
        if (const int rc = icp_check_params(m, &shared, job.p)) return rc;
        if (p.min_support < 1 || p.min_support > 27) return vmap_fail(m, -1, "min_support must lie in 1 .. 27");
        if (!(p.max_flatness >= 0.f)) return vmap_fail(m, -1, "max_flatness must not be negative");
        job.min_support = p.min_support;
        job.max_flatness = p.max_flatness;
        return 0;
    }
    static int eval_args(rgbd360_map*, const IcpJob& job, const Out& o, Args& a) {
        a = {(unsigned)job.min_support, (double)job.max_flatness, o.normal_r, o.cls};
        return 0;
    }
    static void fill_extra(const double* row, double n, Result* res) {      // (n: the contributing points)
        res->n_unsupported = (long long)row[vmap::kPlUnsupported];
        res->n_nonplanar = (long long)row[vmap::kPlNonplanar];
        res->fitness_point = n > 0.0 ? row[vmap::kPlEE] / n : 0.0;
    }
};
}  // namespace

extern "C" void rgbd360_map_default_align_plane_params(const rgbd360_map* m, rgbd360_map_align_plane_params* p) {
    if (!p) return;
    rgbd360_map_align_params shared;
    rgbd360_map_default_align_params(m, &shared);
    p->max_dist = shared.max_dist;
    p->max_iters = shared.max_iters;
    p->eps = shared.eps;
    p->min_count = shared.min_count;
    p->min_matches = shared.min_matches;
    p->min_support = 5;
    p->max_flatness = 0.05f;
}

extern "C" int rgbd360_map_align_plane_sphere(rgbd360_map* m, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                              const float guess[16], int on_device, const rgbd360_map_align_plane_params* params, float pose_out[16],
                                              rgbd360_map_align_plane_result* result) {
    return icp_by_setting<PlaneIcp>(m, [&](auto M) {
        return icp_align<typename decltype(M)::type>(m, sphere_input(nullptr, 0, depth, depth_step, depth_type, rows, cols, convention, on_device), guess, params,
                                                     pose_out, result);
    });
}
extern "C" int rgbd360_map_align_plane_cloud(rgbd360_map* m, const float* xyz, long long n, const float guess[16], int on_device,
                                             const rgbd360_map_align_plane_params* params, float pose_out[16], rgbd360_map_align_plane_result* result) {
    return icp_by_setting<PlaneIcp>(m, [&](auto M) {
        return icp_align<typename decltype(M)::type>(m, cloud_input(xyz, nullptr, n, on_device), guess, params, pose_out, result);
    });
}

// measurement and tests (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_plane_fit(const double cov[6], double max_flatness, double normal[3], double eigen[2]) {
    if (!cov || !normal) return -1;
    double l0 = 0.0, l1 = 0.0;
    const bool planar = vmap::plane_fit(cov, max_flatness, normal, l0, l1);
    if (eigen) eigen[0] = l0, eigen[1] = l1;
    return planar ? 1 : 0;
}

extern "C" int rgbd360_map_align_plane_eval(rgbd360_map* m, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                            const float* xyz, long long n, const float pose[16], int on_device,
                                            const rgbd360_map_align_plane_params* params, double row[30], long long counters[5], int32_t* key3_dev,
                                            float* d2_dev, double* normal_r_dev, uint8_t* class_dev) {
    if (!m) return -1;
    m->err.clear();
    if (!pose) return vmap_fail(m, -1, "pose must not be null");
    return icp_eval<PlaneIcp>(m, icp_eval_input(depth, depth_step, depth_type, rows, cols, convention, xyz, n, on_device), pose, params, row, counters,
                              {key3_dev, d2_dev, normal_r_dev, class_dev});
}

extern "C" int rgbd360_map_time_align_plane(rgbd360_map* m, const void* depth_dev, size_t depth_step, int depth_type, int rows, int cols, int convention,
                                            const float pose[16], const rgbd360_map_align_plane_params* params, int reps, float avg_us[4], double* probes) {
    if (!m) return -1;
    m->err.clear();
    const MapInput in = sphere_input(nullptr, 0, depth_dev, depth_step, depth_type, rows, cols, convention, 1);
    if (const int rc = vmap_check_timed(m, in, pose, reps, avg_us)) return rc;
    IcpJob job;
    if (const int rc = PlaneIcp::check(m, params, job)) return rc;
    if (const int rc = icp_prepare(m, in, job)) return rc;
    const vmap::Params P = vmap_params(m, pose);
    VmapTimer timer(m, m->s->stream);        // made last
    if (timer.rc) return timer.rc;
    int& rc = timer.rc;
    // the point-to-point kernel first, on the same frame, map and buffers, then the plane kernels, whose state stays behind
    rc = icp_launch_init<PointIcp>(m, pose);
    if (rc == 0) rc = icp_launch_eval<PointIcp>(m, job, P, 1, {});      // once untimed: code and tables loaded
    timer.timed(avg_us[1], reps, [&] { return icp_launch_eval<PointIcp>(m, job, P, 1, {}); });
    if (rc == 0) rc = icp_launch_init<PlaneIcp>(m, pose);
    if (rc == 0) rc = icp_launch_eval<PlaneIcp>(m, job, P, 1, {});
    timer.timed(avg_us[0], reps, [&] { return icp_launch_eval<PlaneIcp>(m, job, P, 1, {}); });
    timer.timed(avg_us[2], reps, [&] { return icp_launch_solve<PlaneIcp>(m, job, 1); });
    if (rc == 0 && probes) rc = icp_read_probes<PlaneIcp>(m, probes);
    if (const int failed = timer.finish(avg_us, 0, reps)) return failed;
    return icp_time_whole<PlaneIcp>(m, job, pose, reps, avg_us[3]);
}
