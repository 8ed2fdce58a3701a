// map_align_colour.h -- coloured ICP (Park, Zhou, Koltun: Colored Point Cloud Registration Revisited; Open3D's registration_colored_icp)
// of a posed sphere frame, or of a cloud with colours, against the resident voxel map: the geometric point-to-plane term on the map's
// resident normals joined with a photometric term on the map's resident intensity gradients, which observes the pose along the surfaces
// where geometry alone slides (a corridor, a floor and one wall).  Part of the Frame360 translation unit, behind map_colour.h: the two
// layers are the map's (normals_layer, colour_layer), the match, the row sum and the loop are map_align.h's.  Here: the evaluation's tail
// (ColourTail), the row's description (ColourMethod) and the host's (ColourIcp).
//
// Definition (include/rgbd360_hip.h, "coloured ICP against the map"; tests/map_colour_reference.py restates it in numpy).
// Per source point at the current pose, float64 with + - x / only, no contraction:
//   1 match: steps 1-4 of map_align.h, bit for bit (vmap::classify, vmap::search27<NoSupport>, kept iff d2 <= max_dist^2); e = the
//     float32 w - c of the match, widened.
//   2 class: a kept match whose voxel is not OK in the normal layer is dropped and counted (n_no_normal).  Otherwise n = the doubles of its
//     float32 normal, I and d those of its record in the colour layer (d = 0 with status NO_GRADIENT, counted in n_no_gradient; the point
//     stays), I_q = the source point's intensity (vmap::intensity64 of its three bytes).
//   3 residuals: r_G = (n_x e_x + n_y e_y) + n_z e_z; p_k = e_k - r_G n_k; r_C = (I + ((d_x p_x + d_y p_y) + d_z p_z)) - I_q.
//   4 rows (left perturbation): J_G = [n | w x n], J_C = [d | w x d] (d is tangent: the projection's derivative drops out).
//   5 sums, l = (double)lambda_geometric, c = 1.0 - l, sG = l J_G, sC = c J_C: H_ab += sG_a J_G,b + sC_a J_C,b (a <= b, 21 terms),
//     g_a += sG_a r_G + sC_a r_C, cost += l (r_G r_G) + c (r_C r_C), also sum r_G r_G and sum r_C r_C.
//   6 38 float64 words per workgroup row (kColourWords), the rows added in ascending order; no floating-point atomics.
//   7 H and g straight from the row, cast to float32, gn::step with lambda 0, the stop tests and statuses of map_align.h.
//
//   k_vmap_eval<ColourMethod, SRC>  map_align.h's evaluation on this row, the table and both layers read-only.  Per kept point two
//                        independent 16-byte reads at the matched slot (the slot rides in search27's Match) and, beside them, the
//                        source point's three colour bytes (ColourTail).
//   k_vmap_icp_solve<ColourMethod>  map_align.h's solve kernel on this row.
#pragma once

namespace vmap {

// a partial row: n, the 21 upper-triangle terms of H (row by row), g (6), the cost, sum r_G r_G, sum r_C r_C, then the counters n_valid,
// n_box_rejected, n_out_of_range, n_no_normal, n_no_gradient, probes, points searched (all doubles: exact integers)
constexpr int kColourWords = 38;
enum { kCoN = 0, kCoH = 1, kCoG = 22, kCoCost = 28, kCoGG = 29, kCoCC = 30, kCoValid = 31, kCoBox = 32, kCoRange = 33, kCoNoNormal = 34, kCoNoGradient = 35,
       kCoProbes = 36, kCoSearched = 37 };
enum { kColourKept = 1, kColourNoNormal = 2, kColourNoGradient = 4 };      // the bits of a point's class byte

// what the evaluation takes beyond EvalCommon: the map's two layers by slot.  The per-point outputs (tests; either may be null): res_out
// two doubles per point (r_G and r_C; zeros unless the point contributes), class_out one byte per point: kColourKept a kept match, |
// kColourNoNormal it was dropped, | kColourNoGradient it contributes with d = 0 (key3: the key of the kept MATCH whatever the class).
struct ColourArgs {
    const uint4* normals;
    const uint4* colours;
    float lambda_geometric;
    double* res_out;
    uint8_t* class_out;
};
// coloured ICP's tail: steps 2-5 of the definition; W: the weight policy (map_align.h), one joint weight for both terms
template <class W>
struct ColourTailT {
    const uint8_t* crow;             // the colours by the point's index, as k_vmap_insert takes them (the image's row pointer moved back by the row's first index)
    double acc[kCoCC + 1];           // n, H (21), g (6), the cost, r_G r_G, r_C r_C
    W wt;
    unsigned n_no_normal = 0, n_no_gradient = 0;
    int pclass;                      // of the point added last, for store(): its class and residuals
    double rg, rc;
    __device__ __forceinline__ ColourTailT() {
#pragma unroll
        for (int q = 0; q <= kCoCC; ++q) acc[q] = 0.0;
    }
    template <int SRC>
    __device__ __forceinline__ void begin(const Source& src, unsigned by) {
        crow = SRC == 0 ? src.rgb + (size_t)by * src.rgb_step - 3 * (size_t)by * src.cols : src.rgb;
    }
    template <class Args>
    __device__ __forceinline__ void add(long long index, const float*, const float w[3], const Match<NoSupport>& mt, bool kept, const Args& args) {
#pragma clang fp contract(off)
        const double lam = (double)args.lambda_geometric, oml = 1.0 - lam;
        wt.clear();
        pclass = 0;
        rg = 0.0, rc = 0.0;
        if (kept) {
            const uint4 nw = args.normals[mt.best_slot], cw = args.colours[mt.best_slot];      // the two reads and the point's three bytes: none waits for another
            const uint8_t* c = crow + 3 * (size_t)index;
            const unsigned c0 = c[0], c1 = c[1], c2 = c[2];
            const NormalRec nr = normal_unpack(nw);
            const ColourRec cr = colour_unpack(cw);
            if (nr.status != kClassKept) {
                pclass = kColourKept | kColourNoNormal;
                n_no_normal += 1u;
            } else {
                pclass = kColourKept | (cr.status == kColOk ? 0 : kColourNoGradient);
                n_no_gradient += cr.status == kColOk ? 0u : 1u;
                const double nx = (double)nr.n[0], ny = (double)nr.n[1], nz = (double)nr.n[2];
                const double dx = (double)cr.d[0], dy = (double)cr.d[1], dz = (double)cr.d[2];
                const double wx = w[0], wy = w[1], wz = w[2], ex = mt.be[0], ey = mt.be[1], ez = mt.be[2];
                rg = (nx * ex + ny * ey) + nz * ez;
                const double px = ex - rg * nx, py = ey - rg * ny, pz = ez - rg * nz;
                rc = ((double)cr.I + ((dx * px + dy * py) + dz * pz)) - intensity64(c0, c1, c2, 1ull);
                const double JG[6] = {nx, ny, nz, wy * nz - wz * ny, wz * nx - wx * nz, wx * ny - wy * nx};
                const double JC[6] = {dx, dy, dz, wy * dz - wz * dy, wz * dx - wx * dz, wx * dy - wy * dx};
                const auto s = [&] { return lam * (rg * rg) + oml * (rc * rc); };
                wt.set(s, args);
                acc[kCoN] += wt(1.0);
                int h = kCoH;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const double sg = lam * JG[a], sc = oml * JC[a];
#pragma unroll
                    for (int b = a; b < 6; ++b) acc[h++] += wt(sg * JG[b] + sc * JC[b]);
                    acc[kCoG + a] += wt(sg * rg + sc * rc);
                }
                const double gg = rg * rg, cc = rc * rc;
                acc[kCoCost] += wt.rho(s);
                acc[kCoGG] += gg;
                acc[kCoCC] += cc;
            }
        }
    }
    template <class Args>
    __device__ __forceinline__ void store(long long index, const Args& args) const {
        wt.store(index, args);
        if (args.res_out) {
            args.res_out[2 * index] = rg;
            args.res_out[2 * index + 1] = rc;
        }
        if (args.class_out) args.class_out[index] = (uint8_t)pclass;
    }
    __device__ __forceinline__ void row(double* out) const {
#pragma unroll
        for (int q = 0; q <= kCoCC; ++q) out[q] = acc[q];
        out[kCoNoNormal] = (double)n_no_normal;
        out[kCoNoGradient] = (double)n_no_gradient;
        wt.row(out + kColourWords);
    }
};
using ColourTail = ColourTailT<UnitWeight>;

struct ColourMethod {
    static constexpr int kWords = kColourWords, kN = kCoN, kSumSq = kCoCost, kCounters = kCoValid, kProbes = kCoProbes, kSearched = kCoSearched;
    __host__ __device__ static void assemble(const double* s, float* H, float* g) { plane_assemble(s, H, g); }      // (the plane row's places)
    using Support = NoSupport;
    using Args = ColourArgs;
    using Tail = ColourTail;
    template <class W>
    using TailT = ColourTailT<W>;
};
static_assert(kCoValid + 1 == kCoBox && kCoValid + 2 == kCoRange, "the three counters of every method lead the row's counters");
static_assert(kCoH == kPlH && kCoG == kPlG, "H and g lie where plane_assemble reads them");
static_assert(kColourWords <= kIcpMaxWords, "the buffers of a map hold the widest row");

}  // namespace vmap

namespace {

static_assert(sizeof(rgbd360_map_align_colour_params) == 48 && sizeof(rgbd360_map_align_colour_result) == 256, "the header's structs");

struct ColourIcp : vmap::ColourMethod {
    using Row = vmap::ColourMethod;
    static constexpr int kMethod = RGBD360_MAP_METHOD_COLOUR;
    using Params = rgbd360_map_align_colour_params;
    using Result = rgbd360_map_align_colour_result;
    struct Out {
        int32_t* key3 = nullptr;
        float* d2 = nullptr;
        double* residuals = nullptr;
        uint8_t* cls = nullptr;
    };
    static int check(rgbd360_map* m, const Params* params, IcpJob& job) {
        Params p;
        if (params) p = *params;
        else rgbd360_map_default_align_colour_params(m, &p);
        const rgbd360_map_align_params shared = {p.max_dist, p.max_iters, p.eps, p.min_count, p.min_matches};
        if (const int rc = icp_check_params(m, &shared, job.p)) return rc;
        if (!(p.lambda_geometric >= 0.f && p.lambda_geometric <= 1.f)) return vmap_fail(m, -1, "lambda_geometric must lie in [0, 1]");
        const rgbd360_map_colour_params cp = {p.min_count, p.min_support, p.max_flatness, p.min_gradient_support, p.min_spread};
        rgbd360_map_colour_params checked;
        if (const int rc = colour_check_params(m, &cp, checked)) return rc;
        job.min_support = p.min_support;
        job.max_flatness = p.max_flatness;
        job.lambda_geometric = p.lambda_geometric;
        job.min_gradient_support = p.min_gradient_support;
        job.min_spread = p.min_spread;
        return 0;
    }
    // the map's two layers under this call's parameters, built or reused (a comparison on the host while the map's revision and the
    // parameters stand), ahead of the kernel on the stream
    static int eval_args(rgbd360_map* m, const IcpJob& job, const Out& o, Args& a) {
        if (!job.src.rgb) return vmap_fail(m, -1, "coloured ICP needs the source's colours");
        const uint4 *normals = nullptr, *colours = nullptr;
        if (m->n_voxels > 0) {       // (an empty map matches nothing: the layers are never read)
            const rgbd360_map_colour_params cp = {job.p.min_count, job.min_support, job.max_flatness, job.min_gradient_support, job.min_spread};
            if (const int rc = colour_layer(m, cp)) return rc;
            normals = m->nm_layer.get();
            colours = m->cl_layer.get();
        }
        a = {normals, colours, job.lambda_geometric, o.residuals, o.cls};
        return 0;
    }
    static void fill_extra(const double* row, double n, Result* res) {      // (n: the contributing points)
        res->n_no_normal = (long long)row[vmap::kCoNoNormal];
        res->n_no_gradient = (long long)row[vmap::kCoNoGradient];
        res->rms_geometric = n > 0.0 ? sqrt(row[vmap::kCoGG] / n) : 0.0;
        res->rms_colour = n > 0.0 ? sqrt(row[vmap::kCoCC] / n) : 0.0;
    }
};

// what the entries refuse before anything else is looked at: an input that has points but no colours
bool colour_missing(const MapInput& in) { return !in.rgb && (in.cloud ? in.n > 0 : in.depth != nullptr); }
}  // namespace

extern "C" void rgbd360_map_default_align_colour_params(const rgbd360_map* m, rgbd360_map_align_colour_params* p) {
    if (!p) return;
    rgbd360_map_align_plane_params plane;
    rgbd360_map_default_align_plane_params(m, &plane);
    rgbd360_map_colour_params colour;
    rgbd360_map_default_colour_params(m, &colour);
    memset(p, 0, sizeof(*p));
    p->max_dist = plane.max_dist;
    p->max_iters = plane.max_iters;
    p->eps = plane.eps;
    p->min_count = plane.min_count;
    p->min_matches = plane.min_matches;
    p->lambda_geometric = 0.968f;        // Open3D's
    p->min_support = plane.min_support;
    p->max_flatness = plane.max_flatness;
    p->min_gradient_support = colour.min_gradient_support;
    p->min_spread = colour.min_spread;
}

extern "C" int rgbd360_map_align_colour_sphere(rgbd360_map* m, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type,
                                               int rows, int cols, int convention, const float guess[16], int on_device,
                                               const rgbd360_map_align_colour_params* params, float pose_out[16], rgbd360_map_align_colour_result* result) {
    if (!m) return -1;
    const MapInput in = sphere_input(rgb, rgb_step, depth, depth_step, depth_type, rows, cols, convention, on_device);
    if (colour_missing(in)) return vmap_fail(m, -1, "coloured ICP needs the frame's colours");
    return icp_by_setting<ColourIcp>(m, [&](auto M) { return icp_align<typename decltype(M)::type>(m, in, guess, params, pose_out, result); });
}
extern "C" int rgbd360_map_align_colour_cloud(rgbd360_map* m, const float* xyz, const uint8_t* rgb3, long long n, const float guess[16], int on_device,
                                              const rgbd360_map_align_colour_params* params, float pose_out[16], rgbd360_map_align_colour_result* result) {
    if (!m) return -1;
    const MapInput in = cloud_input(xyz, rgb3, n, on_device);
    if (colour_missing(in)) return vmap_fail(m, -1, "coloured ICP needs the cloud's colours");
    return icp_by_setting<ColourIcp>(m, [&](auto M) { return icp_align<typename decltype(M)::type>(m, in, guess, params, pose_out, result); });
}

// measurement and tests (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_align_colour_eval(rgbd360_map* m, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type,
                                             int rows, int cols, int convention, const float* xyz, const uint8_t* rgb3, long long n, const float pose[16],
                                             int on_device, const rgbd360_map_align_colour_params* params, double row[31], long long counters[5],
                                             int32_t* key3_dev, float* d2_dev, double* residuals_dev, uint8_t* class_dev) {
    if (!m) return -1;
    m->err.clear();
    if (!pose) return vmap_fail(m, -1, "pose must not be null");
    MapInput in = icp_eval_input(depth, depth_step, depth_type, rows, cols, convention, xyz, n, on_device);
    in.rgb = in.cloud ? rgb3 : rgb;
    in.rgb_step = in.cloud ? 0 : rgb_step;
    if (colour_missing(in)) {        // (as icp_eval leaves a refused input: a cloud's outputs zeroed, an image's untouched)
        for (int k = 0; in.cloud && row && k < vmap::kCoValid; ++k) row[k] = 0.0;
        for (int k = 0; in.cloud && counters && k < 5; ++k) counters[k] = 0;
        return vmap_fail(m, -1, "coloured ICP needs the source's colours");
    }
    return icp_eval<ColourIcp>(m, in, pose, params, row, counters, {key3_dev, d2_dev, residuals_dev, class_dev});
}

extern "C" int rgbd360_map_time_align_colour(rgbd360_map* m, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev, size_t depth_step, int depth_type,
                                             int rows, int cols, int convention, const float pose[16], const rgbd360_map_align_colour_params* params,
                                             int reps, float avg_us[4], double* probes) {
    if (!m) return -1;
    m->err.clear();
    const MapInput in = sphere_input(rgb_dev, rgb_step, depth_dev, depth_step, depth_type, rows, cols, convention, 1);
    if (colour_missing(in)) return vmap_fail(m, -1, "coloured ICP needs the frame's colours");
    if (const int rc = vmap_check_timed(m, in, pose, reps, avg_us)) return rc;
    IcpJob job;
    if (const int rc = ColourIcp::check(m, params, job)) return rc;
    job.epsilon = 1e-3f;             // generalized ICP's defaults on the shared parameters, for the kernel timed beside this one
    job.use_target_normals = 1;
    if (const int rc = icp_prepare(m, in, job)) return rc;
    const vmap::Params P = vmap_params(m, pose);
    VmapTimer timer(m, m->s->stream);        // made last
    if (timer.rc) return timer.rc;
    int& rc = timer.rc;
    // generalized ICP's kernel first, on the same frame, map and buffers, then this method's, whose state stays behind
    rc = icp_launch_init<GicpIcp>(m, pose);
    if (rc == 0) rc = icp_launch_eval<GicpIcp>(m, job, P, 1, {});       // once untimed: code and tables loaded, the normal layer built
    timer.timed(avg_us[1], reps, [&] { return icp_launch_eval<GicpIcp>(m, job, P, 1, {}); });
    if (rc == 0) rc = icp_launch_init<ColourIcp>(m, pose);
    if (rc == 0) rc = icp_launch_eval<ColourIcp>(m, job, P, 1, {});     // (and the colour layer built)
    timer.timed(avg_us[0], reps, [&] { return icp_launch_eval<ColourIcp>(m, job, P, 1, {}); });
    timer.timed(avg_us[2], reps, [&] { return icp_launch_solve<ColourIcp>(m, job, 1); });
    if (rc == 0 && probes) rc = icp_read_probes<ColourIcp>(m, probes);
    if (const int failed = timer.finish(avg_us, 0, reps)) return failed;
    return icp_time_whole<ColourIcp>(m, job, pose, reps, avg_us[3]);
}
