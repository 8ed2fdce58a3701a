// map_align_robust.h -- robust kernels of the alignments against the resident voxel map: the setting a map keeps per method, what an
// alignment reports of it, one robust evaluation at a pose, and the A/B measurement.  Part of the Frame360 translation unit, behind the
// four methods (map_align.h, map_align_plane.h, map_align_gicp.h, map_align_colour.h) and the batch (map_align_batch.h).
//
// Definition (include/rgbd360_hip.h, "robust kernels of the alignments against the map"; tests/map_align_robust_reference.py
// restates it in numpy).  The device side is not here: a method's tail is written over a weight policy (map_align.h: UnitWeight, the
// quadratic cost, and RobustWeight, w and rho from gn::robust_rho_w -- the pose graph's text), vmap::Robust<M> is M's row with the count of
// contributing points and of down-weighted points behind it, and the kernels are the templates every method uses:
//   k_vmap_eval<Robust<M>, SRC>, k_vmap_icp_solve<Robust<M>>                 M = Point, Plane, Gicp, Colour
//   k_vmap_eval_batch<Robust<M>, SRC>, k_vmap_icp_solve_batch<Robust<M>>     M = Point, Plane (the two methods the batch has)
// The kind is a runtime value, uniform over a launch: one instantiation per method.  The host side is RobustIcp<B> and icp_by_setting
// (map_align.h): an entry asks the map's setting once and runs B or RobustIcp<B> through the one driver.  With RGBD360_MAP_ROBUST_NONE
// nothing of this is launched.  Not honoured by rig_calib.h, depth_train.h and map_planes.h, which keep the quadratic kernels.
#pragma once

namespace vmap {
static_assert(Robust<PlaneMethod>::kWords <= kIcpMaxWords && Robust<GicpMethod>::kWords <= kIcpMaxWords && Robust<ColourMethod>::kWords <= kIcpMaxWords,
              "the buffers of a map hold the widest row");
static_assert(RGBD360_MAP_ROBUST_HUBER == RGBD360_GRAPH_ROBUST_HUBER && RGBD360_MAP_ROBUST_CAUCHY == RGBD360_GRAPH_ROBUST_CAUCHY &&
                  RGBD360_MAP_ROBUST_GEMAN_MCCLURE == RGBD360_GRAPH_ROBUST_GEMAN_MCCLURE && RGBD360_MAP_ROBUST_NONE == RGBD360_GRAPH_ROBUST_NONE,
              "gn::robust_rho_w takes the graph's kinds");
}  // namespace vmap

namespace {

// f(IcpTag<B>) for the method's host description B; -1 for an unknown method
template <class F>
int robust_with_method(rgbd360_map* m, int method, F&& f) {
    switch (method) {
    case RGBD360_MAP_METHOD_POINT: return f(IcpTag<PointIcp>{});
    case RGBD360_MAP_METHOD_PLANE: return f(IcpTag<PlaneIcp>{});
    case RGBD360_MAP_METHOD_GICP: return f(IcpTag<GicpIcp>{});
    case RGBD360_MAP_METHOD_COLOUR: return f(IcpTag<ColourIcp>{});
    }
    return vmap_fail(m, -1, "method must be one of RGBD360_MAP_METHOD_POINT / _PLANE / _GICP / _COLOUR");
}

// one robust evaluation of method B at `pose`: icp_eval's route with the whole row and w per point as its outputs
template <class B>
int robust_eval(rgbd360_map* m, const MapInput& in, const float pose[16], const typename B::Params* params, double* row, double* w_dev) {
    using M = RobustIcp<B>;
    IcpJob job;
    if (const int rc = M::check(m, params, job)) return rc;
    if (job.robust_kind == RGBD360_MAP_ROBUST_NONE) return vmap_fail(m, -1, "the method has no robust kernel set (rgbd360_map_set_align_robust)");
    const int chk = vmap_check(m, in, true);
    if (chk < 0) return chk;
    for (int k = 0; k < vmap::kIcpMaxWords && row; ++k) row[k] = 0.0;
    if (chk != 0) return 0;
    job.p.max_iters = 0;
    if (const int rc = icp_prepare(m, in, job)) return rc;
    typename M::Out out;
    out.w = w_dev;
    if (const int rc = icp_enqueue<M>(m, job, pose, 0, out)) return rc;
    HIPC(m, hipStreamSynchronize(m->s->stream));
    const IcpState<M>& st = icp_host_state<M>(m);
    for (int k = 0; k < M::kWords && row; ++k) row[k] = st.row[k];
    return 0;
}

// the evaluation, the solve and a whole alignment of method B in both forms on one prepared job, alternating (rgbd360_map_time_align_robust)
template <class B>
int robust_time(rgbd360_map* m, const MapInput& in, const float pose[16], const typename B::Params* params, int reps, float avg_us[6]) {
    using M = RobustIcp<B>;
    if (const int rc = vmap_check_timed(m, in, pose, reps, avg_us)) return rc;
    IcpJob job;
    if (const int rc = M::check(m, params, job)) return rc;
    if (job.robust_kind == RGBD360_MAP_ROBUST_NONE) return vmap_fail(m, -1, "the method has no robust kernel set (rgbd360_map_set_align_robust)");
    if (const int rc = icp_prepare(m, in, job)) return rc;
    const vmap::Params P = vmap_params(m, pose);
    {
        VmapTimer timer(m, m->s->stream);        // made last
        if (timer.rc) return timer.rc;
        int& rc = timer.rc;
        // once untimed in either form: code and tables loaded, the layers built; then pairs of launches, the quadratic form first
        rc = icp_launch_init<B>(m, pose);
        if (rc == 0) rc = icp_launch_eval<B>(m, job, P, 1, {});
        if (rc == 0) rc = icp_launch_init<M>(m, pose);
        if (rc == 0) rc = icp_launch_eval<M>(m, job, P, 1, {});
        for (int r = 0; r < reps; ++r) {
            if (rc == 0) rc = icp_launch_init<B>(m, pose);
            timer.add(1, [&] { return icp_launch_eval<B>(m, job, P, 1, {}); });
            timer.add(3, [&] { return icp_launch_solve<B>(m, job, 1); });
            if (rc == 0) rc = icp_launch_init<M>(m, pose);
            timer.add(0, [&] { return icp_launch_eval<M>(m, job, P, 1, {}); });
            timer.add(2, [&] { return icp_launch_solve<M>(m, job, 1); });
        }
        if (const int failed = timer.finish(avg_us, 4, reps)) return failed;
    }
    if (const int rc = icp_time_whole<M>(m, job, pose, reps, avg_us[4])) return rc;
    return icp_time_whole<B>(m, job, pose, reps, avg_us[5]);
}

// the input of the robust diag entries: a method's own input forms (a cloud's normals: generalized ICP; colours: coloured ICP)
MapInput robust_input(int method, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step, int depth_type, int rows, int cols, int convention,
                      const float* xyz, const float* normal, const uint8_t* rgb3, long long n, int on_device) {
    MapInput in = icp_eval_input(depth, depth_step, depth_type, rows, cols, convention, xyz, n, on_device);
    if (method == RGBD360_MAP_METHOD_GICP && in.cloud && n > 0) in.normal = normal;
    if (method == RGBD360_MAP_METHOD_COLOUR) {
        in.rgb = in.cloud ? rgb3 : rgb;
        in.rgb_step = in.cloud ? 0 : rgb_step;
    }
    return in;
}
}  // namespace

extern "C" int rgbd360_map_set_align_robust(rgbd360_map* m, int method, const rgbd360_map_robust* robust) {
    if (!m) return -1;
    m->err.clear();
    if (m->parent) return vmap_fail(m, -1, "a level of a map pyramid follows its root's robust setting: set it there");
    if (method < RGBD360_MAP_METHOD_POINT || method > RGBD360_MAP_METHOD_COLOUR)
        return vmap_fail(m, -1, "method must be one of RGBD360_MAP_METHOD_POINT / _PLANE / _GICP / _COLOUR");
    if (!robust) return vmap_fail(m, -1, "robust must not be null");
    if (robust->kind < RGBD360_MAP_ROBUST_NONE || robust->kind > RGBD360_MAP_ROBUST_GEMAN_MCCLURE)
        return vmap_fail(m, -1, "kind must be one of RGBD360_MAP_ROBUST_NONE / _HUBER / _CAUCHY / _GEMAN_MCCLURE");
    if (robust->kind != RGBD360_MAP_ROBUST_NONE && !(robust->delta > 0.0 && std::isfinite(robust->delta)))
        return vmap_fail(m, -1, "delta must be finite and positive");
    m->robust[method] = {robust->kind, robust->scale_with_level != 0 ? 1 : 0, robust->delta};
    return 0;
}

extern "C" int rgbd360_map_get_align_robust(rgbd360_map* m, int method, rgbd360_map_robust* robust) {
    if (!m) return -1;
    m->err.clear();
    if (method < RGBD360_MAP_METHOD_POINT || method > RGBD360_MAP_METHOD_COLOUR)
        return vmap_fail(m, -1, "method must be one of RGBD360_MAP_METHOD_POINT / _PLANE / _GICP / _COLOUR");
    if (!robust) return vmap_fail(m, -1, "robust must not be null");
    *robust = icp_robust_setting(m, method);
    return 0;
}

extern "C" int rgbd360_map_align_robust_info(rgbd360_map* m, rgbd360_map_robust_info* info) {
    if (!m) return -1;
    m->err.clear();
    if (!info) return vmap_fail(m, -1, "info must not be null");
    *info = m->a_robust;
    return 0;
}

extern "C" int rgbd360_map_align_batch_robust_info(rgbd360_map* m, int job, rgbd360_map_robust_info* info) {
    if (!m) return -1;
    m->err.clear();
    if (!info) return vmap_fail(m, -1, "info must not be null");
    if (job < 0 || job >= (int)m->b_robust.size()) return vmap_fail(m, -1, "no such job in the map's last batch");
    *info = m->b_robust[(size_t)job];
    return 0;
}

// measurement and tests (rgbd360_hip_diag.h)
extern "C" int rgbd360_map_align_robust_eval(rgbd360_map* m, int method, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t depth_step,
                                             int depth_type, int rows, int cols, int convention, const float* xyz, const float* normal, const uint8_t* rgb3,
                                             long long n, const float pose[16], int on_device, const void* params, double row[40], double* w_dev) {
    if (!m) return -1;
    m->err.clear();
    if (!pose) return vmap_fail(m, -1, "pose must not be null");
    return robust_with_method(m, method, [&](auto B) {
        using Icp = typename decltype(B)::type;
        const MapInput in = robust_input(method, rgb, rgb_step, depth, depth_step, depth_type, rows, cols, convention, xyz, normal, rgb3, n, on_device);
        if (method == RGBD360_MAP_METHOD_COLOUR && colour_missing(in)) return vmap_fail(m, -1, "coloured ICP needs the source's colours");
        return robust_eval<Icp>(m, in, pose, static_cast<const typename Icp::Params*>(params), row, w_dev);
    });
}

extern "C" int rgbd360_map_time_align_robust(rgbd360_map* m, int method, const uint8_t* rgb_dev, size_t rgb_step, const void* depth_dev, size_t depth_step,
                                             int depth_type, int rows, int cols, int convention, const float pose[16], const void* params, int reps,
                                             float avg_us[6]) {
    if (!m) return -1;
    m->err.clear();
    return robust_with_method(m, method, [&](auto B) {
        using Icp = typename decltype(B)::type;
        const MapInput in = robust_input(method, rgb_dev, rgb_step, depth_dev, depth_step, depth_type, rows, cols, convention, nullptr, nullptr, nullptr, 0, 1);
        if (method == RGBD360_MAP_METHOD_COLOUR && colour_missing(in)) return vmap_fail(m, -1, "coloured ICP needs the frame's colours");
        return robust_time<Icp>(m, in, pose, static_cast<const typename Icp::Params*>(params), reps, avg_us);
    });
}
