// rgbd360/PoseGraph.hpp -- the reference's GraphOptimizer (GraphOptimization/GraphOptimizer.h, GraphOptimizer_G2O.cpp: a thin wrapper
// over g2o with Levenberg-Marquardt, a dense linear solver, optimize(10) and vertex 0 fixed) over the device pose-graph optimiser
// (rgbd360_graph_*, ../rgbd360_hip.h).  Header-only, depends on the C ABI and on the PODs of RegisterPhotoICP.hpp; no g2o, no Eigen.
// The call sites it serves, KFsphere_SLAM.cpp:262-265, 542-550, 630, 679-689:
//     optimizer.addVertex(pose);                                              graph.addVertex(pose)            (vertex 0 is fixed)
//     optimizer.addEdge(nearestKF, newKF, relPose, registerer.getInfoMat());  graph.addEdge(nearestKF, newKF, relPose, hessian)
//     optimizer.optimizeGraph(); optimizer.getPoses(Map.vOptimizedPoses);     graph.optimizeGraph(); graph.getPoses(poses)
// relPose is the pose FrameStore::align returns for target `from` and source `to`, the information matrix is rgbd360_result.hessian of the
// same alignment, with no conversion (rgbd360_hip.h).  The optimised poses are what GlobalMap::move takes.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "RegisterPhotoICP.hpp"

namespace rgbd360 {

class PoseGraph {
   public:
    // The graph lives on align's context (device, stream): keep `align` alive and its setters untouched while the graph exists.
    explicit PoseGraph(RegisterPhotoICP& align) {
        rgbd360_ctx* ctx = align.context();
        const int rc = rgbd360_graph_create(ctx, &g_);
        if (rc != 0) throw std::runtime_error("rgbd360_graph_create (" + std::to_string(rc) + "): " + rgbd360_last_error(ctx));
        rgbd360_graph_default_params(&params_);
        rgbd360_graph_default_cov_params(&cov_params_);
    }
    ~PoseGraph() { rgbd360_graph_destroy(g_); }
    PoseGraph(const PoseGraph&) = delete;
    PoseGraph& operator=(const PoseGraph&) = delete;

    // Returns the vertex's index.  The first vertex is fixed (GraphOptimizer_G2O.cpp:46); pass fixed = true to pin another.
    int addVertex(const Mat4f& pose, bool fixed = false) {
        const uint8_t f = fixed || numVertices() == 0 ? 1 : 0;
        return check(rgbd360_graph_add_vertices(g_, 1, pose.m, &f), "rgbd360_graph_add_vertices");
    }
    // relativePose: frame `to` in frame `from`; informationMatrix: the 6x6 Hessian of that alignment (translation first).
    void addEdge(int from, int to, const Mat4f& relativePose, const Mat6f& informationMatrix) {
        check(rgbd360_graph_add_edges(g_, 1, &from, &to, relativePose.m, informationMatrix.m), "rgbd360_graph_add_edges");
    }
    void addEdge(int from, int to, const Mat4f& relativePose) {      // identity information
        check(rgbd360_graph_add_edges(g_, 1, &from, &to, relativePose.m, nullptr), "rgbd360_graph_add_edges");
    }
    // The Hessian of an alignment result as the information matrix of its edge
    static Mat6f information(const rgbd360_result& r) {
        Mat6f I;
        for (int k = 0; k < 36; ++k) I.m[k] = r.hessian[k];
        return I;
    }
    int lastEdge() const { return numEdges() - 1; }      // the index of the edge addEdge added last
    // g2o's edge->setRobustKernel: kind is RGBD360_GRAPH_ROBUST_NONE / HUBER / CAUCHY / GEMAN_MCCLURE, delta > 0 in units of sqrt(chi2)
    void setRobustKernel(int edge, int kind, double delta) {
        check(rgbd360_graph_set_edge_robust(g_, edge, 1, &kind, &delta), "rgbd360_graph_set_edge_robust");
    }
    // A disabled edge adds nothing to the cost or the normal equations; its chi2 is still reported by edgeWeights.
    void setEdgeEnabled(int edge, bool enabled) {
        const uint8_t f = enabled ? 1 : 0;
        check(rgbd360_graph_set_edge_enabled(g_, edge, 1, &f), "rgbd360_graph_set_edge_enabled");
    }
    // Per edge at the current poses: s = r^T Omega r, the robust rho and the weight w (0 for a disabled edge).  Returns the cost.
    double edgeWeights(std::vector<double>& w, std::vector<double>* s = nullptr, std::vector<double>* rho = nullptr) {
        const size_t n = (size_t)numEdges();
        double cost = 0.0;
        w.resize(n);
        if (s) s->resize(n);
        if (rho) rho->resize(n);
        check(rgbd360_graph_edge_weights(g_, &cost, s && n ? s->data() : nullptr, rho && n ? rho->data() : nullptr, n ? w.data() : nullptr),
              "rgbd360_graph_edge_weights");
        return cost;
    }
    void setPose(int vertex, const Mat4f& pose) { check(rgbd360_graph_set_poses(g_, vertex, 1, pose.m), "rgbd360_graph_set_poses"); }
    void setFixed(int vertex, bool fixed) {
        const uint8_t f = fixed ? 1 : 0;
        check(rgbd360_graph_set_fixed(g_, vertex, 1, &f), "rgbd360_graph_set_fixed");
    }
    int numVertices() const { return rgbd360_graph_n_vertices(g_); }
    int numEdges() const { return rgbd360_graph_n_edges(g_); }
    void clear() { check(rgbd360_graph_clear(g_), "rgbd360_graph_clear"); }

    rgbd360_graph_params& params() { return params_; }      // max_iters 10 (the reference's optimize(10)), ...
    // true: RGBD360_OK; false: RGBD360_ILL_POSED (result().status).  The poses are the last accepted ones either way.
    bool optimizeGraph() {
        const int rc = check(rgbd360_graph_optimize(g_, &params_, &result_), "rgbd360_graph_optimize");
        return rc == RGBD360_OK;
    }
    void getPoses(std::vector<Mat4f>& poses) {
        poses.resize((size_t)numVertices());
        if (!poses.empty()) check(rgbd360_graph_get_poses(g_, 0, (int)poses.size(), poses[0].m), "rgbd360_graph_get_poses");
    }
    const rgbd360_graph_result& result() const { return result_; }
    double chi2() {
        double c = 0.0;
        check(rgbd360_graph_chi2(g_, &c, nullptr), "rgbd360_graph_chi2");
        return c;
    }
    std::vector<rgbd360_graph_iteration> trace() {
        int n = 0;
        check(rgbd360_graph_get_trace(g_, 0, &n, nullptr), "rgbd360_graph_get_trace");
        std::vector<rgbd360_graph_iteration> t((size_t)n);
        if (n) check(rgbd360_graph_get_trace(g_, n, nullptr, t.data()), "rgbd360_graph_get_trace");
        return t;
    }
    // g2o's computeMarginals.  Sigma_vv of the vertices, 6x6 blocks of the inverse of the Gauss-Newton matrix at the current poses in the
    // update tangent (translation first); covResult() holds the status, the per-call counts and the variance factor cost / dof by which a
    // caller scales a covariance before gating on it (alignment Hessians are overconfident information matrices, rgbd360_hip.h).
    // Returns one Mat6d per query; throws on bad arguments only: RGBD360_ILL_POSED and RGBD360_NOT_CONVERGED are covResult().status.
    struct Mat6d {
        double m[36];      // column-major
        double operator()(int r, int c) const { return m[c * 6 + r]; }
    };
    rgbd360_graph_cov_params& covParams() { return cov_params_; }      // cg_max_iters 1000, cg_tol 1e-10
    std::vector<Mat6d> marginals(const std::vector<int>& vertices) {
        std::vector<Mat6d> cov(vertices.size());
        check(rgbd360_graph_marginals(g_, (int)vertices.size(), vertices.data(), &cov_params_, cov.empty() ? nullptr : cov[0].m, nullptr, nullptr,
                                      &cov_result_), "rgbd360_graph_marginals");
        return cov;
    }
    // C_ij of the pairs (from[k], to[k]): the covariance of the left perturbation of T_i^-1 T_j, commensurate with the inverse information
    // matrix of an edge (i, j, Z)
    std::vector<Mat6d> relativeCovariances(const std::vector<int>& from, const std::vector<int>& to) {
        if (from.size() != to.size()) throw std::runtime_error("PoseGraph::relativeCovariances: one from and one to per pair");
        std::vector<Mat6d> cov(to.size());
        check(rgbd360_graph_relative_covariances(g_, (int)to.size(), from.data(), to.data(), &cov_params_, cov.empty() ? nullptr : cov[0].m, nullptr,
                                                 nullptr, &cov_result_), "rgbd360_graph_relative_covariances");
        return cov;
    }
    const rgbd360_graph_cov_result& covResult() const { return cov_result_; }
    rgbd360_graph* handle() { return g_; }

   private:
    int check(int rc, const char* what) {
        if (rc < 0) throw std::runtime_error(std::string(what) + " (" + std::to_string(rc) + "): " + rgbd360_graph_last_error(g_));
        return rc;
    }
    rgbd360_graph* g_ = nullptr;
    rgbd360_graph_params params_{};
    rgbd360_graph_result result_{};
    rgbd360_graph_cov_params cov_params_{};
    rgbd360_graph_cov_result cov_result_{};
};

}  // namespace rgbd360
