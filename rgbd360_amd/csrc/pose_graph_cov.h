// pose_graph_cov.h -- marginal and relative pose covariances of the pose graph (rgbd360_graph_marginals, rgbd360_graph_relative_covariances,
// include/rgbd360_hip.h).  Included by rgbd360_api.hip behind pose_graph.h, whose kernels it reuses unchanged: the
// linearisation and the assembly at lambda = 0 (k_pg_edges<linearise>, k_pg_assemble: W, D, Minv = D^-1), and the block-Jacobi PCG
// (k_pg_cg_*) on a view of its own columns, without a damping vector and outside the optimiser's loop (it = -1).
//
// A 6x6 block of H^-1 is B^T X with H X = B, B = E_v (a marginal) or E_j - E_i (a relative covariance): six right-hand sides per query.
// Up to kCovChunk queries, 6 columns each, run in lock step; a batch is a fixed list of launches, enqueued blindly by the host, and one
// stream synchronisation:
//   k_pgc_init              per (vertex, column): res = the column of B, z = Minv res, p = z, x = 0 -> r.z rows; the column's state words
//   cg_max_iters times      k_pg_cg_edge, k_pg_cg_gather, k_pg_cg_update, k_pg_cg_dir (pose_graph.h)
//   k_pgc_finish            per query: M = B^T X, Ad(T_i^-1) M Ad(T_i^-1)^T for a relative covariance, (M + M^T) / 2; iterations, residual, flags
// Every column has its own rows ([column][workgroup]), alpha, beta and stop word; blockIdx.y is the column, so a column's arithmetic is that
// of a batch which holds it alone, and a finished column is frozen (its launches return on its stop word).
// The edge product has two work mappings with the same bits: one thread per (edge, column), which reads the 36 doubles of W once per
// column, and one thread per (edge, query), which holds W in registers for its six columns.  kCovEdgePerQuery chooses; the diagnostics
// time both (rgbd360_graph_time_cov_kernels).  Measured on 16-query batches (profiles/pose_graph_cov_perf.txt): per query 8.4 us against
// 12.0 us per column at 10^3 vertices, 34 us against 102 us at 10^4 -- the batch is bound by memory traffic, and W is two thirds of the
// edge product's.
#pragma once

constexpr int kCovChunk = 16;                  // queries per batch
constexpr bool kCovEdgePerQuery = true;        // the edge product's work mapping (see above)
enum { PGC_NOT_CONVERGED = 1, PGC_NOT_POSITIVE = 2 };      // per-query flags of k_pgc_finish

struct PgCov {
    PgCg cg;                                   // the 6 nq columns
    int nq;                                    // queries of this batch
    int *qi, *qj;                              // per query: `from` (-1: a marginal) and `to` / the vertex
    double* cov;                               // per query: 36, column-major
    int *q_it, *q_flags;                       // per query
    double* q_res;
};

namespace pg {

__global__ void __launch_bounds__(kBlock) k_pgc_init(PgDev G, PgCov C) {
    __shared__ double lds[kBlock];
    const int col = blockIdx.y, qd = col / 6, comp = col % 6;
    const int v = blockIdx.x * kBlock + threadIdx.x;
    double rz = 0.0;
    if (v < G.N) {
        const size_t o = ((size_t)col * G.N + v) * 6;
        double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (G.is_free[v]) {
            if (v == C.qj[qd]) r[comp] += 1.0;
            if (v == C.qi[qd]) r[comp] -= 1.0;
            if (r[comp] != 0.0) {
                const double* Minv = G.Minv + (size_t)v * 36;
                for (int i = 0; i < 6; ++i) {
                    double s = 0.0;
                    for (int c = 0; c < 6; ++c) s += Minv[c * 6 + i] * r[c];
                    z[i] = s;
                    rz += r[i] * s;
                }
            }
        }
        for (int i = 0; i < 6; ++i) {
            C.cg.x[o + i] = 0.0;
            C.cg.res[o + i] = r[i];
            C.cg.z[o + i] = z[i];
            C.cg.p[o + i] = z[i];
            C.cg.q[o + i] = 0.0;
        }
    }
    const double row = block_fold<Sum>(rz, lds);
    if (threadIdx.x == 0) {
        C.cg.rows_rz0[(size_t)col * G.nbV + blockIdx.x] = row;
        C.cg.rows_rz[(size_t)col * 2 * G.nbV + blockIdx.x] = row;
        if (blockIdx.x == 0) {
            C.cg.stop_at[col] = INT_MAX;
            C.cg.it[col] = 0;
            C.cg.broke[col] = 0;
            C.cg.resid[col] = 0.0;
        }
    }
}

// one workgroup of 64 threads per query
__global__ void __launch_bounds__(64) k_pgc_finish(PgDev G, PgCov C) {
    __shared__ double M[36], Ad[36], tmp[36];
    const int qd = blockIdx.x, tid = threadIdx.x;
    const int i = C.qi[qd], j = C.qj[qd];
    const int c = tid / 6, r = tid % 6;
    if (tid < 36) {
        const size_t oc = (size_t)(qd * 6 + c) * G.N;
        double m = C.cg.x[(oc + j) * 6 + r];      // x of a fixed or isolated vertex is 0
        if (i >= 0) m -= C.cg.x[(oc + i) * 6 + r];
        M[tid] = m;
    }
    if (i >= 0) {      // (uniform over the workgroup)
        if (tid == 0) {
            double inv[16], A[36];
            gn::rigid_inv(G.T + (size_t)i * 16, inv);
            gn::se3_adjoint(inv, A);
            for (int m = 0; m < 36; ++m) Ad[m] = A[m];
        }
        __syncthreads();
        if (tid < 36) {
            double s = 0.0;
            for (int m = 0; m < 6; ++m) s += Ad[m * 6 + r] * M[c * 6 + m];
            tmp[tid] = s;
        }
        __syncthreads();
        if (tid < 36) {
            double s = 0.0;
            for (int m = 0; m < 6; ++m) s += tmp[m * 6 + r] * Ad[m * 6 + c];
            M[tid] = s;
        }
    }
    __syncthreads();
    if (tid < 36) C.cov[(size_t)qd * 36 + tid] = 0.5 * (M[c * 6 + r] + M[r * 6 + c]);
    if (tid == 0) {
        int it = 0, flags = 0;
        double res = 0.0;
        for (int m = 0; m < 6; ++m) {
            const int col = qd * 6 + m;
            it = C.cg.it[col] > it ? C.cg.it[col] : it;
            res = C.cg.resid[col] > res ? C.cg.resid[col] : res;
            if (C.cg.broke[col]) flags |= PGC_NOT_POSITIVE;
            else if (C.cg.stop_at[col] == INT_MAX) flags |= PGC_NOT_CONVERGED;
        }
        C.q_it[qd] = it;
        C.q_res[qd] = res;
        C.q_flags[qd] = flags;
    }
}

}  // namespace pg

namespace {

// the device memory of one batch of nq queries (grows only), and C pointing into it
int cov_buffers(rgbd360_graph* g, int nq, PgCov* out) {
    const PgDev& G = g->G;
    const size_t q = nq, cols = 6 * q, n6 = (size_t)6 * std::max(G.N, 1), e6 = (size_t)6 * std::max(G.E, 1), nb = G.nbV;
    PgCov C;
    PgCg& S = C.cg;
    const ArenaPart<double> doubles[] = {{&S.x, cols * n6}, {&S.res, cols * n6}, {&S.z, cols * n6}, {&S.p, cols * n6}, {&S.q, cols * n6}, {&S.t, cols * e6},
                                         {&S.rows_rz0, cols * nb}, {&S.rows_rz, cols * 2 * nb}, {&S.rows_pq, cols * nb}, {&S.resid, cols},
                                         {&C.cov, q * 36}, {&C.q_res, q}};
    const ArenaPart<int> ints[] = {{&S.stop_at, cols}, {&S.it, cols}, {&S.broke, cols}, {&C.qi, q}, {&C.qj, q}, {&C.q_it, q}, {&C.q_flags, q}};
    PGC(g, arena_carve(g->d_cov, doubles));
    PGC(g, arena_carve(g->d_cov_i, ints));
    C.nq = nq; S.ncols = (int)cols;
    S.dd = nullptr;      // lambda = 0
    *out = C;
    return 0;
}

struct UnionFind {
    std::vector<int> parent;
    explicit UnionFind(int n) : parent(n) { for (int k = 0; k < n; ++k) parent[k] = k; }
    int find(int a) {
        while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; }
        return a;
    }
    void join(int a, int b) { parent[find(a)] = find(b); }
};

// relative: C_ij of the pairs (from[k], to[k]); otherwise the marginals of the vertices `to` (from is not read)
int graph_covariances(rgbd360_graph* g, const char* what, bool relative, int n, const int* from, const int* to, const rgbd360_graph_cov_params* params,
                      double* cov, int* cg_iterations, double* cg_residual, rgbd360_graph_cov_result* result) {
    if (!g) return -1;
    rgbd360_graph_cov_params P;
    rgbd360_graph_default_cov_params(&P);
    if (params) P = *params;
    if (n < 0) return graph_fail(g, -1, "n must be >= 0");
    if (P.cg_max_iters < 1 || P.cg_max_iters > 100000) return graph_fail(g, -1, "cg_max_iters must be in 1..100000");
    if (!(P.cg_tol > 0.0) || !(P.cg_tol < 1.0)) return graph_fail(g, -1, "cg_tol must be in (0, 1)");
    if (n > 0 && (!to || !cov || (relative && !from))) return graph_fail(g, -1, "null pointer");
    const int N = g->N(), E = g->E();
    for (int k = 0; k < n; ++k) {      // all of them before anything runs: an index never reaches a kernel unchecked
        const std::string who = "query " + std::to_string(k) + ": ";
        if (relative && (from[k] < 0 || from[k] >= N)) return graph_fail(g, -1, who + "from = " + std::to_string(from[k]) + " is no vertex");
        if (to[k] < 0 || to[k] >= N) return graph_fail(g, -1, who + (relative ? "to = " : "vertex = ") + std::to_string(to[k]) + " is no vertex");
    }
    rgbd360_graph_cov_result R;
    memset(&R, 0, sizeof(R));
    R.variance_factor = 1.0;
    R.n_queries = n;
    if (n == 0) {
        if (result) *result = R;
        return RGBD360_OK;
    }
    // the gauge: every free vertex a query touches must hang, over enabled edges, on a fixed one
    std::vector<char> free_v(N, 0), anchored(N, 0);
    long long n_enabled = 0;
    {
        UnionFind uf(N);
        std::vector<char> has_edge(N, 0);
        for (int e = 0; e < E; ++e)
            if (g->enabled[e]) {
                ++n_enabled;
                has_edge[g->ei[e]] = has_edge[g->ej[e]] = 1;
                uf.join(g->ei[e], g->ej[e]);
            }
        for (int v = 0; v < N; ++v) {
            free_v[v] = !g->fixed[v] && has_edge[v];
            if (g->fixed[v]) anchored[uf.find(v)] = 1;
        }
        for (int k = 0; k < n; ++k)
            for (int side = relative ? 0 : 1; side < 2; ++side) {
                const int v = side ? to[k] : from[k];
                if (relative && from[k] == to[k]) continue;
                if (free_v[v] && !anchored[uf.find(v)]) {
                    R.status = RGBD360_ILL_POSED;
                    if (result) *result = R;
                    return graph_fail(g, RGBD360_ILL_POSED, std::string(what) + ": query " + std::to_string(k) + ": vertex " + std::to_string(v) +
                                      " lies in a component without a fixed vertex: H is singular there");
                }
            }
    }
    int rc = graph_upload(g, false, 0);
    if (rc) return rc;
    R.n_fixed = g->n_fixed;
    R.n_isolated = g->n_isolated;
    rc = graph_chi2_now(g, &R.cost, nullptr);
    if (rc) return rc;
    R.dof = 6 * n_enabled - 6 * (long long)g->n_free;
    if (R.dof > 0) R.variance_factor = R.cost / (double)R.dof;
    // a query whose right-hand side is zero (a fixed or isolated vertex, from == to, two fixed ends) is an exact zero block
    std::vector<int> live;
    for (int k = 0; k < n; ++k) {
        const bool zero = relative ? (from[k] == to[k] || (!free_v[from[k]] && !free_v[to[k]])) : !free_v[to[k]];
        if (zero) {
            for (int m = 0; m < 36; ++m) cov[(size_t)k * 36 + m] = 0.0;
            if (cg_iterations) cg_iterations[k] = 0;
            if (cg_residual) cg_residual[k] = 0.0;
        } else {
            live.push_back(k);
        }
    }
    if (live.empty()) {
        if (result) *result = R;
        return RGBD360_OK;
    }
    hipStream_t s = g->ctx->stream;
    const PgDev& G = g->G;
    rc = graph_put_state(g, 0.0);
    if (rc) return rc;
    const dim3 blk(pg::kBlock);
    hipLaunchKernelGGL(pg::k_pg_edges<0>, dim3(G.nbE), blk, 0, s, G, -1);
    hipLaunchKernelGGL(pg::k_pg_assemble, dim3(G.nbV), blk, 0, s, G, -1);
    PGC(g, hipGetLastError());
    const int chunk = std::min((int)live.size(), kCovChunk);
    PgCov C;
    rc = cov_buffers(g, chunk, &C);
    if (rc) return rc;
    std::vector<int> q(2 * (size_t)chunk), h_it(chunk), h_flags(chunk);
    std::vector<double> h_cov(36 * (size_t)chunk), h_res(chunk), bad(G.nbV);
    bool not_positive = false;
    for (size_t first = 0; first < live.size(); first += chunk) {
        const int nq = (int)std::min(live.size() - first, (size_t)chunk);
        C.nq = nq; C.cg.ncols = 6 * nq;
        for (int k = 0; k < nq; ++k) {
            q[k] = relative ? from[live[first + k]] : -1;
            q[chunk + k] = to[live[first + k]];
        }
        PGC(g, hipMemcpyAsync(C.qi, q.data(), sizeof(int) * nq, hipMemcpyHostToDevice, s));
        PGC(g, hipMemcpyAsync(C.qj, q.data() + chunk, sizeof(int) * nq, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(pg::k_pgc_init, dim3(G.nbV, C.cg.ncols), blk, 0, s, G, C);
        for (int k = 0; k < P.cg_max_iters; ++k) cg_launch_iteration(s, G, C.cg, -1, k, P.cg_tol, kCovEdgePerQuery);
        hipLaunchKernelGGL(pg::k_pgc_finish, dim3(nq), dim3(64), 0, s, G, C);
        PGC(g, hipGetLastError());
        PGC(g, hipMemcpyAsync(h_cov.data(), C.cov, sizeof(double) * 36 * nq, hipMemcpyDeviceToHost, s));
        PGC(g, hipMemcpyAsync(h_res.data(), C.q_res, sizeof(double) * nq, hipMemcpyDeviceToHost, s));
        PGC(g, hipMemcpyAsync(h_it.data(), C.q_it, sizeof(int) * nq, hipMemcpyDeviceToHost, s));
        PGC(g, hipMemcpyAsync(h_flags.data(), C.q_flags, sizeof(int) * nq, hipMemcpyDeviceToHost, s));
        if (first == 0) PGC(g, hipMemcpyAsync(bad.data(), G.rows_bad, sizeof(double) * G.nbV, hipMemcpyDeviceToHost, s));
        PGC(g, hipStreamSynchronize(s));      // the one synchronisation of the batch
        if (first == 0)
            for (int b = 0; b < G.nbV; ++b) not_positive |= bad[b] > 0.0;      // a diagonal block without a Cholesky factor
        for (int k = 0; k < nq; ++k) {
            const int at = live[first + k];
            for (int m = 0; m < 36; ++m) cov[(size_t)at * 36 + m] = h_cov[(size_t)k * 36 + m];
            if (cg_iterations) cg_iterations[at] = h_it[k];
            if (cg_residual) cg_residual[at] = h_res[k];
            R.cg_iterations_max = std::max(R.cg_iterations_max, h_it[k]);
            R.cg_residual_max = std::max(R.cg_residual_max, h_res[k]);
            if (h_flags[k] & PGC_NOT_POSITIVE) not_positive = true;
            else if (h_flags[k] & PGC_NOT_CONVERGED) R.n_not_converged++;
        }
    }
    R.status = not_positive ? RGBD360_ILL_POSED : R.n_not_converged ? RGBD360_NOT_CONVERGED : RGBD360_OK;
    if (result) *result = R;
    if (not_positive) g->err = std::string(what) + ": H is not positive definite (p.q <= 0 on an unfinished column, or a diagonal block without a Cholesky factor)";
    else if (R.n_not_converged) g->err = std::string(what) + ": " + std::to_string(R.n_not_converged) + " queries have columns that did not reach cg_tol within cg_max_iters";
    return R.status;
}

}  // namespace

extern "C" {

void rgbd360_graph_default_cov_params(rgbd360_graph_cov_params* p) {
    if (!p) return;
    p->cg_max_iters = 1000;
    p->cg_tol = 1e-10;
}

int rgbd360_graph_marginals(rgbd360_graph* g, int n, const int* vertices, const rgbd360_graph_cov_params* params, double* cov,
                            int* cg_iterations, double* cg_residual, rgbd360_graph_cov_result* result) {
    return graph_covariances(g, "rgbd360_graph_marginals", false, n, nullptr, vertices, params, cov, cg_iterations, cg_residual, result);
}

int rgbd360_graph_relative_covariances(rgbd360_graph* g, int n, const int* from, const int* to, const rgbd360_graph_cov_params* params,
                                       double* cov, int* cg_iterations, double* cg_residual, rgbd360_graph_cov_result* result) {
    return graph_covariances(g, "rgbd360_graph_relative_covariances", true, n, from, to, params, cov, cg_iterations, cg_residual, result);
}

int rgbd360_graph_time_cov_kernels(rgbd360_graph* g, int n, const int* vertices, int reps, float avg_us[8]) {
    if (!g) return -1;
    if (!avg_us || reps < 1 || n < 1 || n > kCovChunk || !vertices) return graph_fail(g, -1, "bad arguments");
    for (int k = 0; k < n; ++k)
        if (vertices[k] < 0 || vertices[k] >= g->N()) return graph_fail(g, -1, "query " + std::to_string(k) + " is no vertex");
    int rc = graph_upload(g, false, 0);
    if (rc) return rc;
    for (int k = 0; k < 8; ++k) avg_us[k] = 0.f;
    if (!g->E()) return 0;
    hipStream_t s = g->ctx->stream;
    const PgDev& G = g->G;
    rc = graph_put_state(g, 0.0);
    if (rc) return rc;
    PgCov C;
    rc = cov_buffers(g, n, &C);
    if (rc) return rc;
    std::vector<int> q(2 * (size_t)n, -1);
    for (int k = 0; k < n; ++k) q[n + k] = vertices[k];
    PGC(g, hipMemcpyAsync(C.qi, q.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
    PGC(g, hipMemcpyAsync(C.qj, q.data() + n, sizeof(int) * n, hipMemcpyHostToDevice, s));
    const PgCg& S = C.cg;
    const dim3 blk(pg::kBlock), gv(G.nbV, S.ncols);
    hipLaunchKernelGGL(pg::k_pg_edges<0>, dim3(G.nbE), blk, 0, s, G, -1);
    hipLaunchKernelGGL(pg::k_pg_assemble, dim3(G.nbV), blk, 0, s, G, -1);
    // every timed launch carries iteration 0 with a tolerance of 0: no column ever stops, each repetition does the full work
    auto launch = [&](int which) {
        switch (which) {
            case 0: hipLaunchKernelGGL(pg::k_pgc_init, gv, blk, 0, s, G, C); break;
            case 1: hipLaunchKernelGGL(pg::k_pg_cg_edge<false>, dim3(G.nbE, S.ncols), blk, 0, s, G, S, -1, 0); break;
            case 2: hipLaunchKernelGGL(pg::k_pg_cg_edge<true>, dim3(G.nbE, C.nq), blk, 0, s, G, S, -1, 0); break;
            case 3: hipLaunchKernelGGL(pg::k_pg_cg_gather, gv, blk, 0, s, G, S, -1, 0); break;
            case 4: hipLaunchKernelGGL(pg::k_pg_cg_update, gv, blk, 0, s, G, S, -1, 0); break;
            case 5: hipLaunchKernelGGL(pg::k_pg_cg_dir, gv, blk, 0, s, G, S, -1, 0, 0.0); break;
            case 6: hipLaunchKernelGGL(pg::k_pgc_finish, dim3(C.nq), dim3(64), 0, s, G, C); break;
            default: hipLaunchKernelGGL(pg::k_pg_cg_gather, gv, blk, 0, s, G, S, -1, INT_MAX); break;      // returns on the stop word
        }
    };
    return graph_time_slots(g, 8, reps, avg_us, launch, [](int) { return 0; });      // (q is a local: the helper ends on a synchronisation)
}

}  // extern "C"
