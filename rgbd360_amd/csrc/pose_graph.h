// pose_graph.h -- a device pose-graph optimiser (rgbd360_graph_*, include/rgbd360_hip.h).  Included by rgbd360_api.hip
// behind frame_store.h: the edges are what rgbd360_store_align returns (relative pose + Hessian), the optimised poses are what
// rgbd360_map_move_* takes.  The reference does this step in g2o (GraphOptimizer_G2O.cpp: Levenberg-Marquardt, dense linear solver,
// optimize(10), vertex 0 fixed; KFsphere_SLAM.cpp:679-689).
//
// One Levenberg-Marquardt iteration `it` is a fixed list of launches, enqueued blindly by the host:
//   k_pg_edges<linearise>   per edge: r, s = r^T Omega r, the robust rho(s) and w(s), W = w A^T Omega A, b = w A^T Omega r -> one partial row of
//                           rho per workgroup
//   k_pg_assemble           per vertex over its CSR row: diagonal block D, gradient g, (D + lambda diag D)^-1, the PCG start
//   cg_max_iters times      k_pg_cg_edge (t_e = W (p_i - p_j)), k_pg_cg_gather (q = sum +-t_e + lambda diag(D) p, p.q rows),
//                           k_pg_cg_update (x, r, z, r.z rows), k_pg_cg_dir (stop test, p = z + beta p)
//   k_pg_trial              T' = se3_exp(x) T per vertex, max |x| rows
//   k_pg_edges<chi2>        the cost (sum of rho) at T'
//   k_pg_decide             accept / reject, lambda, the trace record, the stop test
// The four k_pg_cg_* kernels are the one block-Jacobi PCG of this library: they work on a view (PgCg) of `ncols` right-hand sides,
// blockIdx.y is the column, every column has its own rows, alpha, beta and stop words.  The optimiser runs them on one column with the
// damping lambda diag D; the covariance batch (pose_graph_cov.h) on up to 96 columns without it.
// House rules: no floating-point atomics; a vertex adds its edges in CSR (= edge list) order; every global scalar is a table of
// per-workgroup partial rows which each consumer re-adds in ascending order in its prologue (pg::rows_fold), so that all blocks take the
// same decision from the same bits; no cooperative launch, no spin barrier, no ticket.  A kernel never reads a state word it writes:
// the stop words are "first index that does not run" (stop_it, a column's stop_at), compared with the index the launch carries, so a
// launch of a finished loop or of a converged PCG returns at once, and the block that records a stop cannot change what its own launch does.
// Robust and switchable edges: per edge one word `kind` (RGBD360_GRAPH_ROBUST_*, -1 = disabled) and one `delta`.  A disabled edge has
// rho = w = 0 and is in no vertex's CSR row, so W, b and t of it are written and never read; a quadratic edge has rho = s and w = an exact
// 1.0, so a graph of quadratic, enabled edges keeps the bits it had before the kinds existed.
#pragma once

#include <climits>

struct rgbd360_graph_state {      // device + pinned host copy
    int stop_it, cg_stop_at, cg_it, status, accepted, converged, iterations, cg_broke;      // cg_*: the optimiser's PCG column (graph_cg)
    long long cg_total;
    double lambda, chi2, chi2_initial, chi2_final, cg_res;
};

struct PgDev {
    int N, E, nbV, nbE;
    const int *ei, *ej, *row_ptr, *inc, *is_free, *kind;      // kind: RGBD360_GRAPH_ROBUST_* of an enabled edge, -1 of a disabled one
    const double *Z, *Om, *delta;
    double *T, *Tt;
    double *r, *W, *b, *echi2, *A;          // per edge (echi2: the raw s; A: diagnostics only, may be null)
    double *erho, *ew;                       // per edge: rho (mode 2 only) and the weight w
    double *D, *g, *Minv, *dd, *x, *res, *z, *p, *q;      // per vertex
    double *t;                               // per edge: W (p_i - p_j)
    double *rows_chi2, *rows_chi2_trial, *rows_rz0, *rows_rz /* [2][nbV] */, *rows_pq, *rows_maxx, *rows_bad;
    rgbd360_graph_state* st;
    rgbd360_graph_iteration* trace;
};

// What the PCG kernels touch: `ncols` systems H x = b on the graph G describes (W per edge, Minv per vertex), solved in lock step.
struct PgCg {
    int ncols;
    double *x, *res, *z, *p, *q;               // [column][6 N]
    double* t;                                 // [column][6 E]
    double *rows_rz0, *rows_rz /* [column][2][nbV] */, *rows_pq;      // [column][nbV]
    int *stop_at, *it, *broke;                 // per column: the first iteration that does not run, iterations done, p.q <= 0 was met
    double* resid;                             // per column: |r|_M / |r_0|_M
    const double* dd;                          // [6 N]: the damping lambda diag D added to H, or null (none)
};

namespace pg {

constexpr int kBlock = 256;

struct Sum { __device__ static double of(double acc, double v) { return acc + v; } };
struct Max { __device__ static double of(double acc, double v) { return v > acc ? v : acc; } };      // (a NaN never raises it)

// rows[0..n) folded in ascending order from 0.0, the same bits in every thread of every block
template <class Fold>
__device__ inline double rows_fold(const double* rows, int n, double* lds) {
    double s = 0.0;
    for (int base = 0; base < n; base += kBlock) {
        __syncthreads();
        if (base + (int)threadIdx.x < n) lds[threadIdx.x] = rows[base + threadIdx.x];
        __syncthreads();
        const int m = n - base < kBlock ? n - base : kBlock;
        for (int k = 0; k < m; ++k) s = Fold::of(s, lds[k]);
    }
    __syncthreads();
    return s;
}
// one partial row: the block's values folded by a fixed tree
template <class Fold>
__device__ inline double block_fold(double v, double* lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] = Fold::of(lds[threadIdx.x], lds[threadIdx.x + s]);
        __syncthreads();
    }
    const double out = lds[0];
    __syncthreads();
    return out;
}

// inv = M^-1 through the Cholesky factor of the symmetric 6x6 M (lower triangle read); false: M has none
GN_HD inline bool chol_inv6(const double* M, double* inv) {
    double L[6][6];
    for (int j = 0; j < 6; ++j) {
        double d = M[j * 6 + j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !(d < 1.7e308)) return false;
        const double l = sqrt(d);
        L[j][j] = l;
        for (int i = j + 1; i < 6; ++i) {
            double s = M[j * 6 + i];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / l;
        }
    }
    for (int col = 0; col < 6; ++col) {
        double y[6];
        for (int i = 0; i < 6; ++i) {
            double s = i == col ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
            y[i] = s / L[i][i];
        }
        for (int i = 5; i >= 0; --i) {
            double s = y[i];
            for (int k = i + 1; k < 6; ++k) s -= L[k][i] * y[k];
            y[i] = s / L[i][i];
        }
        for (int i = 0; i < 6; ++i) inv[col * 6 + i] = y[i];
    }
    return true;
}

// r = se3_log(Z Tj^-1 Ti) and M = Z Tj^-1 of one edge
GN_HD inline void edge_residual(const double* Ti, const double* Tj, const double* Z, double* r, double* M) {
    double inv[16], E[16];
    gn::rigid_inv(Tj, inv);
    gn::rigid_mul(Z, inv, M);
    gn::rigid_mul(M, Ti, E);
    gn::se3_log(E, r);
}

// mode 0: linearise at T (r, W, b, per-edge s and w, A when asked, cost rows); mode 1: the cost at the trial poses (per-edge s, trial rows);
// mode 2: the cost at T into the trial rows, per-edge s, rho and w (rgbd360_graph_chi2, rgbd360_graph_edge_weights)
template <int kMode>
__global__ void __launch_bounds__(kBlock) k_pg_edges(PgDev G, int it) {
    __shared__ double lds[kBlock];
    if (it >= 0 && G.st->stop_it <= it) return;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    double rho = 0.0;
    if (e < G.E) {
        double chi2 = 0.0, w = 0.0;
        const double* P = kMode == 1 ? G.Tt : G.T;
        const double* Om = G.Om + (size_t)e * 36;
        double r[6], M[16], Or[6];
        edge_residual(P + (size_t)G.ei[e] * 16, P + (size_t)G.ej[e] * 16, G.Z + (size_t)e * 16, r, M);
        for (int i = 0; i < 6; ++i) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += Om[k * 6 + i] * r[k];
            Or[i] = s;
        }
        for (int i = 0; i < 6; ++i) chi2 += r[i] * Or[i];
        G.echi2[e] = chi2;
        const int kind = G.kind[e];
        if (kind >= 0) gn::robust_rho_w(kind, G.delta[e], chi2, &rho, &w);
        if (kMode != 1) G.ew[e] = w;
        if (kMode == 2) G.erho[e] = rho;
        if (kMode == 0) {
            double J[36], Ad[36], A[36], OA[36];
            gn::se3_jl_inv(r, J);
            gn::se3_adjoint(M, Ad);
            gn::mat6_mul(J, Ad, A);
            gn::mat6_mul(Om, A, OA);
            double* W = G.W + (size_t)e * 36;
            for (int c = 0; c < 6; ++c)
                for (int rr = 0; rr <= c; ++rr) {
                    double s = 0.0;
                    for (int k = 0; k < 6; ++k) s += A[rr * 6 + k] * OA[c * 6 + k];
                    W[c * 6 + rr] = w * s;
                    W[rr * 6 + c] = w * s;
                }
            for (int i = 0; i < 6; ++i) {
                double s = 0.0;
                for (int k = 0; k < 6; ++k) s += A[i * 6 + k] * Or[k];
                G.b[(size_t)e * 6 + i] = w * s;
                G.r[(size_t)e * 6 + i] = r[i];
            }
            if (G.A)
                for (int k = 0; k < 36; ++k) G.A[(size_t)e * 36 + k] = A[k];
        }
    }
    const double row = block_fold<Sum>(rho, lds);
    if (threadIdx.x == 0) (kMode == 0 ? G.rows_chi2 : G.rows_chi2_trial)[blockIdx.x] = row;
}

__global__ void __launch_bounds__(kBlock) k_pg_assemble(PgDev G, int it) {
    __shared__ double lds[kBlock];
    if (it >= 0 && G.st->stop_it <= it) return;
    const double chi2 = rows_fold<Sum>(G.rows_chi2, G.nbE, lds);
    const double lambda = G.st->lambda;
    const int v = blockIdx.x * kBlock + threadIdx.x;
    double rz = 0.0, bad = 0.0;
    if (v < G.N) {
        double* x = G.x + (size_t)v * 6;
        double* res = G.res + (size_t)v * 6;
        double* z = G.z + (size_t)v * 6;
        double* p = G.p + (size_t)v * 6;
        double* q = G.q + (size_t)v * 6;
        for (int i = 0; i < 6; ++i) x[i] = res[i] = z[i] = p[i] = q[i] = 0.0;
        if (G.is_free[v]) {
            double D[36], g[6], Minv[36];
            for (int k = 0; k < 36; ++k) D[k] = 0.0;
            for (int i = 0; i < 6; ++i) g[i] = 0.0;
            for (int a = G.row_ptr[v]; a < G.row_ptr[v + 1]; ++a) {
                const int code = G.inc[a], e = code >> 1;
                const double* W = G.W + (size_t)e * 36;
                const double* b = G.b + (size_t)e * 6;
                for (int k = 0; k < 36; ++k) D[k] += W[k];
                if (code & 1)
                    for (int i = 0; i < 6; ++i) g[i] -= b[i];
                else
                    for (int i = 0; i < 6; ++i) g[i] += b[i];
            }
            double* dd = G.dd + (size_t)v * 6;
            for (int i = 0; i < 6; ++i) {
                dd[i] = lambda * D[i * 6 + i];
                G.g[(size_t)v * 6 + i] = g[i];
            }
            for (int k = 0; k < 36; ++k) G.D[(size_t)v * 36 + k] = D[k];
            for (int i = 0; i < 6; ++i) D[i * 6 + i] += dd[i];
            if (!chol_inv6(D, Minv)) {
                bad = 1.0;
                for (int k = 0; k < 36; ++k) Minv[k] = 0.0;
            }
            for (int k = 0; k < 36; ++k) G.Minv[(size_t)v * 36 + k] = Minv[k];
            for (int i = 0; i < 6; ++i) {
                double s = 0.0;
                for (int k = 0; k < 6; ++k) s += Minv[k * 6 + i] * (-g[k]);
                res[i] = -g[i];
                z[i] = s;
                p[i] = s;
                rz += -g[i] * s;
            }
        }
    }
    const double row = block_fold<Sum>(rz, lds);
    const double badrow = block_fold<Max>(bad, lds);
    if (threadIdx.x == 0) {
        G.rows_rz0[blockIdx.x] = row;
        G.rows_rz[blockIdx.x] = row;
        G.rows_bad[blockIdx.x] = badrow;
        if (blockIdx.x == 0) {
            G.st->cg_stop_at = INT_MAX;
            G.st->cg_it = 0;
            G.st->cg_res = 0.0;
            G.st->chi2 = chi2;
            if (it <= 0) G.st->chi2_initial = chi2;
        }
    }
}

// ---- the block-Jacobi PCG: iteration k of every column of C that has not stopped.  `it` is the Levenberg-Marquardt iteration the launch
// belongs to, or -1 outside the optimiser's loop (stop_it then decides nothing).  stop_it is never negative, so the test on `it` changes
// nothing where the launches of the loop, which carry it >= 0, did without it.
// Has column `col` of this launch nothing to do?  Both stop words are loaded before either is tested -- hence & and |, not && and || --
// so that a launch waits for one round trip to memory, not for two in a row.
__device__ inline bool cg_stopped(const PgDev& G, const PgCg& C, int col, int it, int k) {
    const int stop_it = G.st->stop_it, stop_at = C.stop_at[col];
    return ((it >= 0) & (stop_it <= it)) | (stop_at <= k);
}

// one column of one edge: t = W (p_i - p_j)
__device__ inline void cg_edge_column(const PgDev& G, const PgCg& C, int e, int col, const double* W) {
    const double* pi = C.p + ((size_t)col * G.N + G.ei[e]) * 6;
    const double* pj = C.p + ((size_t)col * G.N + G.ej[e]) * 6;
    double* t = C.t + ((size_t)col * G.E + e) * 6;
    double d[6];
    for (int i = 0; i < 6; ++i) d[i] = pi[i] - pj[i];
    for (int i = 0; i < 6; ++i) {
        double s = 0.0;
        for (int c = 0; c < 6; ++c) s += W[c * 6 + i] * d[c];
        t[i] = s;
    }
}

// Two work mappings with the same bits.  kPerQuery false: grid (nbE, columns), W read from memory; true: grid (nbE, columns / 6), W held in
// registers for the six columns of a covariance query
template <bool kPerQuery>
__global__ void __launch_bounds__(kBlock) k_pg_cg_edge(PgDev G, PgCg C, int it, int k) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (!kPerQuery) {
        const int col = blockIdx.y;
        if (cg_stopped(G, C, col, it, k) || e >= G.E) return;
        cg_edge_column(G, C, e, col, G.W + (size_t)e * 36);
    } else {
        const int c0 = blockIdx.y * 6;
        bool none = true;
        for (int c = 0; c < 6; ++c) none &= cg_stopped(G, C, c0 + c, it, k);
        if (none || e >= G.E) return;
        double W[36];
        for (int m = 0; m < 36; ++m) W[m] = G.W[(size_t)e * 36 + m];
        for (int c = 0; c < 6; ++c)
            if (C.stop_at[c0 + c] > k) cg_edge_column(G, C, e, c0 + c, W);
    }
}

__global__ void __launch_bounds__(kBlock) k_pg_cg_gather(PgDev G, PgCg C, int it, int k) {
    __shared__ double lds[kBlock];
    const int col = blockIdx.y;
    if (cg_stopped(G, C, col, it, k)) return;
    const int v = blockIdx.x * kBlock + threadIdx.x;
    double pq = 0.0;
    if (v < G.N && G.is_free[v]) {
        const size_t o = ((size_t)col * G.N + v) * 6;
        const double* tc = C.t + (size_t)col * G.E * 6;
        double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int a = G.row_ptr[v]; a < G.row_ptr[v + 1]; ++a) {
            const int code = G.inc[a];
            const double* t = tc + (size_t)(code >> 1) * 6;
            if (code & 1)
                for (int i = 0; i < 6; ++i) q[i] -= t[i];
            else
                for (int i = 0; i < 6; ++i) q[i] += t[i];
        }
        if (C.dd)      // (uniform over the grid; no zero vector in its place: -0.0 + 0.0 would flip a sign bit of q)
            for (int i = 0; i < 6; ++i) q[i] += C.dd[(size_t)v * 6 + i] * C.p[o + i];
        for (int i = 0; i < 6; ++i) {
            C.q[o + i] = q[i];
            pq += C.p[o + i] * q[i];
        }
    }
    const double row = block_fold<Sum>(pq, lds);
    if (threadIdx.x == 0) C.rows_pq[(size_t)col * G.nbV + blockIdx.x] = row;
}

__global__ void __launch_bounds__(kBlock) k_pg_cg_update(PgDev G, PgCg C, int it, int k) {
    __shared__ double lds[kBlock];
    const int col = blockIdx.y;
    if (cg_stopped(G, C, col, it, k)) return;
    const double rz = rows_fold<Sum>(C.rows_rz + ((size_t)col * 2 + (k & 1)) * G.nbV, G.nbV, lds);
    const double pq = rows_fold<Sum>(C.rows_pq + (size_t)col * G.nbV, G.nbV, lds);
    const bool go = pq > 0.0;
    const double alpha = go ? rz / pq : 0.0;
    const int v = blockIdx.x * kBlock + threadIdx.x;
    double rz_new = 0.0;
    if (go && v < G.N && G.is_free[v]) {
        const size_t o = ((size_t)col * G.N + v) * 6;
        const double* Minv = G.Minv + (size_t)v * 36;
        double rr[6];
        for (int i = 0; i < 6; ++i) {
            C.x[o + i] += alpha * C.p[o + i];
            rr[i] = C.res[o + i] - alpha * C.q[o + i];
            C.res[o + i] = rr[i];
        }
        for (int i = 0; i < 6; ++i) {
            double s = 0.0;
            for (int c = 0; c < 6; ++c) s += Minv[c * 6 + i] * rr[c];
            C.z[o + i] = s;
            rz_new += rr[i] * s;
        }
    }
    const double row = block_fold<Sum>(rz_new, lds);
    if (threadIdx.x == 0) C.rows_rz[((size_t)col * 2 + ((k + 1) & 1)) * G.nbV + blockIdx.x] = row;
}

__global__ void __launch_bounds__(kBlock) k_pg_cg_dir(PgDev G, PgCg C, int it, int k, double cg_tol) {
    __shared__ double lds[kBlock];
    const int col = blockIdx.y;
    if (cg_stopped(G, C, col, it, k)) return;
    const double rz0 = rows_fold<Sum>(C.rows_rz0 + (size_t)col * G.nbV, G.nbV, lds);
    const double rz = rows_fold<Sum>(C.rows_rz + ((size_t)col * 2 + (k & 1)) * G.nbV, G.nbV, lds);
    const double pq = rows_fold<Sum>(C.rows_pq + (size_t)col * G.nbV, G.nbV, lds);
    const double rz_new = rows_fold<Sum>(C.rows_rz + ((size_t)col * 2 + ((k + 1) & 1)) * G.nbV, G.nbV, lds);
    const bool broke = !(pq > 0.0);      // nothing was updated: H is not positive definite along p, or the column started at zero (rz0 = 0)
    const bool stop = broke || !(sqrt(rz_new > 0.0 ? rz_new : 0.0) > cg_tol * sqrt(rz0));
    if (!stop) {
        const double beta = rz_new / rz;
        const int v = blockIdx.x * kBlock + threadIdx.x;
        if (v < G.N && G.is_free[v]) {
            const size_t o = ((size_t)col * G.N + v) * 6;
            for (int i = 0; i < 6; ++i) C.p[o + i] = C.z[o + i] + beta * C.p[o + i];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double last = broke ? rz : rz_new;
        C.it[col] = broke ? k : k + 1;
        C.resid[col] = rz0 > 0.0 ? sqrt((last > 0.0 ? last : 0.0) / rz0) : 0.0;
        if (broke) C.broke[col] = 1;
        if (stop) C.stop_at[col] = k + 1;
    }
}

__global__ void __launch_bounds__(kBlock) k_pg_trial(PgDev G, int it) {
    __shared__ double lds[kBlock];
    if (G.st->stop_it <= it) return;
    const int v = blockIdx.x * kBlock + threadIdx.x;
    double mx = 0.0;
    if (v < G.N) {
        const double* T = G.T + (size_t)v * 16;
        double* Tt = G.Tt + (size_t)v * 16;
        if (G.is_free[v]) {
            double x[6], X[16], out[16];
            for (int i = 0; i < 6; ++i) {
                x[i] = G.x[(size_t)v * 6 + i];
                const double a = fabs(x[i]);
                mx = a > mx ? a : mx;      // (a NaN never raises it: the chi2 test rejects such a step)
            }
            gn::se3_exp(x, X);
            gn::rigid_mul(X, T, out);
            for (int k = 0; k < 16; ++k) Tt[k] = out[k];
        } else {
            for (int k = 0; k < 16; ++k) Tt[k] = T[k];
        }
    }
    const double row = block_fold<Max>(mx, lds);
    if (threadIdx.x == 0) G.rows_maxx[blockIdx.x] = row;
}

__global__ void __launch_bounds__(kBlock) k_pg_decide(PgDev G, int it, int max_iters, double tol_update, double lambda_max) {
    __shared__ double lds[kBlock];
    if (G.st->stop_it <= it) return;
    const double cur = rows_fold<Sum>(G.rows_chi2, G.nbE, lds);
    const double trial = rows_fold<Sum>(G.rows_chi2_trial, G.nbE, lds);
    const bool bad = rows_fold<Max>(G.rows_bad, G.nbV, lds) > 0.0;
    const double max_x = rows_fold<Max>(G.rows_maxx, G.nbV, lds);
    const bool accept = !bad && trial < cur;
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (accept && v < G.N && G.is_free[v])
        for (int k = 0; k < 16; ++k) G.T[(size_t)v * 16 + k] = G.Tt[(size_t)v * 16 + k];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        rgbd360_graph_state& S = *G.st;
        const double lambda = S.lambda;
        bool stop = false;
        if (bad) {      // a damped diagonal block without a Cholesky factor: no step was taken, nothing is recorded
            S.status = RGBD360_ILL_POSED;
            stop = true;
        } else {
            rgbd360_graph_iteration& R = G.trace[it];
            R.chi2 = cur; R.chi2_trial = trial; R.lambda = lambda; R.accepted = accept ? 1 : 0;
            R.cg_iterations = S.cg_it; R.cg_residual = S.cg_res; R.max_update = max_x;
            S.iterations = it + 1;
            S.cg_total += S.cg_it;
            if (accept) {
                S.accepted += 1;
                S.chi2_final = trial;
                const double l = lambda / 10.0;
                S.lambda = l < 1e-9 ? 1e-9 : l;
                if (max_x <= tol_update) { S.converged = 1; stop = true; }
            } else {
                S.chi2_final = cur;
                S.lambda = lambda * 10.0;
                if (S.lambda > lambda_max) { S.status = RGBD360_ILL_POSED; stop = true; }
            }
        }
        if (stop || it + 1 >= max_iters) S.stop_it = it + 1;
    }
}

}  // namespace pg

struct rgbd360_graph {
    rgbd360_ctx* ctx = nullptr;
    std::vector<double> T;            // 16 per vertex, column-major: the float32 inputs widened, then what the optimiser left
    std::vector<char> fixed;
    std::vector<int> ei, ej;
    std::vector<double> Z, Om;        // 16 / 36 per edge (Om symmetrised)
    std::vector<int> kind;            // per edge: RGBD360_GRAPH_ROBUST_*
    std::vector<double> delta;
    std::vector<char> enabled;
    bool dirty = true;                // vertices, flags, edges or enabled flags changed since the CSR and edge arrays were uploaded
    bool settings_dirty = true;       // kinds or deltas changed since the two per-edge setting arrays were uploaded
    std::vector<int> kind_up;         // what the kernels read: kind, or -1 for a disabled edge
    std::vector<int> is_free;         // per vertex: not fixed and not isolated (as of the last upload)
    int n_fixed = 0, n_isolated = 0, n_free = 0;
    DevBuf<int> d_ei, d_ej, d_row_ptr, d_inc, d_is_free, d_kind;
    DevBuf<double> d_delta, d_Z, d_Om, d_T, d_Tt, d_edge, d_vert, d_rows, d_A;
    DevBuf<double> d_cov;             // the column vectors, rows and outputs of a covariance batch (pose_graph_cov.h)
    DevBuf<int> d_cov_i;
    DevBuf<rgbd360_graph_state> d_state;
    PinnedBuf<rgbd360_graph_state> h_state;
    DevBuf<rgbd360_graph_iteration> d_trace;
    std::vector<rgbd360_graph_iteration> trace;
    PgDev G;
    std::string err;
    int N() const { return (int)fixed.size(); }
    int E() const { return (int)ei.size(); }
};

namespace {

int graph_fail(rgbd360_graph* g, int code, const std::string& msg) {
    g->err = msg;
    return code;
}

#define PGC(g, expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            (void)hipStreamSynchronize((g)->ctx->stream);                                                 \
            return graph_fail(g, -(int)e_ - 1000, std::string(#expr) + ": " + hipGetErrorString(e_));     \
        }                                                                                                 \
    } while (0)

bool pg_finite(const float* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// One device buffer cut into consecutive parts: the buffer's size is the sum of the list that hands out the pointers.
template <class T>
struct ArenaPart {
    T** at;      // where the part's pointer goes
    size_t count;
};
template <class T, size_t K>
hipError_t arena_carve(DevBuf<T>& buf, const ArenaPart<T> (&parts)[K]) {
    size_t total = 0;
    for (const ArenaPart<T>& part : parts) total += part.count;
    const hipError_t e = buf.ensure(total);
    if (e != hipSuccess) return e;
    T* p = buf;
    for (const ArenaPart<T>& part : parts) {
        *part.at = p;
        p += part.count;
    }
    return hipSuccess;
}

// The optimiser's PCG: one column on the vectors and rows of G, damped by G.dd; its stop words are those of the device state, so that
// k_pg_assemble starts it, k_pg_decide records it and the host reads it back with the state.  (cg_broke is written and never read.)
PgCg graph_cg(const PgDev& G) {
    PgCg C;
    C.ncols = 1;
    C.x = G.x; C.res = G.res; C.z = G.z; C.p = G.p; C.q = G.q; C.t = G.t;
    C.rows_rz0 = G.rows_rz0; C.rows_rz = G.rows_rz; C.rows_pq = G.rows_pq;
    C.stop_at = &G.st->cg_stop_at; C.it = &G.st->cg_it; C.broke = &G.st->cg_broke; C.resid = &G.st->cg_res;
    C.dd = G.dd;
    return C;
}

// One full iteration k of the PCG on every column of C.  per_query: the edge product's work mapping (k_pg_cg_edge), ncols = 6 queries then.
void cg_launch_iteration(hipStream_t s, const PgDev& G, const PgCg& C, int it, int k, double cg_tol, bool per_query) {
    const dim3 blk(pg::kBlock), gv(G.nbV, C.ncols);
    if (per_query) hipLaunchKernelGGL(pg::k_pg_cg_edge<true>, dim3(G.nbE, C.ncols / 6), blk, 0, s, G, C, it, k);
    else hipLaunchKernelGGL(pg::k_pg_cg_edge<false>, dim3(G.nbE, C.ncols), blk, 0, s, G, C, it, k);
    hipLaunchKernelGGL(pg::k_pg_cg_gather, gv, blk, 0, s, G, C, it, k);
    hipLaunchKernelGGL(pg::k_pg_cg_update, gv, blk, 0, s, G, C, it, k);
    hipLaunchKernelGGL(pg::k_pg_cg_dir, gv, blk, 0, s, G, C, it, k, cg_tol);
}

// avg_us[w], w < n: the HIP-event average of `reps` launch(w) after one untimed launch(w), whose outputs are then the inputs the loop
// would hand it.  prepare(w) runs first and may enqueue a change of the state (0, or the code to return).
template <class Launch, class Prepare>
int graph_time_slots(rgbd360_graph* g, int n, int reps, float* avg_us, Launch launch, Prepare prepare) {
    rgbd360_ctx* ctx = g->ctx;
    hipStream_t s = ctx->stream;
    for (int which = 0; which < n; ++which) {
        const int rc = prepare(which);
        if (rc) return rc;
        launch(which);
        PGC(g, hipEventRecord(ctx->ev0, s));
        for (int k = 0; k < reps; ++k) launch(which);
        PGC(g, hipEventRecord(ctx->ev1, s));
        PGC(g, hipGetLastError());
        PGC(g, hipEventSynchronize(ctx->ev1));
        float ms = 0.f;
        PGC(g, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        avg_us[which] = ms * 1000.f / (float)reps;
    }
    PGC(g, hipStreamSynchronize(s));
    return 0;
}

// Everything the kernels read, on the device: the CSR and the edge arrays when the graph changed, the poses always (128 bytes a vertex).
// with_A: room for the diagnostics' per-edge Jacobians.
int graph_upload(rgbd360_graph* g, bool with_A, int max_trace) {
    const int N = g->N(), E = g->E();
    hipStream_t s = g->ctx->stream;
    hipSetDevice(g->ctx->p.device);
    const int nbV = std::max(1, (N + pg::kBlock - 1) / pg::kBlock), nbE = std::max(1, (E + pg::kBlock - 1) / pg::kBlock);
    const size_t n1 = std::max(N, 1), e1 = std::max(E, 1);
    PgDev& G = g->G;
    const bool settings = g->dirty || g->settings_dirty;
    if (g->dirty) {
        std::vector<int> row_ptr(N + 1, 0), inc(2 * (size_t)E);      // (a disabled edge is in no row: inc may end short of 2 E)
        for (int e = 0; e < E; ++e)
            if (g->enabled[e]) { row_ptr[g->ei[e] + 1]++; row_ptr[g->ej[e] + 1]++; }
        for (int v = 0; v < N; ++v) row_ptr[v + 1] += row_ptr[v];
        std::vector<int> at(row_ptr.begin(), row_ptr.end() - 1);
        for (int e = 0; e < E; ++e) {      // a vertex's row lists its enabled edges in edge order: side 0 = `from`, 1 = `to`
            if (!g->enabled[e]) continue;
            inc[at[g->ei[e]]++] = e * 2;
            inc[at[g->ej[e]]++] = e * 2 + 1;
        }
        g->is_free.assign(n1, 0);
        g->n_fixed = g->n_isolated = g->n_free = 0;
        for (int v = 0; v < N; ++v) {
            const bool isolated = row_ptr[v + 1] == row_ptr[v];
            if (g->fixed[v]) g->n_fixed++;
            else if (isolated) g->n_isolated++;
            else { g->is_free[v] = 1; g->n_free++; }
        }
        PGC(g, g->d_ei.ensure(e1)); PGC(g, g->d_ej.ensure(e1)); PGC(g, g->d_row_ptr.ensure(n1 + 1)); PGC(g, g->d_inc.ensure(2 * e1));
        PGC(g, g->d_is_free.ensure(n1)); PGC(g, g->d_Z.ensure(16 * e1)); PGC(g, g->d_Om.ensure(36 * e1));
        PGC(g, g->d_T.ensure(16 * n1)); PGC(g, g->d_Tt.ensure(16 * n1));
        const size_t bV = nbV, bE = nbE;
        const ArenaPart<double> per_edge[] = {{&G.r, 6 * e1}, {&G.W, 36 * e1}, {&G.b, 6 * e1}, {&G.echi2, e1}, {&G.t, 6 * e1}, {&G.erho, e1}, {&G.ew, e1}};
        const ArenaPart<double> per_vertex[] = {{&G.D, 36 * n1}, {&G.g, 6 * n1}, {&G.Minv, 36 * n1}, {&G.dd, 6 * n1}, {&G.x, 6 * n1}, {&G.res, 6 * n1},
                                                {&G.z, 6 * n1}, {&G.p, 6 * n1}, {&G.q, 6 * n1}};
        const ArenaPart<double> rows[] = {{&G.rows_chi2, bE}, {&G.rows_chi2_trial, bE}, {&G.rows_rz0, bV}, {&G.rows_rz, 2 * bV}, {&G.rows_pq, bV},
                                          {&G.rows_maxx, bV}, {&G.rows_bad, bV}};
        PGC(g, arena_carve(g->d_edge, per_edge));
        PGC(g, g->d_kind.ensure(e1)); PGC(g, g->d_delta.ensure(e1));
        PGC(g, arena_carve(g->d_vert, per_vertex));
        PGC(g, arena_carve(g->d_rows, rows));
        PGC(g, g->d_state.ensure(1)); PGC(g, g->h_state.ensure(1));
        if (E) {
            PGC(g, hipMemcpyAsync(g->d_ei, g->ei.data(), sizeof(int) * E, hipMemcpyHostToDevice, s));
            PGC(g, hipMemcpyAsync(g->d_ej, g->ej.data(), sizeof(int) * E, hipMemcpyHostToDevice, s));
            PGC(g, hipMemcpyAsync(g->d_inc, inc.data(), sizeof(int) * 2 * E, hipMemcpyHostToDevice, s));
            PGC(g, hipMemcpyAsync(g->d_Z, g->Z.data(), sizeof(double) * 16 * E, hipMemcpyHostToDevice, s));
            PGC(g, hipMemcpyAsync(g->d_Om, g->Om.data(), sizeof(double) * 36 * E, hipMemcpyHostToDevice, s));
        }
        PGC(g, hipMemcpyAsync(g->d_row_ptr, row_ptr.data(), sizeof(int) * (N + 1), hipMemcpyHostToDevice, s));
        PGC(g, hipMemcpyAsync(g->d_is_free, g->is_free.data(), sizeof(int) * n1, hipMemcpyHostToDevice, s));
        PGC(g, hipStreamSynchronize(s));      // row_ptr and inc are locals
        G.N = N; G.E = E; G.nbV = nbV; G.nbE = nbE;
        G.ei = g->d_ei; G.ej = g->d_ej; G.row_ptr = g->d_row_ptr; G.inc = g->d_inc; G.is_free = g->d_is_free;
        G.Z = g->d_Z; G.Om = g->d_Om; G.T = g->d_T; G.Tt = g->d_Tt;
        G.kind = g->d_kind; G.delta = g->d_delta;
        G.st = g->d_state;
        g->dirty = false;
    }
    if (settings && E) {      // two words per edge: all a change of kind or delta costs
        g->kind_up.resize(E);
        for (int e = 0; e < E; ++e) g->kind_up[e] = g->enabled[e] ? g->kind[e] : -1;
        PGC(g, hipMemcpyAsync(g->d_kind, g->kind_up.data(), sizeof(int) * E, hipMemcpyHostToDevice, s));
        PGC(g, hipMemcpyAsync(g->d_delta, g->delta.data(), sizeof(double) * E, hipMemcpyHostToDevice, s));
        PGC(g, hipStreamSynchronize(s));      // the setters may write kind_up's sources before the next launch
    }
    g->settings_dirty = false;
    if (with_A) PGC(g, g->d_A.ensure(36 * e1));
    G.A = with_A ? g->d_A.get() : nullptr;
    PGC(g, g->d_trace.ensure(std::max(max_trace, 1)));
    G.trace = g->d_trace;
    if (N) PGC(g, hipMemcpyAsync(g->d_T, g->T.data(), sizeof(double) * 16 * N, hipMemcpyHostToDevice, s));
    return 0;
}

int graph_put_state(rgbd360_graph* g, double lambda) {
    rgbd360_graph_state& S = *g->h_state.get();
    memset(&S, 0, sizeof(S));
    S.stop_it = INT_MAX;
    S.cg_stop_at = INT_MAX;
    S.lambda = lambda;
    PGC(g, hipMemcpyAsync(g->d_state, &S, sizeof(S), hipMemcpyHostToDevice, g->ctx->stream));
    return 0;
}

// The cost at the current poses: the edge kernel's partial rows, re-added here in ascending order like every device consumer does;
// per edge (each may be null) the raw s, rho and w
int graph_chi2_now(rgbd360_graph* g, double* chi2, double* per_edge, double* rho = nullptr, double* w = nullptr) {
    const int E = g->E();
    *chi2 = 0.0;
    if (!E) return 0;
    hipStream_t s = g->ctx->stream;
    const PgDev& G = g->G;
    hipLaunchKernelGGL(pg::k_pg_edges<2>, dim3(G.nbE), dim3(pg::kBlock), 0, s, G, -1);
    PGC(g, hipGetLastError());
    std::vector<double> rows(G.nbE);
    PGC(g, hipMemcpyAsync(rows.data(), G.rows_chi2_trial, sizeof(double) * G.nbE, hipMemcpyDeviceToHost, s));
    if (per_edge) PGC(g, hipMemcpyAsync(per_edge, G.echi2, sizeof(double) * E, hipMemcpyDeviceToHost, s));
    if (rho) PGC(g, hipMemcpyAsync(rho, G.erho, sizeof(double) * E, hipMemcpyDeviceToHost, s));
    if (w) PGC(g, hipMemcpyAsync(w, G.ew, sizeof(double) * E, hipMemcpyDeviceToHost, s));
    PGC(g, hipStreamSynchronize(s));
    for (int k = 0; k < G.nbE; ++k) *chi2 += rows[k];
    return 0;
}

}  // namespace

extern "C" {

int rgbd360_graph_create(rgbd360_ctx* ctx, rgbd360_graph** out) {
    if (!out) return -1;
    *out = nullptr;
    if (!ctx) return -1;
    rgbd360_graph* g = new rgbd360_graph();
    g->ctx = ctx;
    *out = g;
    return 0;
}

void rgbd360_graph_destroy(rgbd360_graph* g) {
    if (!g) return;
    hipSetDevice(g->ctx->p.device);
    (void)hipStreamSynchronize(g->ctx->stream);
    delete g;
}

const char* rgbd360_graph_last_error(rgbd360_graph* g) { return g ? g->err.c_str() : "null graph"; }

int rgbd360_graph_n_vertices(const rgbd360_graph* g) { return g ? g->N() : -1; }
int rgbd360_graph_n_edges(const rgbd360_graph* g) { return g ? g->E() : -1; }

int rgbd360_graph_clear(rgbd360_graph* g) {
    if (!g) return -1;
    g->T.clear(); g->fixed.clear(); g->ei.clear(); g->ej.clear(); g->Z.clear(); g->Om.clear(); g->trace.clear();
    g->kind.clear(); g->delta.clear(); g->enabled.clear();
    g->dirty = true;
    return 0;
}

int rgbd360_graph_add_vertices(rgbd360_graph* g, int n, const float* poses, const uint8_t* fixed) {
    if (!g) return -1;
    if (n < 0) return graph_fail(g, -1, "n must be >= 0");
    const int first = g->N();
    if (n == 0) return first;
    if (!poses) return graph_fail(g, -1, "null pointer");
    if ((long long)first + n > (1 << 28)) return graph_fail(g, -1, "a graph holds at most 2^28 vertices");
    for (int k = 0; k < n; ++k)
        if (!pg_finite(poses + (size_t)16 * k, 16)) return graph_fail(g, -1, "vertex " + std::to_string(k) + ": the pose has a non-finite entry");
    for (int k = 0; k < n; ++k) {
        for (int m = 0; m < 16; ++m) g->T.push_back((double)poses[(size_t)16 * k + m]);
        g->fixed.push_back(fixed && fixed[k] ? 1 : 0);
    }
    g->dirty = true;
    return first;
}

int rgbd360_graph_add_edges(rgbd360_graph* g, int n, const int* from, const int* to, const float* rel_poses, const float* information) {
    if (!g) return -1;
    if (n < 0) return graph_fail(g, -1, "n must be >= 0");
    if (n == 0) return 0;
    if (!from || !to || !rel_poses) return graph_fail(g, -1, "null pointer");
    if ((long long)g->E() + n > (1 << 28)) return graph_fail(g, -1, "a graph holds at most 2^28 edges");
    const int N = g->N();
    for (int k = 0; k < n; ++k) {      // all of them before anything is added: an index never reaches a kernel unchecked
        const std::string who = "edge " + std::to_string(k) + ": ";
        if (from[k] < 0 || from[k] >= N) return graph_fail(g, -1, who + "from = " + std::to_string(from[k]) + " is no vertex");
        if (to[k] < 0 || to[k] >= N) return graph_fail(g, -1, who + "to = " + std::to_string(to[k]) + " is no vertex");
        if (from[k] == to[k]) return graph_fail(g, -1, who + "from == to");
        if (!pg_finite(rel_poses + (size_t)16 * k, 16)) return graph_fail(g, -1, who + "the relative pose has a non-finite entry");
        if (information) {
            const float* I = information + (size_t)36 * k;
            if (!pg_finite(I, 36)) return graph_fail(g, -1, who + "the information matrix has a non-finite entry");
            for (int d = 0; d < 6; ++d)
                if (!(I[d * 7] > 0.f)) return graph_fail(g, -1, who + "the information matrix has a non-positive diagonal entry");
        }
    }
    for (int k = 0; k < n; ++k) {
        g->ei.push_back(from[k]);
        g->ej.push_back(to[k]);
        g->kind.push_back(RGBD360_GRAPH_ROBUST_NONE);
        g->delta.push_back(1.0);
        g->enabled.push_back(1);
        for (int m = 0; m < 16; ++m) g->Z.push_back((double)rel_poses[(size_t)16 * k + m]);
        for (int c = 0; c < 6; ++c)
            for (int r = 0; r < 6; ++r)
                g->Om.push_back(information ? 0.5 * ((double)information[(size_t)36 * k + c * 6 + r] + (double)information[(size_t)36 * k + r * 6 + c])
                                            : (r == c ? 1.0 : 0.0));
    }
    g->dirty = true;
    return 0;
}

int rgbd360_graph_set_poses(rgbd360_graph* g, int first, int n, const float* poses) {
    if (!g) return -1;
    if (n < 0 || first < 0 || (long long)first + n > g->N()) return graph_fail(g, -1, "vertex range outside the graph");
    if (n == 0) return 0;
    if (!poses) return graph_fail(g, -1, "null pointer");
    for (int k = 0; k < n; ++k)
        if (!pg_finite(poses + (size_t)16 * k, 16)) return graph_fail(g, -1, "vertex " + std::to_string(first + k) + ": the pose has a non-finite entry");
    for (size_t m = 0; m < (size_t)16 * n; ++m) g->T[(size_t)16 * first + m] = (double)poses[m];
    return 0;
}

int rgbd360_graph_set_fixed(rgbd360_graph* g, int first, int n, const uint8_t* fixed) {
    if (!g) return -1;
    if (n < 0 || first < 0 || (long long)first + n > g->N()) return graph_fail(g, -1, "vertex range outside the graph");
    if (n == 0) return 0;
    if (!fixed) return graph_fail(g, -1, "null pointer");
    for (int k = 0; k < n; ++k) g->fixed[first + k] = fixed[k] ? 1 : 0;
    g->dirty = true;
    return 0;
}

int rgbd360_graph_get_poses(rgbd360_graph* g, int first, int n, float* out) {
    if (!g) return -1;
    if (n < 0 || first < 0 || (long long)first + n > g->N()) return graph_fail(g, -1, "vertex range outside the graph");
    if (n == 0) return 0;
    if (!out) return graph_fail(g, -1, "null pointer");
    for (size_t m = 0; m < (size_t)16 * n; ++m) out[m] = (float)g->T[(size_t)16 * first + m];
    return 0;
}

void rgbd360_graph_default_params(rgbd360_graph_params* p) {
    if (!p) return;
    p->max_iters = 10;
    p->cg_max_iters = 400;
    p->tol_update = 1e-6;
    p->lambda_init = 1e-3;
    p->lambda_max = 1e30;
    p->cg_tol = 1e-8;
}

int rgbd360_graph_chi2(rgbd360_graph* g, double* chi2, double* per_edge) {
    if (!g) return -1;
    if (!chi2) return graph_fail(g, -1, "null pointer");
    int rc = graph_upload(g, false, 0);
    if (rc) return rc;
    return graph_chi2_now(g, chi2, per_edge);
}

int rgbd360_graph_set_edge_robust(rgbd360_graph* g, int first, int n, const int* kinds, const double* deltas) {
    if (!g) return -1;
    if (n < 0 || first < 0 || (long long)first + n > g->E()) return graph_fail(g, -1, "edge range outside the graph");
    if (n == 0) return 0;
    if (!kinds) return graph_fail(g, -1, "null pointer");
    for (int k = 0; k < n; ++k) {      // all of them before anything changes
        const std::string who = "edge " + std::to_string(first + k) + ": ";
        if (kinds[k] < RGBD360_GRAPH_ROBUST_NONE || kinds[k] > RGBD360_GRAPH_ROBUST_GEMAN_MCCLURE)
            return graph_fail(g, -1, who + "kind = " + std::to_string(kinds[k]) + " is no robust kind");
        if (kinds[k] != RGBD360_GRAPH_ROBUST_NONE) {
            if (!deltas) return graph_fail(g, -1, who + "a robust kind needs a delta (null pointer)");
            if (!std::isfinite(deltas[k]) || !(deltas[k] > 0.0)) return graph_fail(g, -1, who + "delta must be finite and > 0");
        }
    }
    for (int k = 0; k < n; ++k) {
        g->kind[first + k] = kinds[k];
        if (deltas && kinds[k] != RGBD360_GRAPH_ROBUST_NONE) g->delta[first + k] = deltas[k];
    }
    g->settings_dirty = true;
    return 0;
}

int rgbd360_graph_set_edge_enabled(rgbd360_graph* g, int first, int n, const uint8_t* enabled) {
    if (!g) return -1;
    if (n < 0 || first < 0 || (long long)first + n > g->E()) return graph_fail(g, -1, "edge range outside the graph");
    if (n == 0) return 0;
    if (!enabled) return graph_fail(g, -1, "null pointer");
    for (int k = 0; k < n; ++k) {
        const char en = enabled[k] ? 1 : 0;
        if (g->enabled[first + k] != en) {      // the incidence lists are built again at the next call that runs a kernel
            g->enabled[first + k] = en;
            g->dirty = true;
        }
    }
    return 0;
}

int rgbd360_graph_get_edge_state(rgbd360_graph* g, int first, int n, int* kinds, double* deltas, uint8_t* enabled) {
    if (!g) return -1;
    if (n < 0 || first < 0 || (long long)first + n > g->E()) return graph_fail(g, -1, "edge range outside the graph");
    for (int k = 0; k < n; ++k) {
        if (kinds) kinds[k] = g->kind[first + k];
        if (deltas) deltas[k] = g->delta[first + k];
        if (enabled) enabled[k] = g->enabled[first + k] ? 1 : 0;
    }
    return 0;
}

int rgbd360_graph_edge_weights(rgbd360_graph* g, double* cost, double* s, double* rho, double* w) {
    if (!g) return -1;
    int rc = graph_upload(g, false, 0);
    if (rc) return rc;
    double c = 0.0;
    rc = graph_chi2_now(g, &c, s, rho, w);
    if (cost) *cost = c;
    return rc;
}

int rgbd360_graph_optimize(rgbd360_graph* g, const rgbd360_graph_params* params, rgbd360_graph_result* result) {
    if (!g) return -1;
    rgbd360_graph_params P;
    rgbd360_graph_default_params(&P);
    if (params) P = *params;
    if (P.max_iters < 0 || P.max_iters > 10000) return graph_fail(g, -1, "max_iters must be in 0..10000");
    if (P.cg_max_iters < 1 || P.cg_max_iters > 100000) return graph_fail(g, -1, "cg_max_iters must be in 1..100000");
    if (!(P.lambda_init > 0.0) || !(P.lambda_max >= P.lambda_init) || !(P.cg_tol >= 0.0) || !(P.tol_update >= 0.0))
        return graph_fail(g, -1, "lambda_init must be > 0, lambda_max >= lambda_init, cg_tol and tol_update >= 0");
    const int N = g->N(), E = g->E();
    bool any_fixed = false;
    for (int v = 0; v < N; ++v) any_fixed |= g->fixed[v] != 0;
    if (N > 0 && !any_fixed) return graph_fail(g, -1, "the graph has no fixed vertex: its poses are determined up to a rigid motion only");
    g->trace.clear();
    rgbd360_graph_result R;
    memset(&R, 0, sizeof(R));
    R.lambda_final = P.lambda_init;
    int rc = graph_upload(g, false, P.max_iters);
    if (rc) return rc;
    R.n_fixed = g->n_fixed;
    R.n_isolated = g->n_isolated;
    if (N == 0 || E == 0 || g->n_free == 0 || P.max_iters == 0) {      // nothing to move
        rc = graph_chi2_now(g, &R.chi2_initial, nullptr);
        if (rc) return rc;
        R.chi2_final = R.chi2_initial;
        if (result) *result = R;
        return 0;
    }
    hipStream_t s = g->ctx->stream;
    const PgDev& G = g->G;
    rc = graph_put_state(g, P.lambda_init);
    if (rc) return rc;
    const PgCg C = graph_cg(G);
    const dim3 blk(pg::kBlock), gv(G.nbV), ge(G.nbE);
    const rgbd360_graph_state& S = *g->h_state.get();
    for (int it = 0; it < P.max_iters; ++it) {
        hipLaunchKernelGGL(pg::k_pg_edges<0>, ge, blk, 0, s, G, it);
        hipLaunchKernelGGL(pg::k_pg_assemble, gv, blk, 0, s, G, it);
        for (int k = 0; k < P.cg_max_iters; ++k) cg_launch_iteration(s, G, C, it, k, P.cg_tol, false);
        hipLaunchKernelGGL(pg::k_pg_trial, gv, blk, 0, s, G, it);
        hipLaunchKernelGGL(pg::k_pg_edges<1>, ge, blk, 0, s, G, it);
        hipLaunchKernelGGL(pg::k_pg_decide, gv, blk, 0, s, G, it, P.max_iters, P.tol_update, P.lambda_max);
        PGC(g, hipGetLastError());
        // the one synchronisation of the iteration: the host stops enqueuing when the loop has ended
        PGC(g, hipMemcpyAsync(g->h_state.get(), g->d_state, sizeof(rgbd360_graph_state), hipMemcpyDeviceToHost, s));
        PGC(g, hipStreamSynchronize(s));
        if (S.stop_it <= it + 1) break;
    }
    g->trace.resize(S.iterations);
    if (S.iterations) PGC(g, hipMemcpyAsync(g->trace.data(), g->d_trace, sizeof(rgbd360_graph_iteration) * S.iterations, hipMemcpyDeviceToHost, s));
    PGC(g, hipMemcpyAsync(g->T.data(), g->d_T, sizeof(double) * 16 * N, hipMemcpyDeviceToHost, s));
    PGC(g, hipStreamSynchronize(s));
    R.status = S.status; R.iterations = S.iterations; R.accepted = S.accepted; R.converged = S.converged;
    R.chi2_initial = S.chi2_initial; R.chi2_final = S.iterations ? S.chi2_final : S.chi2_initial; R.lambda_final = S.lambda;
    R.cg_iterations = S.cg_total;
    if (result) *result = R;
    return R.status;
}

int rgbd360_graph_get_trace(rgbd360_graph* g, int max_trace, int* n_trace, rgbd360_graph_iteration* trace) {
    if (!g) return -1;
    if (n_trace) *n_trace = (int)g->trace.size();
    if (trace)
        for (int k = 0; k < max_trace && k < (int)g->trace.size(); ++k) trace[k] = g->trace[k];
    return 0;
}

int rgbd360_graph_linearize(rgbd360_graph* g, double* r, double* A) {
    if (!g) return -1;
    int rc = graph_upload(g, true, 0);
    if (rc) return rc;
    const int E = g->E();
    if (!E) return 0;
    hipStream_t s = g->ctx->stream;
    rc = graph_put_state(g, 0.0);
    if (rc) return rc;
    hipLaunchKernelGGL(pg::k_pg_edges<0>, dim3(g->G.nbE), dim3(pg::kBlock), 0, s, g->G, -1);
    PGC(g, hipGetLastError());
    if (r) PGC(g, hipMemcpyAsync(r, g->G.r, sizeof(double) * 6 * E, hipMemcpyDeviceToHost, s));
    if (A) PGC(g, hipMemcpyAsync(A, g->G.A, sizeof(double) * 36 * E, hipMemcpyDeviceToHost, s));
    PGC(g, hipStreamSynchronize(s));
    return 0;
}

int rgbd360_graph_apply(rgbd360_graph* g, double lambda, const double* x, double* y) {
    if (!g) return -1;
    if (!x || !y) return graph_fail(g, -1, "null pointer");
    if (!(lambda >= 0.0)) return graph_fail(g, -1, "lambda must be >= 0");
    int rc = graph_upload(g, false, 0);
    if (rc) return rc;
    const int N = g->N(), E = g->E();
    for (size_t k = 0; k < (size_t)6 * N; ++k) y[k] = 0.0;
    if (!N || !E) return 0;
    hipStream_t s = g->ctx->stream;
    const PgDev& G = g->G;
    rc = graph_put_state(g, lambda);
    if (rc) return rc;
    std::vector<double> p((size_t)6 * N);
    for (int v = 0; v < N; ++v)
        for (int i = 0; i < 6; ++i) p[(size_t)6 * v + i] = g->is_free[v] ? x[(size_t)6 * v + i] : 0.0;
    const dim3 blk(pg::kBlock), gv(G.nbV), ge(G.nbE);
    hipLaunchKernelGGL(pg::k_pg_edges<0>, ge, blk, 0, s, G, -1);
    hipLaunchKernelGGL(pg::k_pg_assemble, gv, blk, 0, s, G, -1);
    PGC(g, hipMemcpyAsync(G.p, p.data(), sizeof(double) * 6 * N, hipMemcpyHostToDevice, s));
    const PgCg C = graph_cg(G);
    hipLaunchKernelGGL(pg::k_pg_cg_edge<false>, ge, blk, 0, s, G, C, -1, 0);
    hipLaunchKernelGGL(pg::k_pg_cg_gather, gv, blk, 0, s, G, C, -1, 0);
    PGC(g, hipGetLastError());
    PGC(g, hipMemcpyAsync(y, G.q, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, s));
    PGC(g, hipStreamSynchronize(s));      // (p is a local)
    return 0;
}

int rgbd360_graph_time_kernels(rgbd360_graph* g, int reps, float avg_us[10]) {
    if (!g) return -1;
    if (!avg_us || reps < 1) return graph_fail(g, -1, "bad arguments");
    int rc = graph_upload(g, false, 1);
    if (rc) return rc;
    for (int k = 0; k < 10; ++k) avg_us[k] = 0.f;
    if (!g->N() || !g->E()) return 0;
    hipStream_t s = g->ctx->stream;
    const PgDev& G = g->G;
    rc = graph_put_state(g, 1e-3);
    if (rc) return rc;
    const PgCg C = graph_cg(G);
    const dim3 blk(pg::kBlock), gv(G.nbV), ge(G.nbE);
    const double inf = HUGE_VAL;
    auto launch = [&](int which) {
        switch (which) {
            case 0: hipLaunchKernelGGL(pg::k_pg_edges<0>, ge, blk, 0, s, G, 0); break;
            case 1: hipLaunchKernelGGL(pg::k_pg_assemble, gv, blk, 0, s, G, 0); break;
            case 2: hipLaunchKernelGGL(pg::k_pg_cg_edge<false>, ge, blk, 0, s, G, C, 0, 0); break;
            case 3: hipLaunchKernelGGL(pg::k_pg_cg_gather, gv, blk, 0, s, G, C, 0, 0); break;
            case 4: hipLaunchKernelGGL(pg::k_pg_cg_update, gv, blk, 0, s, G, C, 0, 0); break;
            case 5: hipLaunchKernelGGL(pg::k_pg_cg_dir, gv, blk, 0, s, G, C, 0, 0, 0.0); break;
            case 6: hipLaunchKernelGGL(pg::k_pg_trial, gv, blk, 0, s, G, 0); break;
            case 7: hipLaunchKernelGGL(pg::k_pg_edges<1>, ge, blk, 0, s, G, 0); break;
            case 8: hipLaunchKernelGGL(pg::k_pg_decide, gv, blk, 0, s, G, 0, INT_MAX, -1.0, inf); break;
            default: hipLaunchKernelGGL(pg::k_pg_cg_edge<false>, ge, blk, 0, s, G, C, 0, 0); break;
        }
    };
    auto prepare = [&](int which) {      // slot 9: the loop has ended, every launch returns on the state word
        if (which != 9) return 0;
        g->h_state.get()->stop_it = 0;
        PGC(g, hipMemcpyAsync(g->d_state, g->h_state.get(), sizeof(rgbd360_graph_state), hipMemcpyHostToDevice, s));
        return 0;
    };
    return graph_time_slots(g, 10, reps, avg_us, launch, prepare);
}

}  // extern "C"
