// rig_calib.h -- the rig's sensor extrinsics (and optionally the rig poses of a keyframe window) calibrated against the resident voxel
// map: K frames x S sensors, input (k, s) the cloud of sensor s in frame k, every input evaluated at P_ks = T_k E_s by the unchanged
// batched point-to-plane launch (map_align_batch.h), one unknown per free sensor shared over all frames and, with refine_poses, one per
// frame shared over all sensors.  What Calib360::loadExtrinsicCalibration reads (Rt_0N.txt) this writes.  Part of the Frame360
// translation unit, behind map_align_batch.h.
//
// Definition (include/rgbd360_hip.h, "the rig's extrinsics against the map"; tests/rig_calib_reference.py restates it in
// numpy).  The solve arithmetic -- the adjoint, the blocks of an input, the 6 x 6 Cholesky of a frame, the reduced Cholesky, the
// substitutions and the update -- is ONE __host__ __device__ text, written over a `Par` (the lanes that share a loop and their barrier:
// Serial on the host, Block in a kernel).  A lane computes an element with the same operations in the same order whoever runs the loop,
// so the host build (rgbd360_rig_calib_solve_host) and the kernels (rgbd360_rig_calib_solve_dev) give the same bytes.  Float64 with
// + - x / sqrt, every operation rounded on its own (the units are built without contraction).
//
//   k_rig_pinhole_cloud   all K S pinhole depth images of a _depth call into packed clouds, one launch: f = ((u - cx) / fx, (v - cy) / fy, 1)
//                         in float32, the point z f; a pixel without a measurement a NaN triple.
//                         (its pixel is pinhole_pixel, which depth_apply.h's k_rig_cloud_models instantiates with a correction of z.)
//   k_rig_init            one launch: the head, the inputs' records and, per live input, its loop state at P_ks = T_k E_s (gn::mat4_mul).
//   k_rig_input           one 64-lane workgroup per live input: the partial rows added in ascending order (the first loop of
//                         icp_solve_rows on the 30 sums), then lane 0: A, b, A Ad, Ad^T A Ad, Ad^T b.
//   k_rig_frames          one lane per frame: F_k, f_k, with refine_poses the 6 x 6 Cholesky, L^-1 f_k and L^-1 C_ks.
//   k_rig_solve           ONE workgroup: totals and statuses, the reduced matrix (packed lower triangle in LDS: 96 x 97 / 2 doubles),
//                         Cholesky, the substitutions, the updates applied, the new P_ks into the inputs' states, the trace and the stop test.
//   host                  one init, max_iters x (evaluation, k_rig_input, k_rig_frames, k_rig_solve), the final pass, one copy, ONE
//                         synchronisation: 4 max_iters + 5 launches whatever K and S are.
// No floating-point atomics, no inline assembly.
#pragma once
#include <cstdio>
#include <string>

namespace rigc {

constexpr int kRow = 30;                                 // the sums of a point-to-plane row in front of its counters
constexpr int kMaxSensors = RGBD360_RIG_CALIB_MAX_SENSORS;
constexpr int kMaxN = 6 * kMaxSensors;                   // the reduced system: 6 per free sensor
constexpr int kPacked = kMaxN * (kMaxN + 1) / 2;
constexpr double kPivot = 1e-12;                         // a pivot <= kPivot x its undamped diagonal entry: ill-posed (a setting)

struct Serial {
    GN_HD int lane() const { return 0; }
    GN_HD int lanes() const { return 1; }
    GN_HD void sync() const {}
};
#if defined(__HIPCC__)
struct Block {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return (int)blockDim.x; }
    __device__ void sync() const { __syncthreads(); }
};
#endif

// what the solve keeps of input (k, s); 6 x 6 blocks column-major
struct Input {
    double A[36], b[6];          // the normal equations of the input in the world-left parameterisation
    double C[36];                // A Ad_k
    double G[36], gs[6];         // Ad_k^T A Ad_k, Ad_k^T b
    double W[36];                // L_k^-1 C (frames that are eliminated)
    double n, rr;
    int used, pad;
};
struct Frame {
    double L[36], z[6];          // the Cholesky factor of F_k + lambda diag F_k (lower, column-major), L^-1 f_k
    int has, elim, ill, pad;     // a contributing input; eliminated (refine_poses and has); a pivot failed
};
struct Head {
    int done, status, iterations, converged, n_inputs_used, n_frames_skipped;
    float max_vv, max_ww;
    long long n_matched;
    double cost;
};
struct Settings {
    int K, S, refine, fixed;
    double lambda;
    long long min_input, min_matches;
    float eps;
    int pad;
};
// the problem as the one text sees it: the same on the host and in device memory
struct Problem {
    Settings set;
    float* T;                    // [16 K] world <- rig
    float* E;                    // [16 S] rig <- sensor
    Input* in;                   // [K S]
    Frame* fr;                   // [K]
    float* upd;                  // [6 (K + S)]: delta_k, then epsilon_s, as applied (float32; zeros where none)
    Head* head;
    rgbd360_rig_calib_step* trace;
    rgbd360_rig_calib_sensor* sensors;      // [S], the final pass; may be null
};

GN_HD inline int free_slot(const Settings& s, int sensor) { return s.fixed < 0 || sensor < s.fixed ? sensor : sensor - 1; }
GN_HD inline int free_count(const Settings& s) { return s.fixed < 0 ? s.S : s.S - 1; }
GN_HD inline int sensor_of_slot(const Settings& s, int slot) { return s.fixed < 0 || slot < s.fixed ? slot : slot + 1; }
GN_HD inline int packed(int i, int j) { return i * (i + 1) / 2 + j; }      // i >= j

// column t of the partial rows, added in ascending order
GN_HD inline double sum_rows(const double* part, int n_rows, int stride, int t) {
    double s = 0.0;
    for (int r = 0; r < n_rows; ++r) s += part[(size_t)r * stride + t];
    return s;
}

// Ad(T) in float64 from the float32 pose
GN_HD inline void adjoint_of(const float* T, double* Ad) {
    double Td[16];
    for (int k = 0; k < 16; ++k) Td[k] = (double)T[k];
    gn::se3_adjoint(Td, Ad);
}

// the blocks of one input from its 30 sums; sums of products ascend from 0.0
GN_HD inline void input_blocks(const double* row, long long min_input, const double* Ad, Input& in) {
    int h = 1;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++h) in.A[b * 6 + a] = in.A[a * 6 + b] = row[h];
    for (int k = 0; k < 6; ++k) in.b[k] = row[22 + k];
    in.n = row[0];
    in.rr = row[28];
    in.used = (long long)row[0] >= min_input ? 1 : 0;
    gn::mat6_mul(in.A, Ad, in.C);
    for (int c = 0; c < 6; ++c)
        for (int r = 0; r < 6; ++r) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += Ad[r * 6 + k] * in.C[c * 6 + k];
            in.G[c * 6 + r] = s;
        }
    for (int r = 0; r < 6; ++r) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += Ad[r * 6 + k] * in.b[k];
        in.gs[r] = s;
    }
}

// frame k: F_k = sum_s A_ks and f_k = -sum_s b_ks over the contributing inputs, s ascending; with refine_poses the Cholesky of
// F_k + lambda diag F_k column by column (element (i, j), i >= j: F_ij - sum_{p < j} L_ip L_jp, p ascending; the diagonal's square
// root, the others divided by it), z = L^-1 f_k and W_ks = L^-1 C_ks by forward substitution (p ascending)
GN_HD inline void frame_eliminate(const Problem& P, int k) {
    const Settings& set = P.set;
    Frame& fr = P.fr[k];
    double F[36], f[6], d0[6];
    for (int e = 0; e < 36; ++e) F[e] = 0.0;
    for (int e = 0; e < 6; ++e) f[e] = 0.0;
    int has = 0;
    for (int s = 0; s < set.S; ++s) {
        const Input& in = P.in[(size_t)k * set.S + s];
        if (!in.used) continue;
        has = 1;
        for (int e = 0; e < 36; ++e) F[e] += in.A[e];
        for (int e = 0; e < 6; ++e) f[e] += in.b[e];
    }
    fr.has = has;
    fr.elim = has && set.refine ? 1 : 0;
    fr.ill = 0;
    if (!fr.elim) return;
    for (int e = 0; e < 6; ++e) f[e] = -f[e];
    for (int i = 0; i < 6; ++i) {
        d0[i] = F[i * 6 + i];
        F[i * 6 + i] = d0[i] + set.lambda * d0[i];
    }
    double* L = fr.L;
    for (int e = 0; e < 36; ++e) L[e] = 0.0;
    for (int j = 0; j < 6; ++j)
        for (int i = j; i < 6; ++i) {
            double s = F[j * 6 + i];
            for (int p = 0; p < j; ++p) s -= L[p * 6 + i] * L[p * 6 + j];
            if (i == j) {
                if (!(s > kPivot * d0[j])) {
                    fr.ill = 1;
                    return;
                }
                L[j * 6 + j] = sqrt(s);
            } else {
                L[j * 6 + i] = s / L[j * 6 + j];
            }
        }
    for (int i = 0; i < 6; ++i) {
        double s = f[i];
        for (int p = 0; p < i; ++p) s -= L[p * 6 + i] * fr.z[p];
        fr.z[i] = s / L[i * 6 + i];
    }
    for (int sn = 0; sn < set.S; ++sn) {
        Input& in = P.in[(size_t)k * set.S + sn];
        if (!in.used || sn == set.fixed) continue;
        for (int c = 0; c < 6; ++c)
            for (int i = 0; i < 6; ++i) {
                double s = in.C[c * 6 + i];
                for (int p = 0; p < i; ++p) s -= L[p * 6 + i] * in.W[c * 6 + p];
                in.W[c * 6 + i] = s / L[i * 6 + i];
            }
    }
}

// The reduced system of the free sensors, n = 6 F unknowns: M (packed lower triangle), rhs, d0 and tmp are the caller's work arrays
// (LDS in the kernel).  Element (i, j), i >= j, a = i % 6, c = j % 6, of sensors si and sj:
//   M_ij   = [si == sj] sum_k G_ks(a, c)  -  sum_k sum_{r < 6} W_k,si(r, a) W_k,sj(r, c)      (k ascending, contributing inputs; the second
//            sum over the eliminated frames, each frame's six products summed from 0.0 before they are subtracted)
//   rhs_i  = -(sum_k gs_ks(a))  -  sum_k sum_r W_k,si(r, a) z_k(r)
// then d0 = diag M, M_ii = d0_i + lambda d0_i, the Cholesky column by column as in frame_eliminate, L y = rhs (column j: y_j = rhs_j / L_jj,
// rhs_i -= L_ij y_j for i > j) and L^T x = y (column j descending: x_j = y_j / L_jj, y_i -= L_ji x_j for i < j).  x is left in rhs.
// *ill is set (by every lane alike) when a pivot fails.
template <class Par>
GN_HD inline void reduced_solve(const Par& par, const Problem& P, double* M, double* rhs, double* d0, double* tmp, int* ill) {
    const Settings& set = P.set;
    const int n = 6 * free_count(set), K = set.K, S = set.S;
    for (int q = par.lane(); q < n * n; q += par.lanes()) {
        const int i = q / n, j = q % n;
        if (j > i) continue;
        const int si = sensor_of_slot(set, i / 6), sj = sensor_of_slot(set, j / 6), a = i % 6, c = j % 6;
        double acc = 0.0;
        if (si == sj)
            for (int k = 0; k < K; ++k) {
                const Input& in = P.in[(size_t)k * S + si];
                if (in.used) acc += in.G[c * 6 + a];
            }
        for (int k = 0; k < K; ++k) {
            if (!P.fr[k].elim) continue;
            const Input &ii = P.in[(size_t)k * S + si], &ij = P.in[(size_t)k * S + sj];
            if (!ii.used || !ij.used) continue;
            double s = 0.0;
            for (int r = 0; r < 6; ++r) s += ii.W[a * 6 + r] * ij.W[c * 6 + r];
            acc -= s;
        }
        M[packed(i, j)] = acc;
    }
    for (int i = par.lane(); i < n; i += par.lanes()) {
        const int si = sensor_of_slot(set, i / 6), a = i % 6;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) {
            const Input& in = P.in[(size_t)k * S + si];
            if (in.used) acc += in.gs[a];
        }
        acc = -acc;
        for (int k = 0; k < K; ++k) {
            const Input& in = P.in[(size_t)k * S + si];
            if (!P.fr[k].elim || !in.used) continue;
            double s = 0.0;
            for (int r = 0; r < 6; ++r) s += in.W[a * 6 + r] * P.fr[k].z[r];
            acc -= s;
        }
        rhs[i] = acc;
    }
    par.sync();
    for (int i = par.lane(); i < n; i += par.lanes()) {
        d0[i] = M[packed(i, i)];
        M[packed(i, i)] = d0[i] + set.lambda * d0[i];
    }
    par.sync();
    for (int j = 0; j < n; ++j) {
        for (int i = j + par.lane(); i < n; i += par.lanes()) {
            double s = M[packed(i, j)];
            for (int p = 0; p < j; ++p) s -= M[packed(i, p)] * M[packed(j, p)];
            tmp[i] = s;
        }
        par.sync();
        const double piv = tmp[j];
        if (!(piv > kPivot * d0[j])) {       // (the same value in every lane)
            *ill = 1;
            return;
        }
        const double d = sqrt(piv);
        for (int i = j + par.lane(); i < n; i += par.lanes()) M[packed(i, j)] = i == j ? d : tmp[i] / d;
        par.sync();
    }
    for (int j = 0; j < n; ++j) {
        const double y = rhs[j] / M[packed(j, j)];
        par.sync();
        for (int i = j + par.lane(); i < n; i += par.lanes()) {
            if (i == j) rhs[j] = y;
            else rhs[i] -= M[packed(i, j)] * y;
        }
        par.sync();
    }
    for (int j = n - 1; j >= 0; --j) {
        const double x = rhs[j] / M[packed(j, j)];
        par.sync();
        for (int i = par.lane(); i <= j; i += par.lanes()) {
            if (i == j) rhs[j] = x;
            else rhs[i] -= M[packed(j, i)] * x;
        }
        par.sync();
    }
}

// pose <- pseudo_exp(u) pose with gn_math.h's pseudo-exponential and 4 x 4 product; v.v and w.w of the float32 update
GN_HD inline void apply_update(const double* x, float* pose, float* u_out, float& vv, float& ww) {
    float u[6], Ef[16], out[16];
    double ud[6], Ed[16];
    for (int e = 0; e < 6; ++e) {
        u[e] = (float)x[e];
        ud[e] = (double)u[e];
        u_out[e] = u[e];
    }
    gn::se3_pseudo_exp(ud, Ed);
    for (int e = 0; e < 16; ++e) Ef[e] = (float)Ed[e];
    gn::mat4_mul(Ef, pose, out);
    for (int e = 0; e < 16; ++e) pose[e] = out[e];
    vv = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    ww = (u[3] * u[3] + u[4] * u[4]) + u[5] * u[5];
}

// the updates applied: epsilon_s from x (the reduced solution) to E_s; then per eliminated frame L^T delta_k = z_k - sum_s W_ks epsilon_s
// (s ascending over the free contributing sensors; per row the six products subtracted one after another, c ascending; the back
// substitution with p descending) to T_k.  vvww: [2 (K + S)] the v.v and w.w of every block.
template <class Par>
GN_HD inline void apply_updates(const Par& par, const Problem& P, const double* x, float* vvww) {
    const Settings& set = P.set;
    const int K = set.K, S = set.S;
    for (int s = par.lane(); s < S; s += par.lanes()) {
        float* u = P.upd + 6 * (size_t)(K + s);
        float &vv = vvww[2 * (K + s)], &ww = vvww[2 * (K + s) + 1];
        vv = ww = 0.f;
        for (int e = 0; e < 6; ++e) u[e] = 0.f;
        if (s != set.fixed) apply_update(x + 6 * free_slot(set, s), P.E + 16 * (size_t)s, u, vv, ww);
    }
    for (int k = par.lane(); k < K; k += par.lanes()) {
        float* u = P.upd + 6 * (size_t)k;
        float &vv = vvww[2 * k], &ww = vvww[2 * k + 1];
        vv = ww = 0.f;
        for (int e = 0; e < 6; ++e) u[e] = 0.f;
        const Frame& fr = P.fr[k];
        if (!fr.elim) continue;
        double v[6], d[6];
        for (int e = 0; e < 6; ++e) v[e] = fr.z[e];
        for (int s = 0; s < S; ++s) {
            const Input& in = P.in[(size_t)k * S + s];
            if (!in.used || s == set.fixed) continue;
            const double* xs = x + 6 * free_slot(set, s);
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) v[r] -= in.W[c * 6 + r] * xs[c];
        }
        for (int i = 5; i >= 0; --i) {
            double s = v[i];
            for (int p = 5; p > i; --p) s -= fr.L[i * 6 + p] * d[p];
            d[i] = s / fr.L[i * 6 + i];
        }
        apply_update(d, P.T + 16 * (size_t)k, u, vv, ww);
    }
    par.sync();
}

// One solve step of the call (or its final pass) after the inputs' blocks and the frames: the totals, the statuses, the reduced solve,
// the updates, the trace and the stop test.  Work arrays as in reduced_solve; vvww [2 (K + S)] and flag[2] shared by the lanes.
// Returns nothing: the head says what happened.  Lane 0 alone writes the head.
template <class Par>
GN_HD inline void solve_step(const Par& par, const Problem& P, int final_pass, double* M, double* rhs, double* d0, double* tmp, float* vvww, int* flag) {
    const Settings& set = P.set;
    const int K = set.K, S = set.S;
    Head& head = *P.head;
    if (par.lane() == 0) {
        long long n = 0;
        double cost = 0.0;
        int used = 0, skipped = 0, ill = 0;
        for (int i = 0; i < K * S; ++i) {
            const Input& in = P.in[i];
            if (!in.used) continue;
            used += 1;
            n += (long long)in.n;
            cost += in.rr;
        }
        for (int k = 0; k < K; ++k) {
            skipped += P.fr[k].has ? 0 : 1;
            ill |= P.fr[k].ill;
        }
        head.n_inputs_used = used;
        head.n_frames_skipped = skipped;
        head.n_matched = n;
        head.cost = cost;
        int stop = 0;
        if (final_pass) {
            if (head.status == RGBD360_OK && n < set.min_matches) head.status = RGBD360_NO_VALID_PIXELS;
            stop = 1;
        } else if (n < set.min_matches) {
            head.status = RGBD360_NO_VALID_PIXELS;
            stop = 1;
        } else if (ill) {
            head.status = RGBD360_ILL_POSED;
            stop = 1;
        }
        flag[0] = stop;
        flag[1] = 0;
    }
    par.sync();
    if (final_pass && P.sensors) {
        for (int s = par.lane(); s < S; s += par.lanes()) {
            rgbd360_rig_calib_sensor& out = P.sensors[s];
            long long n = 0;
            double cost = 0.0, G[36], g[6];
            for (int e = 0; e < 36; ++e) G[e] = 0.0;
            for (int e = 0; e < 6; ++e) g[e] = 0.0;
            for (int k = 0; k < K; ++k) {
                const Input& in = P.in[(size_t)k * S + s];
                if (!in.used) continue;
                n += (long long)in.n;
                cost += in.rr;
                for (int e = 0; e < 36; ++e) G[e] += in.G[e];
                for (int e = 0; e < 6; ++e) g[e] += in.gs[e];
            }
            out.n_matched = n;
            out.cost = cost;
            for (int e = 0; e < 36; ++e) out.hessian[e] = (float)G[e];
            for (int e = 0; e < 6; ++e) out.gradient[e] = (float)g[e];
        }
    }
    if (flag[0]) {
        par.sync();
        if (par.lane() == 0) head.done = 1;
        return;
    }
    reduced_solve(par, P, M, rhs, d0, tmp, &flag[1]);
    par.sync();
    if (flag[1]) {
        par.sync();
        if (par.lane() == 0) {
            head.status = RGBD360_ILL_POSED;
            head.done = 1;
        }
        return;
    }
    apply_updates(par, P, rhs, vvww);
    if (par.lane() == 0) {
        float mv = 0.f, mw = 0.f;
        for (int i = 0; i < K + S; ++i) {
            mv = vvww[2 * i] > mv ? vvww[2 * i] : mv;
            mw = vvww[2 * i + 1] > mw ? vvww[2 * i + 1] : mw;
        }
        rgbd360_rig_calib_step rec;
        rec.n = head.n_matched;
        rec.cost = head.cost;
        rec.max_vv = mv;
        rec.max_ww = mw;
        if (P.trace) P.trace[head.iterations] = rec;
        head.iterations += 1;
        head.max_vv = mv;
        head.max_ww = mw;
        if (mv <= set.eps && mw <= set.eps) {
            head.converged = 1;
            head.done = 1;
        }
    }
    par.sync();
}

#if defined(__HIPCC__)
struct Image {
    const void* depth;
    size_t step;
};

// A pixel of the cloud formation.  Correct: what depth_apply.h's k_rig_cloud_models does to a measured z (and whether it is still a
// measurement) before the ray product; k_rig_pinhole_cloud has none.
struct NoCorrection {
    static constexpr bool kOn = false;
    __device__ bool operator()(int, int, int, float&) const { return true; }
};
template <class Correct>
__device__ __forceinline__ void pinhole_pixel(const Image* __restrict__ images, int depth_type, int rows, int cols, float fx, float fy, float cx, float cy,
                                              float* __restrict__ out, const Correct& correct) {
    const long long n = (long long)rows * cols, i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Image im = images[blockIdx.y];
    const int v = (int)(i / cols), u = (int)(i % cols);
    const unsigned char* line = static_cast<const unsigned char*>(im.depth) + (size_t)v * im.step;
    float z;
    bool ok;
    if (depth_type == 0) {
        const unsigned short raw = reinterpret_cast<const unsigned short*>(line)[u];
        z = 0.001f * (float)raw;
        ok = raw != 0;
    } else {
        z = reinterpret_cast<const float*>(line)[u];
        ok = z > 0.f && z < __builtin_inff();
    }
    if (Correct::kOn) ok = ok && correct((int)blockIdx.y, v, u, z);
    const float nan = __builtin_nanf("");
    const float x = (float)u - cx, y = (float)v - cy;
    const float f0 = x / fx, f1 = y / fy;
    float* p = out + ((size_t)blockIdx.y * (size_t)n + (size_t)i) * 3;
    p[0] = ok ? z * f0 : nan;
    p[1] = ok ? z * f1 : nan;
    p[2] = ok ? z : nan;
}

__global__ __launch_bounds__(256) void k_rig_pinhole_cloud(const Image* __restrict__ images, int depth_type, int rows, int cols, float fx, float fy, float cx,
                                                           float cy, float* __restrict__ out) {
    pinhole_pixel(images, depth_type, rows, cols, fx, fy, cx, cy, out, NoCorrection{});
}

// live_of_input[i]: the job of input i among the live ones, -1: an empty input
__global__ __launch_bounds__(64) void k_rig_init(Problem P, const vmap::BatchJob* __restrict__ jobs, const int* __restrict__ live_of_input) {
    const int i = (int)(blockIdx.x * 64 + threadIdx.x), K = P.set.K, S = P.set.S;
    if (i == 0) {
        Head h = {};
        *P.head = h;
    }
    if (i < 6 * (K + S)) P.upd[i] = 0.f;      // (6 (K + S) <= 6 (K S + 1): the grid covers it, see the launch)
    if (i < K) P.fr[i].has = P.fr[i].elim = P.fr[i].ill = 0;
    if (i >= K * S) return;
    P.in[i].used = 0;
    P.in[i].n = P.in[i].rr = 0.0;
    const int j = live_of_input[i];
    if (j < 0 || !jobs[j].state) return;
    vmap::LoopState<vmap::kPlaneWords>* st = static_cast<vmap::LoopState<vmap::kPlaneWords>*>(jobs[j].state);
    float pose[16];
    gn::mat4_mul(P.T + 16 * (size_t)(i / S), P.E + 16 * (size_t)(i % S), pose);
    for (int e = 0; e < 16; ++e) st->pose[e] = pose[e];
    for (int e = 0; e < vmap::kPlaneWords; ++e) st->row[e] = 0.0;
    for (int e = 0; e < 36; ++e) st->H[e] = 0.f;
    for (int e = 0; e < 6; ++e) st->g[e] = 0.f;
    st->done = st->status = st->iterations = st->converged = 0;
}

__global__ __launch_bounds__(64) void k_rig_input(Problem P, const vmap::BatchJob* __restrict__ jobs, const int* __restrict__ input_of_live, int stride,
                                                  int final_pass) {
    if (!final_pass && P.head->done) return;
    __shared__ double s_row[kRow];
    const vmap::BatchJob& job = jobs[blockIdx.x];
    const int t = threadIdx.x;
    if (t < kRow) s_row[t] = sum_rows(job.part, (int)job.n_rows, stride, t);
    __syncthreads();
    if (t != 0) return;
    const int i = input_of_live[blockIdx.x];
    double Ad[36];
    adjoint_of(P.T + 16 * (size_t)(i / P.set.S), Ad);
    input_blocks(s_row, P.set.min_input, Ad, P.in[i]);
}

__global__ __launch_bounds__(64) void k_rig_frames(Problem P, int final_pass) {
    if (!final_pass && P.head->done) return;
    const int k = (int)(blockIdx.x * 64 + threadIdx.x);
    if (k < P.set.K) frame_eliminate(P, k);
}

__global__ __launch_bounds__(256) void k_rig_solve(Problem P, const vmap::BatchJob* __restrict__ jobs, const int* __restrict__ live_of_input, float* __restrict__ vvww,
                                                   int final_pass) {
    if (!final_pass && P.head->done) return;
    __shared__ double s_M[kPacked], s_rhs[kMaxN], s_d0[kMaxN], s_tmp[kMaxN];
    __shared__ int s_flag[2];
    const Block par;
    solve_step(par, P, final_pass, s_M, s_rhs, s_d0, s_tmp, vvww, s_flag);
    __syncthreads();
    // the new P_ks into the inputs' states; a call that has ended stops its evaluations
    const int done = P.head->done, S = P.set.S;
    for (int i = threadIdx.x; i < P.set.K * S; i += blockDim.x) {
        const int j = live_of_input[i];
        if (j < 0 || !jobs[j].state) continue;
        vmap::LoopState<vmap::kPlaneWords>* st = static_cast<vmap::LoopState<vmap::kPlaneWords>*>(jobs[j].state);
        if (!final_pass) {
            float pose[16];
            gn::mat4_mul(P.T + 16 * (size_t)(i / S), P.E + 16 * (size_t)(i % S), pose);
            for (int e = 0; e < 16; ++e) st->pose[e] = pose[e];
        }
        if (done) st->done = 1;
    }
}
#endif

}  // namespace rigc

namespace {

int rig_check_params(rgbd360_map* m, const rgbd360_rig_calib_params* params, int n_sensors, rgbd360_rig_calib_params& p, IcpJob& base) {
    if (params) p = *params;
    else rgbd360_map_default_rig_calib_params(m, &p);
    if (const int rc = PlaneIcp::check(m, &p.plane, base)) return rc;
    if (p.refine_poses != 0 && p.refine_poses != 1) return vmap_fail(m, -1, "refine_poses must be 0 or 1");
    if (p.fixed_sensor < -1 || p.fixed_sensor >= n_sensors) return vmap_fail(m, -1, "fixed_sensor must lie in -1 .. n_sensors - 1");
    if (p.refine_poses && p.fixed_sensor < 0) return vmap_fail(m, -1, "refine_poses needs a fixed_sensor: T_k G^-1, G E_s is a gauge");
    if (!(p.lambda >= 0.f) || !(p.lambda < __builtin_inff())) return vmap_fail(m, -1, "lambda must be finite and not negative");
    if (p.min_input_matches < 1) return vmap_fail(m, -1, "min_input_matches must be at least 1");
    return 0;
}
bool rig_finite(const float* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!(v[i] - v[i] == 0.f)) return false;
    return true;
}
rigc::Settings rig_settings(const rgbd360_rig_calib_params& p, int K, int S) {
    rigc::Settings s = {};
    s.K = K, s.S = S, s.refine = p.refine_poses, s.fixed = p.fixed_sensor;
    s.lambda = (double)p.lambda;
    s.min_input = p.min_input_matches;
    s.min_matches = p.plane.min_matches;
    s.eps = p.plane.eps;
    return s;
}

// the device memory of a call: one block that is copied back (head, T, E, sensors, upd, trace) and the work records behind it
struct RigLayout {
    size_t head, T, E, sensors, upd, trace, out_bytes;      // offsets into c_out
    size_t in, fr, vvww, live_of_input, input_of_live, work_bytes;      // offsets into c_work
    RigLayout(int K, int S, int iters, int n_live) {
        auto a8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
        size_t at = 0;
        head = at, at = a8(at + sizeof(rigc::Head));
        T = at, at = a8(at + 16 * sizeof(float) * K);
        E = at, at = a8(at + 16 * sizeof(float) * S);
        sensors = at, at = a8(at + sizeof(rgbd360_rig_calib_sensor) * S);
        upd = at, at = a8(at + 6 * sizeof(float) * (K + S));
        trace = at, at = a8(at + sizeof(rgbd360_rig_calib_step) * std::max(iters, 1));
        out_bytes = at;
        at = 0;
        in = at, at = a8(at + sizeof(rigc::Input) * K * S);
        fr = at, at = a8(at + sizeof(rigc::Frame) * K);
        vvww = at, at = a8(at + 2 * sizeof(float) * (K + S));
        live_of_input = at, at = a8(at + sizeof(int) * K * S);
        input_of_live = at, at = a8(at + sizeof(int) * std::max(n_live, 1));
        work_bytes = at;
    }
};
rigc::Problem rig_problem(const rigc::Settings& set, const RigLayout& lay, unsigned char* out, unsigned char* work) {
    rigc::Problem P;
    P.set = set;
    P.T = reinterpret_cast<float*>(out + lay.T);
    P.E = reinterpret_cast<float*>(out + lay.E);
    P.in = reinterpret_cast<rigc::Input*>(work + lay.in);
    P.fr = reinterpret_cast<rigc::Frame*>(work + lay.fr);
    P.upd = reinterpret_cast<float*>(out + lay.upd);
    P.head = reinterpret_cast<rigc::Head*>(out + lay.head);
    P.trace = reinterpret_cast<rgbd360_rig_calib_step*>(out + lay.trace);
    P.sensors = reinterpret_cast<rgbd360_rig_calib_sensor*>(out + lay.sensors);
    return P;
}

// what the launches of one call share
struct RigDevice {
    rigc::Problem P;
    const vmap::BatchJob* jobs;
    const int *live_of_input, *input_of_live;
    float* vvww;
    int n_live, stride;
};
int rig_launch_init(rgbd360_map* m, const RigDevice& d) {
    const int K = d.P.set.K, S = d.P.set.S;
    const int threads = std::max(K * S, 6 * (K + S));
    hipLaunchKernelGGL(rigc::k_rig_init, dim3((threads + 63) / 64), dim3(64), 0, m->s->stream, d.P, d.jobs, d.live_of_input);
    HIPC(m, hipGetLastError());
    return 0;
}
// the constant number of solve launches behind an evaluation
int rig_launch_solve(rgbd360_map* m, const RigDevice& d, int final_pass) {
    hipStream_t stream = m->s->stream;
    if (d.n_live) hipLaunchKernelGGL(rigc::k_rig_input, dim3(d.n_live), dim3(64), 0, stream, d.P, d.jobs, d.input_of_live, d.stride, final_pass);
    HIPC(m, hipGetLastError());
    hipLaunchKernelGGL(rigc::k_rig_frames, dim3((d.P.set.K + 63) / 64), dim3(64), 0, stream, d.P, final_pass);
    HIPC(m, hipGetLastError());
    hipLaunchKernelGGL(rigc::k_rig_solve, dim3(1), dim3(256), 0, stream, d.P, d.jobs, d.live_of_input, d.vvww, final_pass);
    HIPC(m, hipGetLastError());
    return 0;
}

// The call on checked-or-not inputs: everything is checked before anything is launched, uploaded or allocated; then the schedule of the
// header comment.  The batch's packing, prefix table and evaluation launch are map_align_batch.h's.
int rig_calibrate(rgbd360_map* m, const std::vector<MapInput>& inputs, int K, int S, float* poses, float* extrinsics, const rgbd360_rig_calib_params& p,
                  const IcpJob& base, rgbd360_rig_calib_result* result, rgbd360_rig_calib_sensor* sensors) {
    const int n_inputs = K * S;
    std::vector<unsigned long long> rows_of(n_inputs, 0), bytes_of(n_inputs, 0);
    unsigned long long total_rows = 0, upload = 0;
    std::vector<size_t> offset_of(n_inputs, 0);
    std::vector<int> live, live_of(n_inputs, -1);
    for (int i = 0; i < n_inputs; ++i) {
        const MapInput& in = inputs[i];
        const int chk = vmap_check(m, in, true);
        if (chk < 0) return chk;
        if (chk == 1) continue;
        rows_of[i] = (unsigned long long)((in.n + vmap::kTile - 1) / vmap::kTile);
        bytes_of[i] = (unsigned long long)in.n * 3 * sizeof(float);
        if (rows_of[i] > (unsigned long long)kBatchMaxRows) return vmap_fail(m, -1, "an input of the call needs more than RGBD360_MAP_BATCH_MAX_ROWS workgroups");
        total_rows += rows_of[i];
        if (total_rows > (unsigned long long)kBatchMaxRows) return vmap_fail(m, -1, "the inputs of the call need more than RGBD360_MAP_BATCH_MAX_ROWS workgroups");
        if (!in.on_device) {
            offset_of[i] = (size_t)upload;
            upload = batch_align256((size_t)(upload + bytes_of[i]));
            if (upload > kBatchMaxUpload) return vmap_fail(m, -1, "the host inputs of the call exceed RGBD360_MAP_BATCH_MAX_UPLOAD bytes");
        }
        live_of[i] = (int)live.size();
        live.push_back(i);
    }

    // the call runs from here on
    using State = IcpState<PlaneIcp>;
    const int n_live = (int)live.size(), iters = base.p.max_iters;
    hipSetDevice(m->s->p.device);
    hipStream_t stream = m->s->stream;
    const RigLayout lay(K, S, iters, n_live);
    const size_t jobs_bytes = (size_t)std::max(n_live, 1) * sizeof(vmap::BatchJob), prefix_bytes = ((size_t)n_live + 1) * sizeof(unsigned);
    const size_t desc_bytes = jobs_bytes + ((prefix_bytes + 7) & ~(size_t)7) + lay.work_bytes - lay.live_of_input;      // jobs, prefix, the two index tables
    HIPC(m, m->a_part.ensure((size_t)std::max<unsigned long long>(total_rows, 1) * vmap::kIcpMaxWords));
    HIPC(m, m->a_state.ensure((size_t)std::max(n_live, 1) * sizeof(State)));
    HIPC(m, m->b_desc.ensure(desc_bytes));
    HIPC(m, m->b_desc_host.ensure(desc_bytes));
    HIPC(m, m->c_out.ensure(lay.out_bytes));
    HIPC(m, m->c_host.ensure(lay.out_bytes));
    HIPC(m, m->c_work.ensure(lay.work_bytes));
    if (upload) HIPC(m, m->up_depth.ensure((size_t)upload));

    unsigned char* hd = m->b_desc_host.get();
    vmap::BatchJob* hj = reinterpret_cast<vmap::BatchJob*>(hd);
    unsigned* hp = reinterpret_cast<unsigned*>(hd + jobs_bytes);
    const size_t tables_at = jobs_bytes + ((prefix_bytes + 7) & ~(size_t)7);
    int* h_live_of = reinterpret_cast<int*>(hd + tables_at);
    int* h_input_of = reinterpret_cast<int*>(hd + tables_at + (lay.input_of_live - lay.live_of_input));
    unsigned at = 0;
    for (int k = 0; k < n_live; ++k) {
        const MapInput& in = inputs[live[k]];
        const float* points = in.xyz;
        if (!in.on_device) {
            uint8_t* dst = m->up_depth.get() + offset_of[live[k]];
            HIPC(m, hipMemcpyAsync(dst, points, (size_t)bytes_of[live[k]], hipMemcpyHostToDevice, stream));
            points = reinterpret_cast<const float*>(dst);
        }
        vmap::BatchJob& d = hj[k];
        memset(&d, 0, sizeof(d));
        d.src = {nullptr, 0, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, points, in.n};
        d.state = m->a_state.get() + (size_t)k * sizeof(State);
        d.trace = nullptr;
        d.part = m->a_part.get() + (size_t)at * vmap::kPlaneWords;
        d.gx = d.n_rows = (unsigned)rows_of[live[k]];
        hp[k] = at;
        at += d.n_rows;
        h_input_of[k] = live[k];
    }
    hp[n_live] = at;
    memcpy(h_live_of, live_of.data(), sizeof(int) * (size_t)n_inputs);
    HIPC(m, hipMemcpyAsync(m->b_desc, m->b_desc_host, desc_bytes, hipMemcpyHostToDevice, stream));
    unsigned char* ho = m->c_host.get();
    memcpy(ho + lay.T, poses, 16 * sizeof(float) * (size_t)K);
    memcpy(ho + lay.E, extrinsics, 16 * sizeof(float) * (size_t)S);
    HIPC(m, hipMemcpyAsync(m->c_out.get() + lay.T, ho + lay.T, lay.sensors - lay.T, hipMemcpyHostToDevice, stream));

    RigDevice d;
    d.P = rig_problem(rig_settings(p, K, S), lay, m->c_out.get(), m->c_work.get());
    d.jobs = reinterpret_cast<const vmap::BatchJob*>(m->b_desc.get());
    d.live_of_input = reinterpret_cast<const int*>(m->b_desc.get() + tables_at);
    d.input_of_live = reinterpret_cast<const int*>(m->b_desc.get() + tables_at + (lay.input_of_live - lay.live_of_input));
    d.vvww = reinterpret_cast<float*>(m->c_work.get() + lay.vvww);
    d.n_live = n_live;
    d.stride = vmap::kPlaneWords;
    const BatchLaunch b = {d.jobs, reinterpret_cast<const unsigned*>(m->b_desc.get() + jobs_bytes), n_live, at, true};
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const vmap::Params VP = vmap_params(m, eye);     // (the pose of an input comes from its state)

    if (const int rc = rig_launch_init(m, d)) return rc;
    for (int it = 0; it <= iters; ++it) {
        const int final_pass = it == iters ? 1 : 0;
        if (n_live)
            if (const int rc = batch_launch_eval<PlaneIcp>(m, base, b, VP, final_pass)) return rc;
        if (const int rc = rig_launch_solve(m, d, final_pass)) return rc;
    }
    HIPC(m, hipMemcpyAsync(m->c_host, m->c_out, lay.out_bytes, hipMemcpyDeviceToHost, stream));
    HIPC(m, hipStreamSynchronize(stream));

    const rigc::Head& head = *reinterpret_cast<const rigc::Head*>(ho + lay.head);
    const rgbd360_rig_calib_step* tr = reinterpret_cast<const rgbd360_rig_calib_step*>(ho + lay.trace);
    m->c_trace.assign(tr, tr + head.iterations);
    memcpy(poses, ho + lay.T, 16 * sizeof(float) * (size_t)K);
    memcpy(extrinsics, ho + lay.E, 16 * sizeof(float) * (size_t)S);
    if (sensors) memcpy(sensors, ho + lay.sensors, sizeof(rgbd360_rig_calib_sensor) * (size_t)S);
    if (result) {
        result->status = head.status;
        result->iterations = head.iterations;
        result->converged = head.converged;
        result->n_inputs_used = head.n_inputs_used;
        result->n_frames_skipped = head.n_frames_skipped;
        result->n_matched = head.n_matched;
        result->cost = head.cost;
        result->fitness = head.n_matched > 0 ? head.cost / (double)head.n_matched : 0.0;
    }
    return head.status;
}

// what every entry refuses before it looks at an input
int rig_check_call(rgbd360_map* m, const void* inputs, int K, int S, const float* poses, const float* extrinsics, const rgbd360_rig_calib_params* params,
                   rgbd360_rig_calib_params& p, IcpJob& base) {
    if (K < 1 || S < 1 || S > RGBD360_RIG_CALIB_MAX_SENSORS) return vmap_fail(m, -1, "n_frames must be at least 1 and n_sensors lie in 1 .. RGBD360_RIG_CALIB_MAX_SENSORS");
    if ((long long)K * S > RGBD360_MAP_BATCH_MAX) return vmap_fail(m, -1, "n_frames x n_sensors must not exceed RGBD360_MAP_BATCH_MAX");
    if (!inputs || !poses || !extrinsics) return vmap_fail(m, -1, "inputs, poses and extrinsics must not be null");
    if (const int rc = rig_check_params(m, params, S, p, base)) return rc;
    if (!rig_finite(poses, 16 * (size_t)K) || !rig_finite(extrinsics, 16 * (size_t)S)) return vmap_fail(m, -1, "poses and extrinsics must be finite");
    return 0;
}
}  // namespace

extern "C" void rgbd360_map_default_rig_calib_params(const rgbd360_map* m, rgbd360_rig_calib_params* p) {
    if (!p) return;
    rgbd360_map_default_align_plane_params(m, &p->plane);
    p->refine_poses = 0;
    p->fixed_sensor = -1;
    p->lambda = 0.f;
    p->min_input_matches = 6;
}

extern "C" int rgbd360_map_calibrate_rig_clouds(rgbd360_map* m, const rgbd360_map_batch_cloud* inputs, int n_frames, int n_sensors, int on_device, float* poses,
                                                float* extrinsics, const rgbd360_rig_calib_params* params, rgbd360_rig_calib_result* result,
                                                rgbd360_rig_calib_sensor* sensors) {
    if (!m) return -1;
    m->err.clear();
    rgbd360_rig_calib_params p;
    IcpJob base;
    if (const int rc = rig_check_call(m, inputs, n_frames, n_sensors, poses, extrinsics, params, p, base)) return rc;
    std::vector<MapInput> in((size_t)n_frames * n_sensors);
    for (size_t i = 0; i < in.size(); ++i) in[i] = cloud_input(inputs[i].xyz, nullptr, inputs[i].n, on_device);
    return rig_calibrate(m, in, n_frames, n_sensors, poses, extrinsics, p, base, result, sensors);
}

namespace {
// What the depth entries (here and in depth_apply.h) refuse of n_inputs pinhole images before anything is launched or uploaded: the
// reason, or null; upload: the bytes of the host images packed side by side.
const char* rig_depth_refusal(const rgbd360_map_batch_frame* depth, int n_inputs, int depth_type, int rows, int cols, float fx, float fy, float cx, float cy,
                              int on_device, unsigned long long& upload) {
    const float pin[4] = {fx, fy, cx, cy};
    if (!rig_finite(pin, 4) || fx == 0.f || fy == 0.f) return "the pinhole must be finite, fx and fy not zero";
    if (depth_type != 0 && depth_type != 1) return "bad depth type";
    if (rows < 0 || cols < 0 || (long long)rows * cols >= (1ll << 30)) return "bad image size";
    const size_t prow = (size_t)cols * (depth_type == 0 ? 2 : 4);
    const long long n = (long long)rows * cols;
    upload = 0;
    for (int i = 0; i < n_inputs && n > 0; ++i) {
        if (!depth[i].depth) return "a depth image must not be null";
        if (depth[i].depth_step < prow) return "row step shorter than a row";
        if (!on_device) upload = batch_align256((size_t)(upload + prow * rows));
    }
    if (upload > kBatchMaxUpload) return "the host inputs of the call exceed RGBD360_MAP_BATCH_MAX_UPLOAD bytes";
    return nullptr;
}
// The images of a checked call where a kernel reads them: host images packed into `up`, the descriptors through img_host into img.
// `o` takes the error text (a map or a Frame360 state).
template <class Owner>
int rig_depth_stage(Owner* o, hipStream_t stream, const rgbd360_map_batch_frame* depth, int n_inputs, int depth_type, int rows, int cols, int on_device,
                    unsigned long long upload, DevBuf<uint8_t>& up, DevBuf<unsigned char>& img, PinnedBuf<unsigned char>& img_host) {
    const size_t prow = (size_t)cols * (depth_type == 0 ? 2 : 4);
    const size_t desc = sizeof(rigc::Image) * (size_t)n_inputs;
    HIPC(o, img.ensure(desc));
    HIPC(o, img_host.ensure(desc));
    if (upload) HIPC(o, up.ensure((size_t)upload));
    rigc::Image* hi = reinterpret_cast<rigc::Image*>(img_host.get());
    size_t at = 0;
    for (int i = 0; i < n_inputs; ++i) {
        hi[i] = {depth[i].depth, depth[i].depth_step};
        if (!on_device) {
            uint8_t* dst = up.get() + at;
            HIPC(o, hipMemcpy2DAsync(dst, prow, depth[i].depth, depth[i].depth_step, prow, (size_t)rows, hipMemcpyHostToDevice, stream));
            hi[i] = {dst, prow};
            at = batch_align256(at + prow * rows);
        }
    }
    HIPC(o, hipMemcpyAsync(img, img_host, desc, hipMemcpyHostToDevice, stream));
    return 0;
}
// the launch of the cloud formation over staged images; depth_apply.h defines it (with a set of depth models: its own kernel)
template <class Owner>
int rig_depth_launch(Owner* o, hipStream_t stream, const rgbd360_depth_models* set, const rigc::Image* images, int n_inputs, int n_sensors, int depth_type, int rows,
                     int cols, float fx, float fy, float cx, float cy, float* out);

// rgbd360_map_calibrate_rig_depth and, with a set, rgbd360_map_calibrate_rig_depth_models
int rig_calibrate_depth(rgbd360_map* m, const rgbd360_depth_models* set, const rgbd360_map_batch_frame* depth, int depth_type, int rows, int cols, float fx, float fy,
                        float cx, float cy, int n_frames, int n_sensors, int on_device, float* poses, float* extrinsics, const rgbd360_rig_calib_params* params,
                        rgbd360_rig_calib_result* result, rgbd360_rig_calib_sensor* sensors) {
    rgbd360_rig_calib_params p;
    IcpJob base;
    if (const int rc = rig_check_call(m, depth, n_frames, n_sensors, poses, extrinsics, params, p, base)) return rc;
    const int n_inputs = n_frames * n_sensors;
    const long long n = (long long)rows * cols;
    unsigned long long upload = 0;
    if (const char* why = rig_depth_refusal(depth, n_inputs, depth_type, rows, cols, fx, fy, cx, cy, on_device, upload)) return vmap_fail(m, -1, why);
    const unsigned long long rows_each = (unsigned long long)((n + vmap::kTile - 1) / vmap::kTile);
    if (rows_each * (unsigned long long)n_inputs > (unsigned long long)kBatchMaxRows)
        return vmap_fail(m, -1, "the inputs of the call need more than RGBD360_MAP_BATCH_MAX_ROWS workgroups");
    std::vector<MapInput> in((size_t)n_inputs);
    if (n > 0) {
        hipSetDevice(m->s->p.device);
        hipStream_t stream = m->s->stream;
        HIPC(m, m->c_cloud.ensure((size_t)n_inputs * (size_t)n * 3));
        if (const int rc = rig_depth_stage(m, stream, depth, n_inputs, depth_type, rows, cols, on_device, upload, m->up_depth, m->c_img, m->c_img_host)) return rc;
        if (const int rc = rig_depth_launch(m, stream, set, reinterpret_cast<const rigc::Image*>(m->c_img.get()), n_inputs, n_sensors, depth_type, rows, cols, fx,
                                            fy, cx, cy, m->c_cloud.get()))
            return rc;
    }
    for (int i = 0; i < n_inputs; ++i) in[(size_t)i] = cloud_input(n > 0 ? m->c_cloud.get() + (size_t)i * (size_t)n * 3 : nullptr, nullptr, n, 1);
    return rig_calibrate(m, in, n_frames, n_sensors, poses, extrinsics, p, base, result, sensors);
}
}  // namespace

extern "C" int rgbd360_map_calibrate_rig_depth(rgbd360_map* m, const rgbd360_map_batch_frame* depth, int depth_type, int rows, int cols, float fx, float fy,
                                               float cx, float cy, int n_frames, int n_sensors, int on_device, float* poses, float* extrinsics,
                                               const rgbd360_rig_calib_params* params, rgbd360_rig_calib_result* result, rgbd360_rig_calib_sensor* sensors) {
    if (!m) return -1;
    m->err.clear();
    return rig_calibrate_depth(m, nullptr, depth, depth_type, rows, cols, fx, fy, cx, cy, n_frames, n_sensors, on_device, poses, extrinsics, params, result, sensors);
}

extern "C" int rgbd360_rig_save_extrinsics(const float* extrinsics, int n_sensors, const char* dir) {
    if (!extrinsics || !dir || n_sensors < 1 || n_sensors > RGBD360_RIG_CALIB_MAX_SENSORS) return -1;
    for (int s = 0; s < n_sensors; ++s) {
        char name[32];
        std::snprintf(name, sizeof(name), "/Rt_0%d.txt", s + 1);
        std::FILE* f = std::fopen((std::string(dir) + name).c_str(), "w");
        if (!f) return 1;
        const float* M = extrinsics + 16 * (size_t)s;
        bool ok = true;
        for (int r = 0; r < 4; ++r)
            ok = std::fprintf(f, "%.9g %.9g %.9g %.9g\n", (double)M[r], (double)M[4 + r], (double)M[8 + r], (double)M[12 + r]) > 0 && ok;
        ok = std::fclose(f) == 0 && ok;
        if (!ok) return 1;
    }
    return 0;
}

// measurement and tests (rgbd360_hip_diag.h)
namespace {
int rig_solve_args(const double* rows, int K, int S, const float* poses, const float* extrinsics, const rgbd360_rig_calib_params* p) {
    if (!rows || !poses || !extrinsics || !p || K < 1 || S < 1 || S > RGBD360_RIG_CALIB_MAX_SENSORS || (long long)K * S > RGBD360_MAP_BATCH_MAX) return -1;
    if (p->fixed_sensor < -1 || p->fixed_sensor >= S || (p->refine_poses && p->fixed_sensor < 0) || (p->refine_poses != 0 && p->refine_poses != 1)) return -1;
    if (!(p->lambda >= 0.f) || !(p->lambda < __builtin_inff()) || p->min_input_matches < 1) return -1;
    return rig_finite(poses, 16 * (size_t)K) && rig_finite(extrinsics, 16 * (size_t)S) ? 0 : -1;
}
void rig_solve_out(const unsigned char* out, const RigLayout& lay, int K, int S, float* updates, float* poses_new, float* extrinsics_new, int* status) {
    if (updates) memcpy(updates, out + lay.upd, 6 * sizeof(float) * (size_t)(K + S));
    if (poses_new) memcpy(poses_new, out + lay.T, 16 * sizeof(float) * (size_t)K);
    if (extrinsics_new) memcpy(extrinsics_new, out + lay.E, 16 * sizeof(float) * (size_t)S);
    if (status) *status = reinterpret_cast<const rigc::Head*>(out + lay.head)->status;
}
}  // namespace

extern "C" int rgbd360_rig_calib_solve_host(const double* rows, int n_frames, int n_sensors, const float* poses, const float* extrinsics,
                                            const rgbd360_rig_calib_params* params, float* updates, float* poses_new, float* extrinsics_new, int* status) {
    const int K = n_frames, S = n_sensors;
    if (rig_solve_args(rows, K, S, poses, extrinsics, params)) return -1;
    const RigLayout lay(K, S, 1, K * S);
    std::vector<unsigned char> out(lay.out_bytes, 0), work(lay.work_bytes, 0);
    const rigc::Problem P = rig_problem(rig_settings(*params, K, S), lay, out.data(), work.data());
    memcpy(P.T, poses, 16 * sizeof(float) * (size_t)K);
    memcpy(P.E, extrinsics, 16 * sizeof(float) * (size_t)S);
    for (int i = 0; i < K * S; ++i) {
        double row[rigc::kRow], Ad[36];
        for (int t = 0; t < rigc::kRow; ++t) row[t] = rigc::sum_rows(rows + (size_t)i * rigc::kRow, 1, rigc::kRow, t);
        rigc::adjoint_of(P.T + 16 * (size_t)(i / S), Ad);
        rigc::input_blocks(row, P.set.min_input, Ad, P.in[i]);
    }
    for (int k = 0; k < K; ++k) rigc::frame_eliminate(P, k);
    std::vector<double> M(rigc::kPacked), v(3 * rigc::kMaxN);
    int flag[2] = {0, 0};
    rigc::solve_step(rigc::Serial{}, P, 0, M.data(), v.data(), v.data() + rigc::kMaxN, v.data() + 2 * rigc::kMaxN, reinterpret_cast<float*>(work.data() + lay.vvww), flag);
    rig_solve_out(out.data(), lay, K, S, updates, poses_new, extrinsics_new, status);
    return 0;
}

namespace {
// given rows as the inputs' only partial rows, without loop states: what rgbd360_rig_calib_solve_dev and the timing entry launch on
int rig_rows_to_device(rgbd360_map* m, const double* rows, int K, int S, const float* poses, const float* extrinsics, const rgbd360_rig_calib_params* params,
                       const RigLayout& lay, RigDevice& d) {
    const int n = K * S;
    hipSetDevice(m->s->p.device);
    hipStream_t stream = m->s->stream;
    const size_t jobs_bytes = (size_t)n * sizeof(vmap::BatchJob), tables = lay.work_bytes - lay.live_of_input, desc_bytes = jobs_bytes + tables;
    HIPC(m, m->a_part.ensure((size_t)n * vmap::kIcpMaxWords));
    HIPC(m, m->b_desc.ensure(desc_bytes));
    HIPC(m, m->b_desc_host.ensure(desc_bytes));
    HIPC(m, m->c_out.ensure(lay.out_bytes));
    HIPC(m, m->c_host.ensure(lay.out_bytes));
    HIPC(m, m->c_work.ensure(lay.work_bytes));
    unsigned char* hd = m->b_desc_host.get();
    vmap::BatchJob* hj = reinterpret_cast<vmap::BatchJob*>(hd);
    int* h_live_of = reinterpret_cast<int*>(hd + jobs_bytes);
    int* h_input_of = reinterpret_cast<int*>(hd + jobs_bytes + (lay.input_of_live - lay.live_of_input));
    for (int i = 0; i < n; ++i) {
        memset(&hj[i], 0, sizeof(hj[i]));
        hj[i].part = m->a_part.get() + (size_t)i * rigc::kRow;     // the given row as the input's only partial row; no loop state
        hj[i].gx = hj[i].n_rows = 1;
        h_live_of[i] = h_input_of[i] = i;
    }
    HIPC(m, hipMemcpyAsync(m->a_part, rows, sizeof(double) * rigc::kRow * (size_t)n, hipMemcpyHostToDevice, stream));
    HIPC(m, hipMemcpyAsync(m->b_desc, m->b_desc_host, desc_bytes, hipMemcpyHostToDevice, stream));
    unsigned char* ho = m->c_host.get();
    memcpy(ho + lay.T, poses, 16 * sizeof(float) * (size_t)K);
    memcpy(ho + lay.E, extrinsics, 16 * sizeof(float) * (size_t)S);
    HIPC(m, hipMemcpyAsync(m->c_out.get() + lay.T, ho + lay.T, lay.sensors - lay.T, hipMemcpyHostToDevice, stream));
    d.P = rig_problem(rig_settings(*params, K, S), lay, m->c_out.get(), m->c_work.get());
    d.jobs = reinterpret_cast<const vmap::BatchJob*>(m->b_desc.get());
    d.live_of_input = reinterpret_cast<const int*>(m->b_desc.get() + jobs_bytes);
    d.input_of_live = reinterpret_cast<const int*>(m->b_desc.get() + jobs_bytes + (lay.input_of_live - lay.live_of_input));
    d.vvww = reinterpret_cast<float*>(m->c_work.get() + lay.vvww);
    d.n_live = n;
    d.stride = rigc::kRow;
    return 0;
}
}  // namespace

extern "C" int rgbd360_rig_calib_solve_dev(rgbd360_map* m, const double* rows, int n_frames, int n_sensors, const float* poses, const float* extrinsics,
                                           const rgbd360_rig_calib_params* params, float* updates, float* poses_new, float* extrinsics_new, int* status) {
    if (!m) return -1;
    m->err.clear();
    const int K = n_frames, S = n_sensors;
    if (rig_solve_args(rows, K, S, poses, extrinsics, params)) return vmap_fail(m, -1, "bad arguments");
    const RigLayout lay(K, S, 1, K * S);
    RigDevice d;
    if (const int rc = rig_rows_to_device(m, rows, K, S, poses, extrinsics, params, lay, d)) return rc;
    if (const int rc = rig_launch_init(m, d)) return rc;
    if (const int rc = rig_launch_solve(m, d, 0)) return rc;
    HIPC(m, hipMemcpyAsync(m->c_host, m->c_out, lay.out_bytes, hipMemcpyDeviceToHost, m->s->stream));
    HIPC(m, hipStreamSynchronize(m->s->stream));
    rig_solve_out(m->c_host.get(), lay, K, S, updates, poses_new, extrinsics_new, status);
    return 0;
}

extern "C" int rgbd360_rig_calib_time_solve(rgbd360_map* m, const double* rows, int n_frames, int n_sensors, const float* poses, const float* extrinsics,
                                            const rgbd360_rig_calib_params* params, int reps, float avg_us[4]) {
    if (!m) return -1;
    m->err.clear();
    const int K = n_frames, S = n_sensors;
    if (rig_solve_args(rows, K, S, poses, extrinsics, params) || reps < 1 || !avg_us) return vmap_fail(m, -1, "bad arguments");
    std::vector<double> still(rows, rows + (size_t)rigc::kRow * K * S);
    for (int i = 0; i < K * S; ++i)
        for (int e = 0; e < 6; ++e) still[(size_t)i * rigc::kRow + 22 + e] = 0.0;      // no gradient: updates of exactly zero, the poses stay
    const RigLayout lay(K, S, 1, K * S);
    RigDevice d;
    if (const int rc = rig_rows_to_device(m, still.data(), K, S, poses, extrinsics, params, lay, d)) return rc;
    hipStream_t stream = m->s->stream;
    HIPC(m, hipStreamSynchronize(stream));      // (`still` is the host's)
    const auto chain = [&](int n_kernels) {
        if (const int rc = rig_launch_init(m, d)) return rc;
        if (n_kernels >= 1) hipLaunchKernelGGL(rigc::k_rig_input, dim3(d.n_live), dim3(64), 0, stream, d.P, d.jobs, d.input_of_live, d.stride, 0);
        if (n_kernels >= 2) hipLaunchKernelGGL(rigc::k_rig_frames, dim3((K + 63) / 64), dim3(64), 0, stream, d.P, 0);
        if (n_kernels >= 3) hipLaunchKernelGGL(rigc::k_rig_solve, dim3(1), dim3(256), 0, stream, d.P, d.jobs, d.live_of_input, d.vvww, 0);
        return hipGetLastError() == hipSuccess ? 0 : -100;
    };
    VmapTimer timer(m, stream);      // made last
    if (timer.rc) return timer.rc;
    timer.rc = chain(3);             // once untimed: code loaded
    for (int c = 0; c < 4; ++c) timer.timed(avg_us[c], reps, [&] { return chain(c); });
    return timer.finish(avg_us, 0, reps);
}

extern "C" int rgbd360_rig_calib_trace(rgbd360_map* m, int max_trace, int* n_trace, rgbd360_rig_calib_step* trace) {
    if (!m) return -1;
    m->err.clear();
    if (n_trace) *n_trace = (int)m->c_trace.size();
    for (int k = 0; trace && k < max_trace && k < (int)m->c_trace.size(); ++k) trace[k] = m->c_trace[k];
    return 0;
}
