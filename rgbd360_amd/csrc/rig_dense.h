// rig_dense.h -- dense registration of two frames of the 8-sensor rig: RegisterRGBD360::RegisterDensePhotoICP
// (RegisterRGBD360.h:344-520) over calcPhotoICPError_robot (RPI.h:4905-5076) and calcHessianGradient_robot (RPI.h:5083-5407).
// SURVEY.md 8f rank 3.  Included by rgbd360_api.hip after sequence_engine.h (shares its fused frame set-up).
//
// The unknown is the RIG's relative pose T (p_rig1 = T p_rig2); sensor s sees it through its extrinsic Rt_s (sensor -> rig).  One
// fused pass evaluates, for all sensors in ONE launch (blockIdx.y = sensor), the error sums of calcPhotoICPError_robot (every
// visible pixel, no saliency test) and the normal equations of calcHessianGradient_robot (saliency-gated rows) at one pose;
// the rows are accumulated directly in the rig's left-perturbation coordinates, so the 8 per-sensor H, g just add up.
//
// The reference function cannot be followed to the letter -- as written it never accepts a step and reads an uninitialised
// Jacobian row.  SURVEY.md asks for it "with the reference's bugs fixed"; the three fixes (A: new_error at the candidate pose,
// B: jacobianRt_z = row 2 of the transform Jacobian, C: depth residual against the TRANSFORMED point's depth) are documented in
// oracle/photo_icp_ref.cpp, which restates the same fixed function line by line and is this file's checker.
//
// Device arithmetic definition of the warp (the oracle's math_mode 1 repeats it): q = (T Rt_s) p and P' = Rt_s^-1 q with fused
// multiply-adds, correctly rounded 1/Z', column = round(fma(X' fx, 1/Z', ox)), row likewise, round = floor(x + 0.5).  One chain serves
// both passes.
// The REFERENCE's arithmetic (LIBM = 1, rgbd360_rig_set_index_arithmetic(rig, 1); the oracle's math_mode 0): the two passes warp a
// pixel differently, so every pixel goes through both chains --
//   chain 0, calcPhotoICPError_robot (RPI.h:4923-4924, 5021-5029): P' = C_s p with C_s = (Rt_s^-1 T) Rt_s formed in float,
//            column = round((double)(X' fx) * inv + ox), inv = 1.0 / (double)Z';
//   chain 1, calcHessianGradient_robot (RPI.h:5278-5290): q = T (Rt_s p), P' = Rt_s^-1 q, column = round(((double)X' * fx) * inv + ox);
// Eigen's product order without fused multiply-adds, round half away from zero, a |x| > 1e9 or non-finite projection is invisible.
// The error sums (and FIX C's depth Z') follow chain 0, the Jacobian rows (q, X', Y', Z', 1/Z' and the target they read) chain 1.
// Row algebra: jacobianT36 = R_s^-1 [I | -skew(q)], so a camera-frame row vector a contributes (b, q x b) with b = R_s a.
#pragma once

namespace r360 {

constexpr int kMaxRigSensors = 8;      // NUM_ASUS_SENSORS
struct RigPoses {
    float M[kMaxRigSensors][12];       // rows of (T * Rt_s):   q  = M p      (r00 r01 r02 tx | r10 ... | r20 ...)
    float Ri[kMaxRigSensors][12];      // rows of Rt_s^-1:      P' = Ri q
};
// What the reference's arithmetic needs besides.  A kernel argument of its own BEHIND the others: the argument offsets of the default
// instantiation stay what they were, and k_eval_rig<M, 0> compiles to the former k_eval_rig<M> (hipcc -S: one commutative s_and_b64 of the
// projection's sane mask has its operands swapped; nothing else differs).
struct RigPosesRef {
    float Rt[kMaxRigSensors][12];      // rows of Rt_s
    float C[kMaxRigSensors][12];       // rows of C_s = (Rt_s^-1 T) Rt_s   (relPoseCam; gn::mat4_mul = the oracle's mat4_mul_f32)
    float T[12];                       // rows of T
};
// k_eval_rig's argument block: 4 pointers, 6 ints / floats, PinK, EvalConsts and both pose blocks (~1.7 KiB) -- within the 4 KiB a
// kernel argument block may hold
static_assert(sizeof(RigPoses) + sizeof(RigPosesRef) + sizeof(PinK) + sizeof(EvalConsts) + 4 * sizeof(void*) + 6 * sizeof(int) <= 4096,
              "rig kernel arguments exceed 4 KiB: pass the pose blocks in a device buffer");

__device__ __forceinline__ void xform12(const float* m, float x, float y, float z, float& X, float& Y, float& Z) {
    X = fmaf(m[2], z, fmaf(m[1], y, fmaf(m[0], x, m[3])));
    Y = fmaf(m[6], z, fmaf(m[5], y, fmaf(m[4], x, m[7])));
    Z = fmaf(m[10], z, fmaf(m[9], y, fmaf(m[8], x, m[11])));
}

// the oracle's xform_f32: ((m0 x + m1 y) + m2 z) + t, no contraction
__device__ __forceinline__ void xform12_ref(const float* m, float x, float y, float z, float& X, float& Y, float& Z) {
#pragma clang fp contract(off)
    X = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    Y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    Z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

// The warp of one source point of sensor s: q (the point in the rig frame after the motion; not formed by LIBM = 1's chain 0), P' = (X,
// Y, Z), iz = 1 / Z and the target pixel (ri, ci); returns whether the projection is finite and within 1e9 (the caller tests the image
// bounds and the point's own validity).  LIBM = 0: the device definition, `chain` unused.  LIBM = 1: the reference's chain `chain` (0:
// error pass, 1: H / g pass).  k_eval_rig and the diagnostic k_rig_warp_indices both warp through this function.
template <int LIBM>
__device__ __forceinline__ bool rig_warp(const float* Mq, const float* Ri, const RigPosesRef& ref, int s, int chain, float px, float py, float pz,
                                         const PinK& K, float& qx, float& qy, float& qz, float& X, float& Y, float& Z, float& iz, int& ri,
                                         int& ci) {
    if (LIBM == 0) {
        xform12(Mq, px, py, pz, qx, qy, qz);
        xform12(Ri, qx, qy, qz, X, Y, Z);
        iz = rcp_rn(Z);
        const float tc = fmaf(X * K.fx, iz, K.ox);
        const float tr = fmaf(Y * K.fy, iz, K.oy);
        const bool sane = (fabsf(tr) < 1e9f) && (fabsf(tc) < 1e9f);
        ri = round_index(sane ? tr : -1.f);
        ci = round_index(sane ? tc : -1.f);
        return sane;
    }
    double dc, dr;
    if (chain == 0) {                                     // uniform
#pragma clang fp contract(off)
        qx = qy = qz = 0.f;
        xform12_ref(ref.C[s], px, py, pz, X, Y, Z);       // relPoseCam * p
        const double inv = 1.0 / (double)Z;
        iz = (float)inv;
        dc = (double)(X * K.fx) * inv + (double)K.ox;
        dr = (double)(Y * K.fy) * inv + (double)K.oy;
    } else {
#pragma clang fp contract(off)
        float ux, uy, uz;
        xform12_ref(ref.Rt[s], px, py, pz, ux, uy, uz);   // Rt_s * p
        xform12_ref(ref.T, ux, uy, uz, qx, qy, qz);       // T * (Rt_s * p)
        xform12_ref(Ri, qx, qy, qz, X, Y, Z);             // Rt_s^-1 * q
        const double inv = 1.0 / (double)Z;
        iz = (float)inv;
        dc = ((double)X * (double)K.fx) * inv + (double)K.ox;
        dr = ((double)Y * (double)K.fy) * inv + (double)K.oy;
    }
    const bool sane = fabs(dr) <= 1e9 && fabs(dc) <= 1e9;      // false for inf and NaN too
    ri = (int)round(sane ? dr : -1.0);                          // round(): half away from zero
    ci = (int)round(sane ? dc : -1.0);
    return sane;
}

// b = R_s a, a residual row taken from sensor s into the rig frame: R_s = (Rt_s^-1 rotation)^T, i.e. b_i = sum_j Ri[j][i] a_j
__device__ __forceinline__ F3 to_rig(const float* Ri, const F3& a) {
#pragma clang fp contract(fast)
    return {Ri[0] * a.a + Ri[4] * a.b + Ri[8] * a.c, Ri[1] * a.a + Ri[5] * a.b + Ri[9] * a.c, Ri[2] * a.a + Ri[6] * a.b + Ri[10] * a.c};
}

// One pixel of k_eval_rig in the reference's arithmetic: the error terms from chain 0, the Jacobian rows from chain 1.  The target is
// gathered once, and a second time only by the lanes whose chain-1 pixel differs (rare: a projection within rounding of a pixel border).
template <int METHOD>
__device__ __forceinline__ void eval_rig_ref_pixel(EvalAcc& A, const float* Ri, const RigPosesRef& ref, int s, const float4& p, int i,
                                                   bool in_range, const F3* __restrict__ trgP, const F3* __restrict__ trgD, int rows, int cols,
                                                   const PinK& K, const EvalConsts& ec, float sal_thr) {
    float qx, qy, qz, X0, Y0, Z0, iz0, X, Y, Z, iz;
    int r0, c0, r1, c1;
    const bool ok0 = rig_warp<1>(nullptr, Ri, ref, s, 0, p.x, p.y, p.z, K, qx, qy, qz, X0, Y0, Z0, iz0, r0, c0) &&
                     ((unsigned)r0 < (unsigned)rows) && ((unsigned)c0 < (unsigned)cols);
    const bool ok1 = rig_warp<1>(nullptr, Ri, ref, s, 1, p.x, p.y, p.z, K, qx, qy, qz, X, Y, Z, iz, r1, c1) &&
                     ((unsigned)r1 < (unsigned)rows) && ((unsigned)c1 < (unsigned)cols);
    bool live = in_range && (p.x != kInvalidPoint);
    if (sal_thr >= 0.f) {      // uniform: bUseSalientPixels -- the list holds source indices, both passes read it
        const F3 ts = trgP[in_range ? i : 0];
        live = live && (fabsf(ts.b) > sal_thr || fabsf(ts.c) > sal_thr);
    }
    const bool vis0 = ok0 && live, vis = ok1 && live;
    const unsigned t0 = vis0 ? (unsigned)(r0 * cols + c0) : 0u, t1 = vis ? (unsigned)(r1 * cols + c1) : 0u;
    F3 tp0 = {0.f, 0.f, 0.f}, td0 = {0.f, 0.f, 0.f};
    if (METHOD != 1) tp0 = trgP[t0];
    if (METHOD != 0) td0 = trgD[t0];
    F3 tp = tp0, td = td0;
    if (vis && t1 != t0) {
        if (METHOD != 1) tp = trgP[t1];
        if (METHOD != 0) td = trgD[t1];
    }
    // calcPhotoICPError_robot: every visible pixel of chain 0, no saliency test
    if (METHOD != 1) {
        A.nP += ballot_count(vis0);
        if (vis0) {
#pragma clang fp contract(fast)
            const float res = pin_photo_res(tp0.a, p.w, ec).res;
            A.e2p += res * res;
        }
    }
    if (METHOD != 0) {
        const bool err_on = vis0 && isfinite(td0.a);
        A.nD += ballot_count(err_on);
        if (err_on) {
#pragma clang fp contract(fast)
            const float res = pin_depth_res(td0.a, Z0, ec).res;                   // FIX C: chain 0's transformed depth
            A.e2d += res * res;
        }
    }
    // calcHessianGradient_robot: the rows of chain 1's pixel, with its saliency `continue`s (RPI.h:5331-5332, 5352-5353)
    const bool sal_p = !(fabsf(tp.b) < ec.thr_photo && fabsf(tp.c) < ec.thr_photo);
    const bool sal_d = !(fabsf(td.b) < ec.thr_depth && fabsf(td.c) < ec.thr_depth);
    const bool fin_d = METHOD != 0 && isfinite(td.a);
    const float iz2 = iz * iz;
    if (METHOD != 1) {
        const bool row_on = vis && sal_p && (METHOD == 0 || !fin_d || sal_d);
        A.nVis += ballot_count(row_on);
        if (row_on) {
            const PinRes ph = pin_photo_res(tp.a, p.w, ec);
            const F3 j = to_rig(Ri, pin_photo_row(tp.b, tp.c, K, X, Y, iz, iz2, ph.w));
            accumulate_row(A, j.a, j.b, j.c, qx, qy, qz, ph.res);
        }
    }
    if (METHOD != 0) {
        const bool row_on = vis && fin_d && sal_d && (METHOD == 1 || sal_p);
        A.nVis += ballot_count(row_on);
        if (row_on) {
            const PinRes dp = pin_depth_res(td.a, Z, ec);                         // FIX C
            const F3 j = to_rig(Ri, pin_depth_row(td.b, td.c, K, X, Y, iz, iz2, dp.w));      // FIX B: - jacobianT36.row(2)
            accumulate_row(A, j.a, j.b, j.c, qx, qy, qz, dp.res);
        }
    }
}

template <int METHOD, int LIBM>
__global__ __launch_bounds__(kEvalThreads) void k_eval_rig(const float4* __restrict__ src, const F3* __restrict__ trgP,
                                                            const F3* __restrict__ trgD, int rows, int cols, int n, PinK K, EvalConsts ec,
                                                            RigPoses poses, double* __restrict__ partials, int partials_stride, int chunk, float sal_thr,
                                                            RigPosesRef ref) {
    const int b = blockIdx.x, s = blockIdx.y;
    const int base = b * chunk;
    const int end = min(base + chunk, n);
    src += (size_t)s * n; trgP += (size_t)s * n; trgD += (size_t)s * n;
    const float* Mq = poses.M[s];
    const float* Ri = poses.Ri[s];

    EvalAcc A;
#pragma unroll
    for (int k = 0; k < 27; ++k) A.acc[k] = 0.f;
    A.e2p = A.e2d = 0.f;
    A.nP = A.nD = A.nVis = 0;

    const int n_steps = (end - base + kEvalThreads - 1) / kEvalThreads;      // wave-uniform: the ballots count whole waves
    for (int k = 0; k < n_steps; ++k) {
        const int i = base + k * kEvalThreads + (int)threadIdx.x;
        const bool in_range = i < end;
        const float4 p = src[in_range ? i : n - 1];
        if constexpr (LIBM != 0) {
            eval_rig_ref_pixel<METHOD>(A, Ri, ref, s, p, i, in_range, trgP, trgD, rows, cols, K, ec, sal_thr);
            continue;
        }
        float qx, qy, qz, X, Y, Z, iz;
        int ri, ci;
        const bool sane = rig_warp<0>(Mq, Ri, ref, s, 0, p.x, p.y, p.z, K, qx, qy, qz, X, Y, Z, iz, ri, ci);
        bool vis = sane && ((unsigned)ri < (unsigned)rows) && ((unsigned)ci < (unsigned)cols) && in_range && (p.x != kInvalidPoint);
        if (sal_thr >= 0.f) {      // uniform: bUseSalientPixels (RPI.h:4930-5003, 5121-5262) -- both passes run over vSalientPixels only, the
            const F3 ts = trgP[in_range ? i : 0];      // interior pixels whose TARGET gray gradient exceeds thresSaliency, used as source indices
            vis = vis && (fabsf(ts.b) > sal_thr || fabsf(ts.c) > sal_thr);
        }
        const unsigned ti = vis ? (unsigned)(ri * cols + ci) : 0u;
        F3 tp = {0.f, 0.f, 0.f}, td = {0.f, 0.f, 0.f};
        if (METHOD != 1) tp = trgP[ti];
        if (METHOD != 0) td = trgD[ti];
        const float depth2 = td.a;
        const bool sal_p = !(fabsf(tp.b) < ec.thr_photo && fabsf(tp.c) < ec.thr_photo);
        const bool sal_d = !(fabsf(td.b) < ec.thr_depth && fabsf(td.c) < ec.thr_depth);
        const bool fin_d = METHOD != 0 && isfinite(depth2);
        const float iz2 = iz * iz;
        if (METHOD != 1) {
            A.nP += ballot_count(vis);                                             // calcPhotoICPError_robot: no saliency test
            // calcHessianGradient_robot: a non-salient intensity gradient skips the pixel (RPI.h:5331-5332); a finite target depth with a
            // flat depth gradient skips it too, photometric row included (RPI.h:5352-5353)
            const bool row_on = vis && sal_p && (METHOD == 0 || !fin_d || sal_d);
            A.nVis += ballot_count(row_on);
            if (vis) {
#pragma clang fp contract(fast)
                const PinRes ph = pin_photo_res(tp.a, p.w, ec);
                A.e2p += ph.res * ph.res;
                if (row_on) {
                    const F3 j = to_rig(Ri, pin_photo_row(tp.b, tp.c, K, X, Y, iz, iz2, ph.w));
                    accumulate_row(A, j.a, j.b, j.c, qx, qy, qz, ph.res);
                }
            }
        }
        if (METHOD != 0) {
            const bool err_on = vis && fin_d;
            A.nD += ballot_count(err_on);
            const bool row_on = err_on && sal_d && (METHOD == 1 || sal_p);
            A.nVis += ballot_count(row_on);
            if (err_on) {
#pragma clang fp contract(fast)
                const PinRes dp = pin_depth_res(depth2, Z, ec);                     // FIX C: the transformed point's depth
                A.e2d += dp.res * dp.res;
                if (row_on) {
                    const F3 j = to_rig(Ri, pin_depth_row(td.b, td.c, K, X, Y, iz, iz2, dp.w));      // FIX B: - jacobianT36.row(2)
                    accumulate_row(A, j.a, j.b, j.c, qx, qy, qz, dp.res);
                }
            }
        }
    }

    __shared__ double red[kEvalThreads / 64][kNumPartials];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        float v[32], out[2];
#pragma unroll
        for (int k = 0; k < 27; ++k) v[k] = A.acc[k];
        v[P_E2P] = A.e2p;
        v[P_E2D] = A.e2d;
        v[P_NP] = v[P_ND] = v[P_NVIS] = 0.f;
        wave_reduce32(v, out);
        if ((lane & 3) == 0) {
            const int row = lane >> 4, quad = (lane >> 2) & 3;
            const int idx = 2 * (quad & 1) + 4 * (quad >> 1) + 8 * (row & 1) + 16 * (row >> 1);
            if (idx + 0 < P_NP) red[wave][idx + 0] = (double)out[0];
            if (idx + 1 < P_NP) red[wave][idx + 1] = (double)out[1];
        }
        if (lane == 63) {
            red[wave][P_NP] = (double)A.nP;
            red[wave][P_ND] = (double)A.nD;
            red[wave][P_NVIS] = (double)A.nVis;
        }
    }
    __syncthreads();
    if (threadIdx.x < kNumPartials) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kEvalThreads / 64; ++w) v += red[w][threadIdx.x];
        partials[(size_t)s * partials_stride + (size_t)b * kNumPartials + threadIdx.x] = v;
    }
}

// Per-sensor totals of the partial rows, fixed order, written straight into pinned host memory: block s -> out[s][32].
// The block that finishes last stores the host's sequence tag (host_wait.h): no tag kernel behind this one.
__global__ __launch_bounds__(256) void k_rig_reduce(const double* __restrict__ partials, int partials_stride, int nb, double* __restrict__ out,
                                                    unsigned* __restrict__ ticket, unsigned* __restrict__ tag, unsigned seq) {
    __shared__ double red[8][kNumPartials];
    const int s = blockIdx.x, v = threadIdx.x & 31, q = threadIdx.x >> 5;
    double acc = 0.0;
    for (int b = q; b < nb; b += 8) acc += partials[(size_t)s * partials_stride + (size_t)b * kNumPartials + v];
    red[q][v] = acc;
    __syncthreads();
    if (threadIdx.x < kNumPartials) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += red[k][threadIdx.x];
        out[(size_t)s * kNumPartials + threadIdx.x] = t;
        __threadfence_system();        // this block's totals (written by this wave alone) are on their way to the host before it takes its ticket
    }
    __syncthreads();
    // acq_rel on the ticket: the block that draws the last number synchronises with every earlier block's release, so their host
    // writes (fenced above) are ordered before the tag it stores next
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
        __threadfence_system();
        *ticket = 0u;
        __hip_atomic_store(tag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// rgbd360_rig_warp_indices: the (row, col) every source pixel of sensor blockIdx.y warps to, through rig_warp; (-1, -1) for an invalid
// source point or an invisible projection.  out = [S][n][2].
template <int LIBM>
__global__ __launch_bounds__(256) void k_rig_warp_indices(const float4* __restrict__ src, int rows, int cols, int n, PinK K, RigPoses poses,
                                                          RigPosesRef ref, int chain, int32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (i >= n) return;
    const size_t o = (size_t)s * n + i;
    const float4 p = src[o];
    int r = -1, c = -1;
    if (p.x != kInvalidPoint) {
        float qx, qy, qz, X, Y, Z, iz;
        int ri, ci;
        const bool sane = rig_warp<LIBM>(poses.M[s], poses.Ri[s], ref, s, chain, p.x, p.y, p.z, K, qx, qy, qz, X, Y, Z, iz, ri, ci);
        if (sane && ((unsigned)ri < (unsigned)rows) && ((unsigned)ci < (unsigned)cols)) { r = ri; c = ci; }
    }
    out[2 * o] = r;
    out[2 * o + 1] = c;
}

}  // namespace r360

struct rgbd360_rig {
    rgbd360_params p;
    int S = 0, rows = 0, cols = 0;
    float cam[4] = {0, 0, 0, 0};
    float Rt[r360::kMaxRigSensors][16], Rt_inv[r360::kMaxRigSensors][16];
    SeqEngine* E = nullptr;           // buffers + fused set-up of S "slots" (one per sensor), created at the first frame
    PinnedBuf<double> h_tot{hostwait::kPublishedFlags};      // [S][32]
    hostwait::SpinTag tag;
    DevBuf<unsigned> d_ticket;        // device counter of k_rig_reduce's blocks
    bool have_src = false, have_trg = false;
    float sal_thr = -1.f;             // useSaliency(true) on the per-sensor objects: thresSaliency (RPI.h:217); < 0 = off
    int index_libm = 0;               // rgbd360_rig_set_index_arithmetic: 1 = the warp in the reference's arithmetic (k_eval_rig<M, 1>)
    std::string err;
};

namespace {

int rfail(rgbd360_rig* R, int code, const std::string& msg) {
    R->err = msg;
    return code;
}

void rigid_inverse(const float* M, float* Inv) {       // [R | t]^-1 = [R^T | -R^T t], float, the oracle's order
    for (int k = 0; k < 16; ++k) Inv[k] = 0.f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Inv[j * 4 + i] = M[i * 4 + j];
    for (int i = 0; i < 3; ++i) Inv[12 + i] = -((Inv[0 * 4 + i] * M[12] + Inv[1 * 4 + i] * M[13]) + Inv[2 * 4 + i] * M[14]);
    Inv[15] = 1.f;
}

// the 8 sensor images of one frame -> pyramids + records of every level (fused set-up, 1 launch per level for all sensors)
int rig_set_frames(rgbd360_rig* R, bool target, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth, size_t depth_step,
                   int depth_type, int rows, int cols) {
    if (!rgb || !depth) return rfail(R, -1, "null pointer");
    if (depth_type != 0 && depth_type != 1) return rfail(R, -1, "depth_type must be 0 (u16 mm) or 1 (f32 m)");
    for (int s = 0; s < R->S; ++s)
        if (!rgb[s] || !depth[s]) return rfail(R, -1, "null sensor image");
    hipSetDevice(R->p.device);
    if (!R->E || R->rows != rows || R->cols != cols) {
        seq_free(R->E);
        R->E = nullptr;
        R->have_src = R->have_trg = false;
        std::string err;
        const int rc = seq_create(R->p, R->S, rows, cols, 256, &R->E, &err);
        if (rc) return rfail(R, rc, err);
        R->rows = rows; R->cols = cols;
    }
    SeqEngine* E = R->E;
    const size_t dpx = depth_type == 0 ? 2 : 4;
    int rc = seq_ensure_stage(E, depth_type);
    if (rc) return rfail(R, rc, E->err);
    FramePtrs fp;
    memset(&fp, 0, sizeof(fp));
    for (int s = 0; s < R->S; ++s) {
        uint8_t* const s_rgb = E->ring.rgb[0] + s * E->frame_bytes(3);
        uint8_t* const s_depth = E->ring.depth[0] + s * E->frame_bytes(dpx);
        const hipError_t e = copy_frame_h2d(s_rgb, s_depth, rgb[s], rgb_step, depth[s], depth_step, depth_type, rows, cols, E->stream);
        if (e != hipSuccess) return rfail(R, -(int)e - 1000, hipGetErrorString(e));
        fp.rgb[s] = s_rgb;
        fp.depth[s] = s_depth;
    }
    const unsigned long long live = (1ull << R->S) - 1ull;
    for (int l = 0; l < R->p.n_pyr; ++l) {
        const SeqLevel& L = E->levels[l];
        FrameLevelArgs A;
        memset(&A, 0, sizeof(A));
        A.rows = L.rows; A.cols = L.cols;
        if (l + 1 < R->p.n_pyr) {
            const SeqLevel& N = E->levels[l + 1];
            A.drows = N.rows; A.dcols = N.cols;
            A.gray_next = N.gray; A.depth_next = N.depth;
        }
        A.seam = 0;                                      // no seam mask on a pinhole sensor
        A.depth_type = depth_type;
        A.rgb_step = (size_t)cols * 3; A.depth_step = (size_t)cols * dpx;
        A.gray_in = L.gray; A.depth_in = L.depth;
        A.src_rec = L.srcRec; A.trg_p = L.trgP[0]; A.trg_d = L.trgD[0];
        A.min_depth = R->p.min_depth; A.max_depth = R->p.max_depth;
        A.live_mask = live; A.src_mask = target ? 0ull : live; A.trg_mask = target ? live : 0ull;
        A.pinhole = 1;
        const PinK K = level_K(R->cam, l);
        A.pin_ox = K.ox; A.pin_oy = K.oy;
        A.pin_inv_fx = 1. / K.fx; A.pin_inv_fy = 1. / K.fy;      // RPI.h:4921-4922 (float = double quotient, as pin_prepare_level)
        const dim3 g((L.cols + kFsTW - 1) / kFsTW, (L.rows + kFsTH - 1) / kFsTH, R->S);
        if (l == 0) hipLaunchKernelGGL((k_frame_level_b<true>), g, dim3(256), 0, E->stream, A, fp);
        else hipLaunchKernelGGL((k_frame_level_b<false>), g, dim3(256), 0, E->stream, A, fp);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(E->stream);      // the caller may reuse its host images
    if (e != hipSuccess) return rfail(R, -(int)e - 1000, hipGetErrorString(e));
    if (target) R->have_trg = true; else R->have_src = true;
    return 0;
}

// the pose blocks of the warp at rig pose T (column-major); Q is filled for the reference's arithmetic only
void rig_poses(const rgbd360_rig* R, const float* T, RigPoses* P, RigPosesRef* Q) {
    for (int s = 0; s < R->S; ++s) {
        float M[16];
        gn::mat4_mul(T, R->Rt[s], M);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                P->M[s][4 * r + c] = M[c * 4 + r];
                P->Ri[s][4 * r + c] = R->Rt_inv[s][c * 4 + r];
            }
    }
    memset(Q, 0, sizeof(*Q));
    if (!R->index_libm) return;
    for (int s = 0; s < R->S; ++s) {
        float A[16], C[16];
        gn::mat4_mul(R->Rt_inv[s], T, A);
        gn::mat4_mul(A, R->Rt[s], C);                     // relPoseCam = poseCamRobot_inv * poseGuess * poseCamRobot   RPI.h:4923-4924
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                Q->Rt[s][4 * r + c] = R->Rt[s][c * 4 + r];
                Q->C[s][4 * r + c] = C[c * 4 + r];
            }
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) Q->T[4 * r + c] = T[c * 4 + r];
}

// one fused pass over all sensors at rig pose T; per-sensor totals are cast to float and added in sensor order like
// `Hessian += alignSensorID[sensor_id].getHessian()` (RegisterRGBD360.h:435-440)
int rig_eval(rgbd360_rig* R, int level, const float* T, int method, lm::Sums* out) {
    SeqEngine* E = R->E;
    const SeqLevel& L = E->levels[level];
    RigPoses P;
    RigPosesRef Q;
    rig_poses(R, T, &P, &Q);
    const PinK K = level_K(R->cam, level);
    const EvalConsts ec = eval_consts(R->p);
    const dim3 g(L.nblocks, R->S), b(kEvalThreads);
    with_choice<0, 1>(R->index_libm != 0, [&](auto Lm) {
        with_method(method, [&](auto M) {
            hipLaunchKernelGGL((k_eval_rig<M, Lm>), g, b, 0, E->stream, L.srcRec.get(), L.trgP[0].get(), L.trgD[0].get(), L.rows, L.cols, L.n, K, ec, P, E->d_partials.get(),
                               E->partials_stride, L.chunk, R->sal_thr, Q);
        });
    });
    hipLaunchKernelGGL(k_rig_reduce, dim3(R->S), dim3(256), 0, E->stream, E->d_partials.get(), E->partials_stride, L.nblocks, R->h_tot.get(), R->d_ticket.get(),
                       R->tag.h, ++R->tag.seq);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hostwait::wait(R->tag, E->stream);      // (spin on a pinned tag: one round trip per LM evaluation)
    if (e != hipSuccess) return rfail(R, -(int)e - 1000, hipGetErrorString(e));
    for (int s = 0; s < R->S; ++s) out->add_row(R->h_tot + (size_t)s * kNumPartials);
    return 0;
}

}  // namespace

extern "C" {

void rgbd360_rig_destroy(rgbd360_rig* R) {
    if (!R) return;
    hipSetDevice(R->p.device);
    seq_free(R->E);
    hostwait::spin_tag_free(&R->tag);
    delete R;
}

int rgbd360_rig_create(const rgbd360_params* p, int n_sensors, const float* Rt, float fx, float fy, float ox, float oy, rgbd360_rig** out) {
    if (!p || !out || !Rt || n_sensors < 1 || n_sensors > kMaxRigSensors) return -1;
    *out = nullptr;
    if (p->n_pyr < 1 || p->n_pyr > 8) return -1;
    if (!(fx > 0.f) || !(fy > 0.f)) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -100;      // no HIP device: no fallback
    if (p->device < 0 || p->device >= ndev) return -101;
    if (hipSetDevice(p->device) != hipSuccess) return -102;
    rgbd360_rig* R = new rgbd360_rig();
    R->p = *p;
    R->p.mask_seams = 0;
    R->S = n_sensors;
    R->cam[0] = fx; R->cam[1] = fy; R->cam[2] = ox; R->cam[3] = oy;
    for (int s = 0; s < n_sensors; ++s) {
        memcpy(R->Rt[s], Rt + 16 * s, sizeof(float) * 16);
        rigid_inverse(R->Rt[s], R->Rt_inv[s]);
    }
    if (R->h_tot.ensure((size_t)kNumPartials * kMaxRigSensors) != hipSuccess || hostwait::spin_tag_init(&R->tag) != hipSuccess ||
        R->d_ticket.ensure(1) != hipSuccess || hipMemset(R->d_ticket, 0, sizeof(unsigned)) != hipSuccess) {
        rgbd360_rig_destroy(R);
        return -103;
    }
    *out = R;
    return 0;
}

const char* rgbd360_rig_last_error(rgbd360_rig* R) { return R ? R->err.c_str() : "null handle"; }

int rgbd360_rig_use_saliency(rgbd360_rig* R, int on, float thres_saliency) {
    if (!R) return -1;
    if (on && !(thres_saliency >= 0.f)) return rfail(R, -1, "thres_saliency must be >= 0");
    R->sal_thr = on ? thres_saliency : -1.f;
    return 0;
}

int rgbd360_rig_set_index_arithmetic(rgbd360_rig* R, int mode) {
    if (!R) return -1;
    if (mode != 0 && mode != 1) return rfail(R, -1, "index arithmetic: 0 (device definition) or 1 (the reference's arithmetic)");
    R->index_libm = mode;
    return 0;
}
int rgbd360_rig_get_index_arithmetic(rgbd360_rig* R) { return R ? R->index_libm : -1; }

int rgbd360_rig_warp_indices(rgbd360_rig* R, int level, const float pose[16], int chain, int32_t* host_out_rc) {
    if (!R) return -1;
    if (!R->have_src) return rfail(R, -2, "rgbd360_rig_set_source must be called first");
    if (level < 0 || level >= R->p.n_pyr) return rfail(R, -3, "bad pyramid level");
    if (chain != 0 && chain != 1) return rfail(R, -4, "chain must be 0 (error pass) or 1 (H / g pass)");
    if (!pose || !host_out_rc) return rfail(R, -1, "null pointer");
    hipSetDevice(R->p.device);
    SeqEngine* E = R->E;
    const SeqLevel& L = E->levels[level];
    RigPoses P;
    RigPosesRef Q;
    rig_poses(R, pose, &P, &Q);
    const size_t bytes = (size_t)R->S * L.n * 2 * sizeof(int32_t);
    DevBuf<int32_t> d_out;
    hipError_t e = d_out.ensure(bytes / sizeof(int32_t));
    if (e != hipSuccess) return rfail(R, -(int)e - 1000, hipGetErrorString(e));
    const dim3 g((L.n + 255) / 256, R->S);
    with_choice<0, 1>(R->index_libm != 0, [&](auto Lm) {
        hipLaunchKernelGGL(k_rig_warp_indices<Lm>, g, dim3(256), 0, E->stream, L.srcRec.get(), L.rows, L.cols, L.n, level_K(R->cam, level), P, Q, chain, d_out.get());
    });
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host_out_rc, d_out, bytes, hipMemcpyDeviceToHost, E->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(E->stream);
    if (e != hipSuccess) return rfail(R, -(int)e - 1000, hipGetErrorString(e));
    return 0;
}

int rgbd360_rig_set_target(rgbd360_rig* R, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth, size_t depth_step,
                           int depth_type, int rows, int cols) {
    return R ? rig_set_frames(R, true, rgb, rgb_step, depth, depth_step, depth_type, rows, cols) : -1;
}
int rgbd360_rig_set_source(rgbd360_rig* R, const uint8_t* const* rgb, size_t rgb_step, const void* const* depth, size_t depth_step,
                           int depth_type, int rows, int cols) {
    return R ? rig_set_frames(R, false, rgb, rgb_step, depth, depth_step, depth_type, rows, cols) : -1;
}

int rgbd360_rig_eval(rgbd360_rig* R, int level, const float pose[16], int method, double err2_split[2], long long n_split[2], float H[36],
                     float g[6], double H64[36], double g64[6], long long* n_rows) {
    if (!R) return -1;
    if (!R->have_src || !R->have_trg) return rfail(R, -2, "rgbd360_rig_set_target and _set_source must be called first");
    if (level < 0 || level >= R->p.n_pyr) return rfail(R, -3, "bad pyramid level");
    if (method < 0 || method > 2) return rfail(R, -4, "bad method");
    if (!pose) return rfail(R, -1, "null pose pointer");
    hipSetDevice(R->p.device);
    lm::Sums S;
    const int rc = rig_eval(R, level, pose, method, &S);
    if (rc) return rc;
    S.write(err2_split, n_split, H, g, H64, g64, n_rows);
    return 0;
}

// RegisterRGBD360.h:383-500 (with fix A).  Returns 0 / RGBD360_ILL_POSED (pose_out = the pose reached, like `rigidTransf = pose_estim;
// return false`).  res->hessian = the last summed Hessian (informationM), res->iters = accepted steps per level, res->err_final =
// the error (sum of squared weighted residuals) at the returned pose.
int rgbd360_rig_align(rgbd360_rig* R, const float guess[16], int method, float pose_out[16], rgbd360_result* res) {
    if (!R) return -1;
    if (!R->have_src || !R->have_trg) return rfail(R, -2, "rgbd360_rig_set_target and _set_source must be called first");
    if (method < 0 || method > 2) return rfail(R, -4, "bad method");
    if (!guess || !pose_out) return rfail(R, -1, "null pose pointer");
    hipSetDevice(R->p.device);
    // FIX A: every candidate is evaluated at pose_estim_temp; the error is error2, the plain sum calcPhotoICPError_robot returns; the
    // exponential is CPose3D::exp(update), the full one (RegisterRGBD360.h:455)
    lm::Outcome O;
    const int rc = lm::align(lm::rig_schedule(), R->p.n_pyr, guess, [](int) { return 0; },
                             [&](int level, const float* pose, lm::Sums& S) { return rig_eval(R, level, pose, method, &S); },
                             [](const lm::Sums& S) { return S.e2p + S.e2d; }, [](const lm::Trip&) {}, &O);
    if (rc) return rc;
    memcpy(pose_out, O.pose, sizeof(O.pose));
    rgbd360_result Rs;
    memset(&Rs, 0, sizeof(Rs));
    Rs.status = O.status;
    Rs.err_final = O.final_error;
    memcpy(Rs.iters, O.iters, sizeof(O.iters));
    memcpy(Rs.hessian, O.H, sizeof(O.H));
    memcpy(Rs.gradient, O.g, sizeof(O.g));
    if (res) *res = Rs;
    return O.status;
}

}  // extern "C"
