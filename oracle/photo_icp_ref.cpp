// =====================================================================================
//  oracle/photo_icp_ref.cpp  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
//  CPU restatement of the dense spherical RGB-D alignment path of EduFdez/rgbd360
//  (RegisterPhotoICP::setTargetFrame / setSourceFrame / alignFrames360 and what they
//  call).  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
//  load this library; the product (rgbd360_amd/) never does.
//
//  PARITY UNPINNED: the reference ships no tests, golden vectors or recorded poses for
//  this path and cannot be compiled here (it needs MRPT, OpenCV,
//  PCL, Eigen, Boost, none of which is installed).  This file therefore follows the
//  reference source line by line; every function cites the lines it restates
//  ("RPI.h" = /root/reference/include/RegisterPhotoICP.h).  Arithmetic that the
//  reference delegates to third-party libraries is restated from their published
//  algorithms and marked THIRD-PARTY below:
//     OpenCV 2.4  cvtColor(CV_RGB2GRAY) on 8U, Mat::convertTo, pyrDown (5x5 binomial)
//     Eigen 3     fixed-size products, Matrix<float,6,6>::inverse() (partial-pivot LU)
//     MRPT 1.x    Eigen plugin rank() (ColPivHouseholderQR), CPose3D::exp(.,pseudo=true)
//
//  Float semantics: the reference is built by GCC -O3 -mtune=native (top CMakeLists.txt
//  :77), i.e. x86-64 baseline SSE2: no FMA contraction.  Build this file with
//  -ffp-contract=off and without fast-math (oracle/Makefile does).
//
//  Two switches exist purely for checking the HIP path:
//    math_mode   0 = libm asinf/atan2f/roundf (reference-faithful)
//                1 = the branch-free polynomial asinf/atan2f the device kernels use
//                    (same operations in the same order => warped pixel indices of the
//                    HIP path can be compared bit-for-bit)
//    reduce_mode 0 = float32 accumulators for H,g like RPI.h:3117-3195 (OpenMP chunking)
//                1 = float64 accumulation of the same float32 per-pixel rows (the
//                    comparison target for the GPU's f32-lane / f64-block reduction)
// =====================================================================================
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include <algorithm>
#ifdef _OPENMP
#include <omp.h>
#endif

namespace {

// Miscellaneous.h:43-45 -- truncated literal, type double.
constexpr double kPI = 3.14159265359;
// RPI.h:40
constexpr float kInvalidPoint = -10000.f;

enum { METHOD_PHOTO = 0, METHOD_DEPTH = 1, METHOD_PHOTO_DEPTH = 2 };  // RPI.h:194

struct Params {
    int   n_pyr;            // RPI.h:204 nPyrLevels(4)
    float min_depth;        // RPI.h:202 (0.3)
    float max_depth;        // RPI.h:203 (6.0)
    float sigma_photo;      // RPI.h:208 stdDevPhoto = 6/255
    float sigma_depth;      // RPI.h:211 stdDevDepth = 0.2
    float thres_sal_photo;  // RPI.h:218 (0.01)
    float thres_sal_depth;  // RPI.h:219 (0.01)
    int   max_iters;        // RPI.h:4593 (10)
    float tol_residual;     // RPI.h:4594 (1e-3)
    float tol_update;       // RPI.h:4595 (1e-4)
    int   mask_seams;       // RPI.h:4538-4549 (1)
    int   math_mode;
    int   reduce_mode;
};

struct Image {
    int rows = 0, cols = 0;
    std::vector<float> d;
    void alloc(int r, int c) { rows = r; cols = c; d.assign((size_t)r * c, 0.f); }
    float& at(int r, int c) { return d[(size_t)r * cols + c]; }
    float at(int r, int c) const { return d[(size_t)r * cols + c]; }
};

struct IterTrace {          // one record per error evaluation inside alignFrames360
    int level, it, accepted;
    double error, new_error;
    float pose[16];
    float update[6];
    long  n_valid;
};

struct Result {
    int    status;          // 0 ok, 1 ill-posed, 2 no valid pixels
    int    iters[8];
    float  sso;
    double err_final, rms_photo, rms_depth;
    float  hessian[36];     // column-major
    float  gradient[6];
};

struct Ctx {
    Params p;
    std::vector<Image> graySrc, grayTrg, depthSrc, depthTrg, gTrgGx, gTrgGy, dTrgGx, dTrgGy;
    std::vector<float> lut;         // xyz AoS, 3 floats / pixel (Eigen::Vector3f)
    int lut_level = -1;
    float H[36], g[6];              // column-major 6x6, like Eigen
    double H64[36], g64[6];         // same sums accumulated in double (diagnostics)
    float sso = 0.f;
    long  n_visible = 0;
    double last_err2 = 0, last_err2_photo = 0, last_err2_depth = 0;
    long  last_nvalid = 0, last_nvalid_photo = 0, last_nvalid_depth = 0;
    std::vector<IterTrace> trace;
    bool keep_intermediates = true;  // allocate J arrays per call like RPI.h:2761-2767
    float cam[4] = {0, 0, 0, 0};     // cameraMatrix(0,0), (1,1), (0,2), (1,2)   RPI.h:89, 254-257
    bool have_cam = false;
    bool use_saliency = false;       // bUseSalientPixels (RPI.h:146, 266-269)
    float thres_saliency = 0.01f;    // thresSaliency (RPI.h:217)
    std::vector<std::vector<int>> salient;      // vSalientPixels (RPI.h:157): per level, built from the TARGET's gray gradients
};

// ------------------------------------------------------------------------------------
// Scalar helpers
// ------------------------------------------------------------------------------------

// RPI.h:545-554 weightHuber<T>, T = float on this path.
inline float weightHuber(float error, float regularization) {
    float error_abs = fabsf(error);
    if (error_abs < regularization) return 1.f;
    float weight = sqrtf(2 * regularization * error_abs - regularization * regularization) / error_abs;
    return weight;
}

// C round(): half away from zero.  Written with exact float ops so that the device can
// use the identical sequence.
inline float round_half_away(float x) {
    float t = truncf(x);
    float f = fabsf(x - t);           // exact
    if (f >= 0.5f) t += copysignf(1.f, x);
    return t;
}

// Device arithmetic (math_mode 1): the operation sequence of rgbd360_amd/csrc/photo_icp_kernels.h warp_pixel.
// Pure float32 fma / mul / add / correctly rounded sqrt and reciprocal: IEEE-exact on x86 and gfx950 alike, hence
// bit-identical results (the device's sqrt_rn / rcp_rn are checked against IEEE by its own self-test).
inline float atan_unit(float t) {     // atan(t), t in [0,1]: odd minimax polynomial
    const float q0 = -0.3333333195069166f, q1 = 0.19999765993465415f, q2 = -0.14279110844310372f,
                q3 = 0.11037993832882714f, q4 = -0.08673169371217875f, q5 = 0.06284358078457526f,
                q6 = -0.03627014369584507f, q7 = 0.01375026672953864f, q8 = -0.00244702708829393f;
    const float s = t * t;
    float p = fmaf(s, q8, q7);
    p = fmaf(s, p, q6);
    p = fmaf(s, p, q5);
    p = fmaf(s, p, q4);
    p = fmaf(s, p, q3);
    p = fmaf(s, p, q2);
    p = fmaf(s, p, q1);
    p = fmaf(s, p, q0);
    return fmaf(t * s, p, t);
}
inline float atan2_from_t(float y, float x, float ay, float ax, float t) {
    float a = atan_unit(t);
    if (ay > ax) a = 1.57079637f - a;
    if (std::signbit(x)) a = 3.14159274f - a;
    return copysignf(a, y);
}
// Stand-alone forms of the device's angle functions (unit tests): asin(x) = atan2(x, sqrt(1 - x^2)).
inline float atan2f_poly(float y, float x) {
    const float ay = fabsf(y), ax = fabsf(x);
    const float mx = fmaxf(fmaxf(ay, ax), 1e-9f), mn = fminf(ay, ax);
    return atan2_from_t(y, x, ay, ax, mn * (1.f / mx));
}
inline float asinf_poly(float x) { return atan2f_poly(x, sqrtf(fmaxf(fmaf(-x, x, 1.f), 0.f))); }
inline int round_index(float x) { return (int)floor((double)x + 0.5); }   // v_cvt_rpi_i32_f32: exact sum, then floor

// ------------------------------------------------------------------------------------
// THIRD-PARTY restatements (OpenCV)
// ------------------------------------------------------------------------------------

// cv::cvtColor(CV_RGB2GRAY) for CV_8UC3 (OpenCV 2.4 RGB2Gray<uchar>: fixed point, shift 14,
// coefficients R 4899 / G 9617 / B 1868, rounding term 1<<13), followed by
// Mat::convertTo(CV_32FC1, 1./255) (cvtScale_<uchar,float,float>: float(src)*float(scale)).
// Call sites RPI.h:485-486, 502-503.
void rgb_to_gray_f32(const uint8_t* rgb, size_t step, int rows, int cols, Image& out) {
    out.alloc(rows, cols);
    const float scale = (float)(1. / 255);
    for (int r = 0; r < rows; ++r) {
        const uint8_t* row = rgb + (size_t)r * step;
        for (int c = 0; c < cols; ++c) {
            int v = (4899 * row[3 * c] + 9617 * row[3 * c + 1] + 1868 * row[3 * c + 2] + 8192) >> 14;
            out.at(r, c) = (float)v * scale;
        }
    }
}

inline int reflect101(int i, int n) {           // cv::BORDER_REFLECT_101
    if (n == 1) return 0;
    while (i < 0 || i >= n) {
        if (i < 0) i = -i;
        else i = 2 * n - 2 - i;
    }
    return i;
}

// cv::pyrDown on CV_32FC1 with explicit dsize (cols/2, rows/2)  (RPI.h:303).
// OpenCV 2.4 pyrDown_<FltCast<float,8>>: horizontal 1-4-6-4-1 into row buffers,
// vertical 1-4-6-4-1, one multiply by 1/256.  Source index 2*x+k, BORDER_REFLECT_101.
void pyr_down_f32(const Image& src, Image& dst) {
    const int dr = src.rows / 2, dc = src.cols / 2;
    dst.alloc(dr, dc);
    std::vector<float> hbuf((size_t)src.rows * dc);
    for (int r = 0; r < src.rows; ++r)
        for (int x = 0; x < dc; ++x) {
            int c0 = reflect101(2 * x - 2, src.cols), c1 = reflect101(2 * x - 1, src.cols), c2 = 2 * x,
                c3 = reflect101(2 * x + 1, src.cols), c4 = reflect101(2 * x + 2, src.cols);
            hbuf[(size_t)r * dc + x] =
                src.at(r, c2) * 6 + (src.at(r, c1) + src.at(r, c3)) * 4 + src.at(r, c0) + src.at(r, c4);
        }
    for (int y = 0; y < dr; ++y) {
        int r0 = reflect101(2 * y - 2, src.rows), r1 = reflect101(2 * y - 1, src.rows), r2 = 2 * y,
            r3 = reflect101(2 * y + 1, src.rows), r4 = reflect101(2 * y + 2, src.rows);
        for (int x = 0; x < dc; ++x) {
            float v = hbuf[(size_t)r2 * dc + x] * 6 + (hbuf[(size_t)r1 * dc + x] + hbuf[(size_t)r3 * dc + x]) * 4 +
                      hbuf[(size_t)r0 * dc + x] + hbuf[(size_t)r4 * dc + x];
            dst.at(y, x) = v * (1.f / 256.f);
        }
    }
}

// ------------------------------------------------------------------------------------
// RPI.h:292-308 buildPyramid
// ------------------------------------------------------------------------------------
void buildPyramid(const Image& img, std::vector<Image>& pyr, int nLevels) {
    pyr.resize(nLevels);
    pyr[0] = img;
    for (int level = 1; level < nLevels; ++level) pyr_down_f32(pyr[level - 1], pyr[level]);
}

// RPI.h:312-354 buildPyramidRange.  depth_type 0: CV_16U millimetres -> convertTo(CV_32FC1, 0.001)
// (float(src)*float(0.001)); depth_type 1: already float metres.
void buildPyramidRange(const void* depth, size_t step, int depth_type, int rows, int cols, const Params& p,
                       std::vector<Image>& pyr) {
    pyr.resize(p.n_pyr);
    pyr[0].alloc(rows, cols);
    for (int r = 0; r < rows; ++r) {
        if (depth_type == 0) {
            const uint16_t* row = (const uint16_t*)((const uint8_t*)depth + (size_t)r * step);
            for (int c = 0; c < cols; ++c) pyr[0].at(r, c) = (float)row[c] * 0.001f;
        } else {
            const float* row = (const float*)((const uint8_t*)depth + (size_t)r * step);
            for (int c = 0; c < cols; ++c) pyr[0].at(r, c) = row[c];
        }
    }
    for (int level = 1; level < p.n_pyr; ++level) {
        const Image& prev = pyr[level - 1];
        Image& cur = pyr[level];
        cur.alloc(prev.rows / 2, prev.cols / 2);
#pragma omp parallel for
        for (int r = 0; r < cur.rows * 2; r += 2)          // reference iterates r < prev.rows; identical for even sizes,
            for (int c = 0; c < cur.cols * 2; c += 2) {     // and it would write out of bounds for odd ones.
                float avDepth = 0.f;
                unsigned nValidPixels = 0;
                for (int i = 0; i < 2; ++i)
                    for (int j = 0; j < 2; ++j) {
                        float z = prev.at(r + i, c + j);
                        if (z > p.min_depth && z < p.max_depth) {
                            avDepth += z;
                            ++nValidPixels;
                        }
                    }
                if (nValidPixels > 0) cur.at(r / 2, c / 2) = avDepth / nValidPixels;
            }
    }
}

// RPI.h:365-398 calcGradientXY
void calcGradientXY(const Image& src, Image& gradX, Image& gradY) {
    gradX.alloc(src.rows, src.cols);
    gradY.alloc(src.rows, src.cols);
#pragma omp parallel for
    for (int r = 1; r < src.rows - 1; ++r)
        for (int c = 1; c < src.cols - 1; ++c) {
            const float v = src.at(r, c);
            if ((v > src.at(r, c + 1) && v < src.at(r, c - 1)) || (v < src.at(r, c + 1) && v > src.at(r, c - 1)))
                gradX.at(r, c) = 2.f / (1 / (src.at(r, c + 1) - v) + 1 / (v - src.at(r, c - 1)));
            if ((v > src.at(r + 1, c) && v < src.at(r - 1, c)) || (v < src.at(r + 1, c) && v > src.at(r - 1, c)))
                gradY.at(r, c) = 2.f / (1 / (src.at(r + 1, c) - v) + 1 / (v - src.at(r - 1, c)));
        }
}

// RPI.h:4538-4549 seam mask: 2-px-wide bands at c = s*(nCols/8)-1, s = 1..7
void maskSeams(Image& img) {
    int width_sensor = img.cols / 8;
    for (int s = 1; s < 8; ++s)
        for (int r = 0; r < img.rows; ++r)
            for (int k = 0; k < 2; ++k) {
                int c = s * width_sensor - 1 + k;
                if (c >= 0 && c < img.cols) img.at(r, c) = 0.f;
            }
}

// RPI.h:4554-4587 LUT of 3-D points of the source sphere
void buildLUT(Ctx& ctx, int level) {
    const Image& depth = ctx.depthSrc[level];
    const int nRows = depth.rows, nCols = depth.cols;
    ctx.lut.assign((size_t)nRows * nCols * 3, 0.f);
    const float angle_res = 2 * kPI / nCols;
    std::vector<float> v_sinTheta(nCols), v_cosTheta(nCols);
    for (int c = 0; c < nCols; ++c) {
        float theta = c * angle_res;
        v_sinTheta[c] = sinf(theta);
        v_cosTheta[c] = cosf(theta);
    }
    const float half_nRows = 0.5 * nRows - 0.5;
    for (int r = 0; r < nRows; ++r) {
        float phi = (half_nRows - r) * angle_res;
        float sin_phi = sinf(phi), cos_phi = cosf(phi);
        for (int c = 0; c < nCols; ++c) {
            size_t i = (size_t)r * nCols + c;
            float depth1 = depth.at(r, c);
            if (ctx.p.min_depth < depth1 && depth1 < ctx.p.max_depth) {
                ctx.lut[3 * i + 0] = depth1 * sin_phi;
                ctx.lut[3 * i + 1] = -depth1 * cos_phi * v_sinTheta[c];
                ctx.lut[3 * i + 2] = -depth1 * cos_phi * v_cosTheta[c];
            } else
                ctx.lut[3 * i + 0] = kInvalidPoint;
        }
    }
    ctx.lut_level = level;
}

// Shared per-pixel front end of RPI.h:2663-2684 and 2959-2989.
struct Warp {
    float X, Y, Z, dist, dist_inv;
    int r, c;
    bool visible;
};

struct PoseRT {
    float R[9];  // row-major R[i*3+j]
    float t[3];
};
inline PoseRT split_pose(const float* pose /*col-major 4x4*/) {
    PoseRT o;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o.R[i * 3 + j] = pose[j * 4 + i];
        o.t[i] = pose[12 + i];
    }
    return o;
}

inline Warp warp_pixel(const PoseRT& T, const float* p, int nRows, int nCols, float half_nRows, float angle_res_inv,
                       int math_mode) {
    Warp w;
    if (math_mode == 0) {
        // Eigen fixed-size product rotation*LUT + translation: ((a0*b0 + a1*b1) + a2*b2) + t
        w.X = ((T.R[0] * p[0] + T.R[1] * p[1]) + T.R[2] * p[2]) + T.t[0];
        w.Y = ((T.R[3] * p[0] + T.R[4] * p[1]) + T.R[5] * p[2]) + T.t[1];
        w.Z = ((T.R[6] * p[0] + T.R[7] * p[1]) + T.R[8] * p[2]) + T.t[2];
        w.dist = sqrtf((w.X * w.X + w.Y * w.Y) + w.Z * w.Z);  // Eigen norm()
        w.dist_inv = 1.f / w.dist;
        float phi_trg = asinf(w.X * w.dist_inv);
        float theta_trg = (float)((double)atan2f(w.Y, w.Z) + kPI);  // float + double PI, stored to float
        w.r = (int)roundf(half_nRows - phi_trg * angle_res_inv);
        w.c = (int)roundf(theta_trg * angle_res_inv);
        w.visible = (w.r >= 0 && w.r < nRows) && w.c < nCols;  // RPI.h:2684 (c==nCols dropped, not wrapped)
        if (w.visible && w.c < 0) w.visible = false;           // cannot occur (theta_trg >= 0); guards the index
    } else {
        // device arithmetic: same IEEE operations in the same order as photo_icp_kernels.h warp_pixel
        w.X = fmaf(T.R[2], p[2], fmaf(T.R[1], p[1], fmaf(T.R[0], p[0], T.t[0])));
        w.Y = fmaf(T.R[5], p[2], fmaf(T.R[4], p[1], fmaf(T.R[3], p[0], T.t[1])));
        w.Z = fmaf(T.R[8], p[2], fmaf(T.R[7], p[1], fmaf(T.R[6], p[0], T.t[2])));
        const float rho2 = fmaf(w.Z, w.Z, w.Y * w.Y);
        const float d2 = fmaf(w.X, w.X, rho2);
        w.dist = sqrtf(d2);
        w.dist_inv = 1.f / w.dist;
        const float rho = sqrtf(rho2);
        const float ax = fabsf(w.X), ay = fabsf(w.Y), az = fabsf(w.Z);
        const float mxp = fmaxf(fmaxf(ax, rho), 1e-9f), mnp = fminf(ax, rho);
        const float mxt = fmaxf(fmaxf(ay, az), 1e-9f), mnt = fminf(ay, az);
        const float r = 1.f / (mxp * mxt);
        const float tp = mnp * (r * mxt);
        const float tt = mnt * (r * mxp);
        float phi_trg = atan_unit(tp);
        if (ax > rho) phi_trg = 1.57079637f - phi_trg;
        phi_trg = copysignf(phi_trg, w.X);
        const float theta = atan2_from_t(w.Y, w.Z, ay, az, tt);
        const float pi_k = (float)(kPI * (double)angle_res_inv);      // the +PI of RPI.h:2677 folded into the column scaling
        w.r = round_index(fmaf(phi_trg, -angle_res_inv, half_nRows));
        w.c = round_index(fmaf(theta, angle_res_inv, pi_k));
        w.visible = ((unsigned)w.r < (unsigned)nRows) && ((unsigned)w.c < (unsigned)nCols);
    }
    return w;
}

// ------------------------------------------------------------------------------------
// RPI.h:2545-2739 errorPhotoICP_sphere
// ------------------------------------------------------------------------------------
double errorPhotoICP_sphere(Ctx& ctx, int level, const float* pose, int method) {
    double error2 = 0.0, error2_photo = 0.0, error2_depth = 0.0;
    long numValidPts = 0, nPhoto = 0, nDepth = 0;
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const float angle_res = 2 * kPI / nCols;
    const float angle_res_inv = 1 / angle_res;
    const float half_nRows = 0.5 * nRows - 0.5;
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const double stdDevPhoto_inv = 1. / stdDevPhoto;
    const PoseRT T = split_pose(pose);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level], &dgx = ctx.dTrgGx[level], &dgy = ctx.dTrgGy[level];
    const float thrI = ctx.p.thres_sal_photo, thrD = ctx.p.thres_sal_depth;
    const long n = (long)nRows * nCols;
    const int mm = ctx.p.math_mode;

#pragma omp parallel for reduction(+ : error2, error2_photo, error2_depth, numValidPts, nPhoto, nDepth)
    for (long i = 0; i < n; ++i) {
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        Warp w = warp_pixel(T, p, nRows, nCols, half_nRows, angle_res_inv, mm);
        if (!w.visible) continue;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            if (fabsf(gx.at(w.r, w.c)) < thrI && fabsf(gy.at(w.r, w.c)) < thrI) continue;
            float pixel1 = graySrc.d[i];
            float pixel2 = grayTrg.at(w.r, w.c);
            float photoDiff = pixel2 - pixel1;
            double weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;  // float * double
            float weightedErrorPhoto = weight_photo * photoDiff;
            error2 += weightedErrorPhoto * weightedErrorPhoto;
            error2_photo += weightedErrorPhoto * weightedErrorPhoto;
            ++numValidPts;
            ++nPhoto;
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            float depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                if (fabsf(dgx.at(w.r, w.c)) < thrD && fabsf(dgy.at(w.r, w.c)) < thrD) continue;
                float depthDiff = depth2 - w.dist;
                float stdDev_depth1 = stdDevDepth * depth2;
                double weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;  // float/float -> double
                float weightedErrorDepth = weight_depth * depthDiff;
                error2 += weightedErrorDepth * weightedErrorDepth;
                error2_depth += weightedErrorDepth * weightedErrorDepth;
                ++numValidPts;
                ++nDepth;
            }
        }
    }
    ctx.last_err2 = error2;
    ctx.last_nvalid = numValidPts;
    ctx.last_err2_photo = error2_photo;
    ctx.last_err2_depth = error2_depth;
    ctx.last_nvalid_photo = nPhoto;
    ctx.last_nvalid_depth = nDepth;
    // RPI.h:2737 prints "error2 ... numValidPts ..." on every call: silenced.
    return sqrt(error2 / numValidPts);
}

// jacobianWarpRt = jacobianProj23 * jacobianT36 of RPI.h:2994-3026: d(c', r') / d(delta) for the left perturbation
// exp(delta) * T, delta = [t; w], evaluated at the transformed point p' = (X, Y, Z).
inline void warp_jacobian(float X, float Y, float Z, float dist_inv, float angle_res_inv, float Jw0[6], float Jw1[6]) {
    // jacobianT36 = [ I | -skew(p') ]  (RPI.h:2994-2996, Miscellaneous.h:88-98)
    // -skew(p') = [ 0  Z -Y ; -Z 0  X ; Y -X 0 ]
    // jacobianProj23 (RPI.h:3000-3016)
    float z_inv = 1.f / Z;
    float z_inv2 = z_inv * z_inv;
    float D_atan_theta = 1.f / (1 + Y * Y * z_inv2) * angle_res_inv;
    float a1 = D_atan_theta * z_inv;
    float a2 = -Y * z_inv2 * D_atan_theta;
    float dist_inv2 = dist_inv * dist_inv;
    float x_dist_inv2 = X * dist_inv2;
    float D_asin = 1.f / sqrtf(1 - X * x_dist_inv2) * angle_res_inv;
    float b0 = -D_asin * dist_inv * (1 - X * x_dist_inv2);
    float b1 = D_asin * (x_dist_inv2 * Y * dist_inv);
    float b2 = D_asin * (x_dist_inv2 * Z * dist_inv);
    // jacobianWarpRt = jacobianProj23 * jacobianT36 (RPI.h:3026); Eigen coefficient products
    // ((a0*b0 + a1*b1) + a2*b2) with the structural zeros dropped (adding +-0 is exact).
    const float r0[6] = {0.f, a1, a2, a1 * (-Z) + a2 * Y, a2 * (-X), a1 * X};
    const float r1[6] = {b0, b1, b2, b1 * (-Z) + b2 * Y, b0 * Z + b2 * (-X), b0 * (-Y) + b1 * X};
    for (int j = 0; j < 6; ++j) {
        Jw0[j] = r0[j];
        Jw1[j] = r1[j];
    }
}

// ------------------------------------------------------------------------------------
// RPI.h:2745-3228 calcHessGrad_sphere
// ------------------------------------------------------------------------------------
void calcHessGrad_sphere(Ctx& ctx, int level, const float* pose, int method) {
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const long imgSize = (long)nRows * nCols;
    const float angle_res = 2 * kPI / nCols;
    const float angle_res_inv = 1 / angle_res;
    const float half_nRows = 0.5 * nRows - 0.5;

    // RPI.h:2761-2767: per-call intermediates (Eigen::MatrixXf is column-major: 6 planes of imgSize)
    std::vector<float> jacobiansPhoto((size_t)imgSize * 6), jacobiansDepth((size_t)imgSize * 6);
    std::vector<float> residualsPhoto(imgSize, 0.f), residualsDepth(imgSize, 0.f);
    std::vector<int> validPixelsPhoto(imgSize, 0), validPixelsDepth(imgSize, 0);
    std::vector<float> invDepthBuffer(imgSize, 0.f);  // allocated+zeroed by the reference, unused on this path
    (void)invDepthBuffer;

    const PoseRT T = split_pose(pose);
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const float stdDevPhoto_inv = 1. / stdDevPhoto;
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level], &dgx = ctx.dTrgGx[level], &dgy = ctx.dTrgGy[level];
    const float thrI = ctx.p.thres_sal_photo, thrD = ctx.p.thres_sal_depth;
    const int mm = ctx.p.math_mode;
    long numVisiblePixels = 0;

#pragma omp parallel for reduction(+ : numVisiblePixels)
    for (long i = 0; i < imgSize; ++i) {
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        Warp w = warp_pixel(T, p, nRows, nCols, half_nRows, angle_res_inv, mm);
        if (!w.visible) continue;
        ++numVisiblePixels;
        const float X = w.X, Y = w.Y, Z = w.Z, dist_inv = w.dist_inv;

        float Jw0[6], Jw1[6];
        warp_jacobian(X, Y, Z, dist_inv, angle_res_inv, Jw0, Jw1);

        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            float tgx = gx.at(w.r, w.c), tgy = gy.at(w.r, w.c);
            if (fabsf(tgx) < thrI && fabsf(tgy) < thrI) continue;
            float pixel1 = graySrc.d[i];
            float pixel2 = grayTrg.at(w.r, w.c);
            float photoDiff = pixel2 - pixel1;
            float weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            float weightedErrorPhoto = weight_photo * photoDiff;
            // jacobianPhoto = weight_photo * target_imgGradient * jacobianWarpRt, evaluated left to right
            float wgx = weight_photo * tgx, wgy = weight_photo * tgy;
            for (int j = 0; j < 6; ++j) jacobiansPhoto[(size_t)j * imgSize + i] = wgx * Jw0[j] + wgy * Jw1[j];
            residualsPhoto[i] = weightedErrorPhoto;
            validPixelsPhoto[i] = 1;
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            float depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                float tdx = dgx.at(w.r, w.c), tdy = dgy.at(w.r, w.c);
                if (fabsf(tdx) < thrD && fabsf(tdy) < thrD) continue;
                float depthDiff = depth2 - w.dist;
                float stdDev_depth1 = stdDevDepth * depth2;
                float weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                float weightedErrorDepth = weight_depth * depthDiff;
                // jacobianDepthSrc = p'/dist ; (p'/dist) * jacobianT36
                float n0 = X * dist_inv, n1 = Y * dist_inv, n2 = Z * dist_inv;
                float nJ[6] = {n0, n1, n2, n1 * (-Z) + n2 * Y, n0 * Z + n2 * (-X), n0 * (-Y) + n1 * X};
                for (int j = 0; j < 6; ++j)
                    jacobiansDepth[(size_t)j * imgSize + i] = weight_depth * ((tdx * Jw0[j] + tdy * Jw1[j]) - nJ[j]);
                residualsDepth[i] = weightedErrorDepth;
                validPixelsDepth[i] = 1;
            }
        }
    }

    // RPI.h:3117-3195: 21 + 6 scalar reductions, float accumulators (reduce_mode 0) or double (1).
    float hf[21] = {0}, gf[6] = {0};
    double hd[21] = {0}, gd[6] = {0};
    auto reduce_rows = [&](const std::vector<float>& J, const std::vector<float>& res, const std::vector<int>& valid) {
        double H0[21] = {0}, G0[6] = {0};
#pragma omp parallel
        {
            float lh[21] = {0}, lg[6] = {0};
            double lhd[21] = {0}, lgd[6] = {0};
#pragma omp for schedule(static) nowait
            for (long i = 0; i < imgSize; ++i)
                if (valid[i]) {
                    float Ji[6];
                    for (int j = 0; j < 6; ++j) Ji[j] = J[(size_t)j * imgSize + i];
                    int k = 0;
                    for (int a = 0; a < 6; ++a)
                        for (int b = a; b < 6; ++b, ++k) {
                            float prod = Ji[a] * Ji[b];
                            lh[k] += prod;
                            lhd[k] += (double)prod;
                        }
                    for (int a = 0; a < 6; ++a) {
                        float prod = Ji[a] * res[i];
                        lg[a] += prod;
                        lgd[a] += (double)prod;
                    }
                }
#pragma omp critical
            {
                for (int k = 0; k < 21; ++k) { hf[k] += lh[k]; H0[k] += lhd[k]; }
                for (int a = 0; a < 6; ++a) { gf[a] += lg[a]; G0[a] += lgd[a]; }
            }
        }
        for (int k = 0; k < 21; ++k) hd[k] += H0[k];
        for (int a = 0; a < 6; ++a) gd[a] += G0[a];
    };
    if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) reduce_rows(jacobiansPhoto, residualsPhoto, validPixelsPhoto);
    if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) reduce_rows(jacobiansDepth, residualsDepth, validPixelsDepth);

    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++k) {
            float v = ctx.p.reduce_mode == 0 ? hf[k] : (float)hd[k];
            ctx.H[b * 6 + a] = ctx.H[a * 6 + b] = v;
            ctx.H64[b * 6 + a] = ctx.H64[a * 6 + b] = hd[k];
        }
    for (int a = 0; a < 6; ++a) {
        ctx.g[a] = ctx.p.reduce_mode == 0 ? gf[a] : (float)gd[a];
        ctx.g64[a] = gd[a];
    }
    ctx.n_visible = numVisiblePixels;
    ctx.sso = (float)numVisiblePixels / imgSize;  // RPI.h:3226
}

// ------------------------------------------------------------------------------------
// Occlusion-aware variants.  The reference runs their pixel loops under `#pragma omp parallel
// for` while the loop bodies read and write shared z-buffers / per-target rows without synchronisation, so the OpenMP
// build's results depend on thread timing.  What is restated here is the SEQUENTIAL semantics of the same source
// (ENABLE_OPENMP 0): pixels visited in index order.  RPI.h:4525 hard-codes thresDepthOutliers = 0.3.
// ------------------------------------------------------------------------------------
constexpr float kThresDepthOutliers = 0.3f;

struct OccSums {
    double photo = 0, depth = 0;    // sums of the squared weighted residuals
    long nPhoto = 0, nDepth = 0;
};

// RPI.h:3232-3367 errorPhotoICP_sphereOcc1: residuals and z-buffer indexed by the TARGET pixel; a closer (or equal)
// source pixel overwrites the residual, the counters count every write.  Returns avPhotoResidual + avDepthResidual
// (NaN when one of the two modalities is unused: 0/0 -- the reference's behaviour for PHOTO / DEPTH only).
double errorPhotoICP_sphereOcc1(Ctx& ctx, int level, const float* pose, int method, OccSums* out) {
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const long imgSize = (long)nRows * nCols;
    std::vector<float> residualsPhoto(imgSize, 0.f), residualsDepth(imgSize, 0.f), invDepthBuffer(imgSize, 0.f);
    const float angle_res = 2 * kPI / nCols;
    const float angle_res_inv = 1 / angle_res;
    const float half_nRows = 0.5 * nRows - 0.5;
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const double stdDevPhoto_inv = 1. / stdDevPhoto;
    const PoseRT T = split_pose(pose);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level], &dgx = ctx.dTrgGx[level], &dgy = ctx.dTrgGy[level];
    const float thrI = ctx.p.thres_sal_photo, thrD = ctx.p.thres_sal_depth;
    long nValidPhotoPts = 0, nValidDepthPts = 0;
    for (long i = 0; i < imgSize; ++i) {
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        Warp w = warp_pixel(T, p, nRows, nCols, half_nRows, angle_res_inv, ctx.p.math_mode);
        if (!w.visible) continue;
        const long ii = (long)w.r * nCols + w.c;
        if (invDepthBuffer[ii] > 0 && w.dist_inv < invDepthBuffer[ii]) continue;   // RPI.h:3297-3299
        invDepthBuffer[ii] = w.dist_inv;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            if (fabsf(gx.at(w.r, w.c)) < thrI && fabsf(gy.at(w.r, w.c)) < thrI) continue;
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            double weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            float weightedErrorPhoto = weight_photo * photoDiff;
            residualsPhoto[ii] = weightedErrorPhoto * weightedErrorPhoto;
            ++nValidPhotoPts;
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            float depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                if (fabsf(dgx.at(w.r, w.c)) < thrD && fabsf(dgy.at(w.r, w.c)) < thrD) continue;
                float depthDiff = depth2 - w.dist;
                float stdDev_depth1 = stdDevDepth * depth2;
                double weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                float weightedErrorDepth = weight_depth * depthDiff;
                residualsDepth[ii] = weightedErrorDepth * weightedErrorDepth;
                ++nValidDepthPts;
            }
        }
    }
    double PhotoResidual = 0.0, DepthResidual = 0.0;
    for (long i = 0; i < imgSize; ++i) {
        PhotoResidual += residualsPhoto[i];
        DepthResidual += residualsDepth[i];
    }
    if (out) { out->photo = PhotoResidual; out->depth = DepthResidual; out->nPhoto = nValidPhotoPts; out->nDepth = nValidDepthPts; }
    ctx.last_err2_photo = PhotoResidual; ctx.last_err2_depth = DepthResidual;
    ctx.last_nvalid_photo = nValidPhotoPts; ctx.last_nvalid_depth = nValidDepthPts;
    ctx.last_nvalid = nValidPhotoPts + nValidDepthPts;
    return sqrt(PhotoResidual / nValidPhotoPts) + sqrt(DepthResidual / nValidDepthPts);    // RPI.h:3358-3366
}

// RPI.h:3720-3856 errorPhotoICP_sphereOcc2: depth-outlier gate, z-buffer by TARGET pixel, residuals by SOURCE pixel
// (an accepted pixel is not retracted when a closer one arrives later); both averages divide by nValidDepthPts, which
// counts the accepted pixels before any saliency test.
double errorPhotoICP_sphereOcc2(Ctx& ctx, int level, const float* pose, int method, OccSums* out) {
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const long imgSize = (long)nRows * nCols;
    std::vector<float> residualsPhoto(imgSize, 0.f), residualsDepth(imgSize, 0.f), invDepthBuffer(imgSize, 0.f);
    const float angle_res = 2 * kPI / nCols;
    const float angle_res_inv = 1 / angle_res;
    const float half_nRows = 0.5 * nRows - 0.5;
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const double stdDevPhoto_inv = 1. / stdDevPhoto;
    const PoseRT T = split_pose(pose);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level], &dgx = ctx.dTrgGx[level], &dgy = ctx.dTrgGy[level];
    const float thrI = ctx.p.thres_sal_photo, thrD = ctx.p.thres_sal_depth;
    long nValidDepthPts = 0;
    for (long i = 0; i < imgSize; ++i) {
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        Warp w = warp_pixel(T, p, nRows, nCols, half_nRows, angle_res_inv, ctx.p.math_mode);
        if (!w.visible) continue;
        float depth2 = depthTrg.at(w.r, w.c);
        float depthDiff = depth2 - w.dist;
        if (fabsf(depthDiff) > kThresDepthOutliers) continue;                      // RPI.h:3788-3791
        const long ii = (long)w.r * nCols + w.c;
        if (invDepthBuffer[ii] > 0 && w.dist_inv < invDepthBuffer[ii]) continue;   // RPI.h:3794-3796
        invDepthBuffer[ii] = w.dist_inv;
        ++nValidDepthPts;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            if (fabsf(gx.at(w.r, w.c)) < thrI && fabsf(gy.at(w.r, w.c)) < thrI) continue;
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            double weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            float weightedErrorPhoto = weight_photo * photoDiff;
            residualsPhoto[i] = weightedErrorPhoto * weightedErrorPhoto;
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            if (std::isfinite(depth2)) {
                if (fabsf(dgx.at(w.r, w.c)) < thrD && fabsf(dgy.at(w.r, w.c)) < thrD) continue;
                float stdDev_depth1 = stdDevDepth * depth2;
                double weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                float weightedErrorDepth = weight_depth * depthDiff;
                residualsDepth[i] = weightedErrorDepth * weightedErrorDepth;
            }
        }
    }
    double PhotoResidual = 0.0, DepthResidual = 0.0;
    for (long i = 0; i < imgSize; ++i) {
        PhotoResidual += residualsPhoto[i];
        DepthResidual += residualsDepth[i];
    }
    if (out) { out->photo = PhotoResidual; out->depth = DepthResidual; out->nPhoto = nValidDepthPts; out->nDepth = nValidDepthPts; }
    ctx.last_err2_photo = PhotoResidual; ctx.last_err2_depth = DepthResidual;
    ctx.last_nvalid_photo = nValidDepthPts; ctx.last_nvalid_depth = nValidDepthPts;
    ctx.last_nvalid = nValidDepthPts;
    return sqrt(PhotoResidual / nValidDepthPts) + sqrt(DepthResidual / nValidDepthPts);     // RPI.h:3848-3855
}

// RPI.h:3373-3716 calcHessGrad_sphereOcc1 (occ == 1) and RPI.h:3861-4249 calcHessGrad_sphereOcc2 (occ == 2).
//  Occ1: the z-buffer is indexed by the SOURCE pixel (RPI.h:3473-3475), every pixel is visited once, so nothing is ever
//        rejected; rows are stored per source pixel.  Unlike the plain pass the rows are stored in one trailing block
//        (RPI.h:3575-3600), which a `continue` of the depth saliency test skips: a pixel whose depth gradient is not
//        salient loses its photometric row as well.
//  Occ2: depth-outlier gate, then rows are stored per TARGET pixel without a depth test (RPI.h:4096-4120): the pixel
//        visited last wins.  numVisiblePixels counts the distinct target pixels (RPI.h:3981-3982).
void calcHessGrad_sphereOcc(Ctx& ctx, int level, const float* pose, int method, int occ) {
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const long imgSize = (long)nRows * nCols;
    const float angle_res = 2 * kPI / nCols;
    const float angle_res_inv = 1 / angle_res;
    const float half_nRows = 0.5 * nRows - 0.5;
    std::vector<float> jacobiansPhoto((size_t)imgSize * 6), jacobiansDepth((size_t)imgSize * 6);
    std::vector<float> residualsPhoto(imgSize, 0.f), residualsDepth(imgSize, 0.f);
    std::vector<int> validPixelsPhoto(imgSize, 0), validPixelsDepth(imgSize, 0);
    std::vector<float> invDepthBuffer(imgSize, 0.f);
    const PoseRT T = split_pose(pose);
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const float stdDevPhoto_inv = 1. / stdDevPhoto;
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level], &dgx = ctx.dTrgGx[level], &dgy = ctx.dTrgGy[level];
    const float thrI = ctx.p.thres_sal_photo, thrD = ctx.p.thres_sal_depth;
    long numVisiblePixels = 0;
    for (long i = 0; i < imgSize; ++i) {
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        Warp w = warp_pixel(T, p, nRows, nCols, half_nRows, angle_res_inv, ctx.p.math_mode);
        if (!w.visible) continue;
        long row;       // where this pixel's rows are stored
        if (occ == 1) {
            if (invDepthBuffer[i] > 0 && w.dist_inv < invDepthBuffer[i]) continue;     // never true: one visit per i
            invDepthBuffer[i] = w.dist_inv;
            ++numVisiblePixels;
            row = i;
        } else {
            float depthDiff0 = depthTrg.at(w.r, w.c) - w.dist;
            if (fabsf(depthDiff0) > kThresDepthOutliers) continue;                     // RPI.h:3968-3979
            const long ii = (long)w.r * nCols + w.c;
            if (invDepthBuffer[ii] == 0) ++numVisiblePixels;
            invDepthBuffer[ii] = w.dist_inv;
            row = ii;
        }
        const float X = w.X, Y = w.Y, Z = w.Z, dist_inv = w.dist_inv;
        float Jw0[6], Jw1[6];
        warp_jacobian(X, Y, Z, dist_inv, angle_res_inv, Jw0, Jw1);
        float jacobianPhoto[6] = {0, 0, 0, 0, 0, 0}, jacobianDepth[6] = {0, 0, 0, 0, 0, 0};
        float weightedErrorPhoto = 0.f, weightedErrorDepth = 0.f, depth2 = 0.f;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            float tgx = gx.at(w.r, w.c), tgy = gy.at(w.r, w.c);
            if (fabsf(tgx) < thrI && fabsf(tgy) < thrI) continue;
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            float weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            weightedErrorPhoto = weight_photo * photoDiff;
            float wgx = weight_photo * tgx, wgy = weight_photo * tgy;
            for (int j = 0; j < 6; ++j) jacobianPhoto[j] = wgx * Jw0[j] + wgy * Jw1[j];
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                float tdx = dgx.at(w.r, w.c), tdy = dgy.at(w.r, w.c);
                if (fabsf(tdx) < thrD && fabsf(tdy) < thrD) continue;      // also skips the trailing store of the photo row
                float depthDiff = depth2 - w.dist;
                float stdDev_depth1 = stdDevDepth * depth2;
                float weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                weightedErrorDepth = weight_depth * depthDiff;
                float n0 = X * dist_inv, n1 = Y * dist_inv, n2 = Z * dist_inv;
                float nJ[6] = {n0, n1, n2, n1 * (-Z) + n2 * Y, n0 * Z + n2 * (-X), n0 * (-Y) + n1 * X};
                for (int j = 0; j < 6; ++j) jacobianDepth[j] = weight_depth * ((tdx * Jw0[j] + tdy * Jw1[j]) - nJ[j]);
            }
        }
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            for (int j = 0; j < 6; ++j) jacobiansPhoto[(size_t)j * imgSize + row] = jacobianPhoto[j];
            residualsPhoto[row] = weightedErrorPhoto;
            validPixelsPhoto[row] = 1;
        }
        if ((method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) && std::isfinite(depth2)) {
            for (int j = 0; j < 6; ++j) jacobiansDepth[(size_t)j * imgSize + row] = jacobianDepth[j];
            residualsDepth[row] = weightedErrorDepth;
            validPixelsDepth[row] = 1;
        }
    }
    float hf[21] = {0}, gf[6] = {0};
    double hd[21] = {0}, gd[6] = {0};
    auto reduce_rows = [&](const std::vector<float>& J, const std::vector<float>& res, const std::vector<int>& valid) {
        for (long i = 0; i < imgSize; ++i)
            if (valid[i]) {
                float Ji[6];
                for (int j = 0; j < 6; ++j) Ji[j] = J[(size_t)j * imgSize + i];
                int k = 0;
                for (int a = 0; a < 6; ++a)
                    for (int b = a; b < 6; ++b, ++k) {
                        float prod = Ji[a] * Ji[b];
                        hf[k] += prod;
                        hd[k] += (double)prod;
                    }
                for (int a = 0; a < 6; ++a) {
                    float prod = Ji[a] * res[i];
                    gf[a] += prod;
                    gd[a] += (double)prod;
                }
            }
    };
    if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) reduce_rows(jacobiansPhoto, residualsPhoto, validPixelsPhoto);
    if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) reduce_rows(jacobiansDepth, residualsDepth, validPixelsDepth);
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++k) {
            float v = ctx.p.reduce_mode == 0 ? hf[k] : (float)hd[k];
            ctx.H[b * 6 + a] = ctx.H[a * 6 + b] = v;
            ctx.H64[b * 6 + a] = ctx.H64[a * 6 + b] = hd[k];
        }
    for (int a = 0; a < 6; ++a) {
        ctx.g[a] = ctx.p.reduce_mode == 0 ? gf[a] : (float)gd[a];
        ctx.g64[a] = gd[a];
    }
    ctx.n_visible = numVisiblePixels;
    ctx.sso = (float)numVisiblePixels / imgSize;
}

// ------------------------------------------------------------------------------------
// THIRD-PARTY restatements (Eigen / MRPT) for the 6x6 step
// ------------------------------------------------------------------------------------

// MRPT 1.x Eigen plugin rank(): ColPivHouseholderQR(m).rank() with Eigen's default threshold
// epsilon * diagonalSize; a pivot counts if |R_ii| > |maxpivot| * threshold.  (RPI.h:4682)
int rank6_colpiv_qr(const float* Mcm /*col-major 6x6*/) {
    float A[6][6];
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) A[r][c] = Mcm[c * 6 + r];
    float colNormsSq[6];
    for (int c = 0; c < 6; ++c) {
        float s = 0;
        for (int r = 0; r < 6; ++r) s += A[r][c] * A[r][c];
        colNormsSq[c] = s;
    }
    float maxNormSq = *std::max_element(colNormsSq, colNormsSq + 6);
    const float eps = 1.1920929e-07f;
    float threshold_helper = maxNormSq * (eps * eps) / 6.f;  // Eigen 3.2: maxCoeff * abs2(eps) / rows
    int nonzero_pivots = 6;
    float maxpivot = 0.f;
    float diag[6] = {0};
    for (int k = 0; k < 6; ++k) {
        int best = k;
        float bestv = -1.f;
        for (int c = k; c < 6; ++c) {
            float s = 0;
            for (int r = k; r < 6; ++r) s += A[r][c] * A[r][c];  // recompute exactly
            if (s > bestv) { bestv = s; best = c; }
        }
        if (bestv < threshold_helper * (float)(6 - k)) { nonzero_pivots = k; break; }
        if (best != k)
            for (int r = 0; r < 6; ++r) std::swap(A[r][k], A[r][best]);
        // Householder on column k, rows k..5
        float tailSq = 0;
        for (int r = k + 1; r < 6; ++r) tailSq += A[r][k] * A[r][k];
        float c0 = A[k][k], beta, tau;
        float v[6] = {0};
        if (tailSq == 0.f) {
            tau = 0.f;
            beta = c0;
        } else {
            beta = sqrtf(c0 * c0 + tailSq);
            if (c0 >= 0.f) beta = -beta;
            for (int r = k + 1; r < 6; ++r) v[r] = A[r][k] / (c0 - beta);
            tau = (beta - c0) / beta;
        }
        v[k] = 1.f;
        for (int c = k + 1; c < 6; ++c) {
            float dot = 0;
            for (int r = k; r < 6; ++r) dot += v[r] * A[r][c];
            dot *= tau;
            for (int r = k; r < 6; ++r) A[r][c] -= dot * v[r];
        }
        A[k][k] = beta;
        for (int r = k + 1; r < 6; ++r) A[r][k] = 0.f;
        diag[k] = beta;
        if (fabsf(beta) > maxpivot) maxpivot = fabsf(beta);
    }
    float thr = maxpivot * (eps * 6.f);
    int rank = 0;
    for (int k = 0; k < nonzero_pivots; ++k) rank += (fabsf(diag[k]) > thr);
    return rank;
}

// Eigen Matrix<float,6,6>::inverse(): PartialPivLU, then solve against identity. (RPI.h:4693)
bool inverse6_partial_piv_lu(const float* Mcm, float* inv_cm) {
    float LU[6][6];
    int perm[6];
    for (int r = 0; r < 6; ++r) {
        perm[r] = r;
        for (int c = 0; c < 6; ++c) LU[r][c] = Mcm[c * 6 + r];
    }
    for (int k = 0; k < 6; ++k) {
        int piv = k;
        float best = fabsf(LU[k][k]);
        for (int r = k + 1; r < 6; ++r)
            if (fabsf(LU[r][k]) > best) { best = fabsf(LU[r][k]); piv = r; }
        if (best == 0.f) return false;
        if (piv != k) {
            for (int c = 0; c < 6; ++c) std::swap(LU[k][c], LU[piv][c]);
            std::swap(perm[k], perm[piv]);
        }
        for (int r = k + 1; r < 6; ++r) {
            LU[r][k] /= LU[k][k];
            for (int c = k + 1; c < 6; ++c) LU[r][c] -= LU[r][k] * LU[k][c];
        }
    }
    for (int col = 0; col < 6; ++col) {
        float y[6];
        for (int r = 0; r < 6; ++r) {  // forward: L y = P e_col
            float s = (perm[r] == col) ? 1.f : 0.f;
            for (int c = 0; c < r; ++c) s -= LU[r][c] * y[c];
            y[r] = s;
        }
        for (int r = 5; r >= 0; --r) {  // backward: U x = y
            float s = y[r];
            for (int c = r + 1; c < 6; ++c) s -= LU[r][c] * y[c];
            y[r] = s / LU[r][r];
        }
        for (int r = 0; r < 6; ++r) inv_cm[col * 6 + r] = y[r];
    }
    return true;
}

// MRPT 1.x CPose3D::exp(v, pseudo_exponential = true)  (SE_traits<3>::pseudo_exp): translation copied
// verbatim from v[0..2], rotation = Rodrigues(v[3..5]) = I + sin(a)/a W + (1-cos(a))/a^2 W^2. (RPI.h:4697)
void se3_pseudo_exp(const double* v, double* M /*col-major 4x4*/) {
    const double wx = v[3], wy = v[4], wz = v[5];
    const double angle = sqrt(wx * wx + wy * wy + wz * wz);
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    if (angle >= 128 * 2.220446049250313e-16) {
        const double W[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
        double W2[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s = 0;
                for (int k = 0; k < 3; ++k) s += W[i][k] * W[k][j];
                W2[i][j] = s;
            }
        const double a = sin(angle) / angle, b = (1 - cos(angle)) / (angle * angle);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] += a * W[i][j] + b * W2[i][j];
    }
    for (int k = 0; k < 16; ++k) M[k] = 0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) M[j * 4 + i] = R[i][j];
        M[12 + i] = v[i];
    }
    M[15] = 1;
}

inline void mat4_mul_f32(const float* A, const float* B, float* C) {  // col-major, Eigen coefficient order
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r)
            C[c * 4 + r] = ((A[0 * 4 + r] * B[c * 4 + 0] + A[1 * 4 + r] * B[c * 4 + 1]) + A[2 * 4 + r] * B[c * 4 + 2]) +
                           A[3 * 4 + r] * B[c * 4 + 3];
}

// ====================================================================================
// Pinhole single-sensor path: alignFrames RPI.h:4254-4512 with errorPhotoICP RPI.h:560-748 and
// calcHessGrad RPI.h:754-1104 (occlusion 0, bUseSalientPixels false = the constructor default RPI.h:205).
// ====================================================================================
struct PinholeK {
    float fx, fy, ox, oy;
};
inline PinholeK level_intrinsics(const Ctx& ctx, int level) {   // RPI.h:571-575
    const float scaleFactor = 1.0 / pow(2, level);
    return {ctx.cam[0] * scaleFactor, ctx.cam[1] * scaleFactor, ctx.cam[2] * scaleFactor, ctx.cam[3] * scaleFactor};
}

// RPI.h:4277-4300: LUT of the source sensor's 3-D points; z is written for every pixel, x = INVALID marks bad depth
void buildLUT_pinhole(Ctx& ctx, int level) {
    const Image& depth = ctx.depthSrc[level];
    const int nRows = depth.rows, nCols = depth.cols;
    ctx.lut.assign((size_t)nRows * nCols * 3, 0.f);
    const PinholeK K = level_intrinsics(ctx, level);
    const float inv_fx = 1. / K.fx, inv_fy = 1. / K.fy;
    for (int r = 0; r < nRows; ++r)
        for (int c = 0; c < nCols; ++c) {
            const size_t i = (size_t)r * nCols + c;
            float* P = &ctx.lut[3 * i];
            P[2] = depth.at(r, c);
            if (ctx.p.min_depth < P[2] && P[2] < ctx.p.max_depth) {
                P[0] = (c - K.ox) * P[2] * inv_fx;
                P[1] = (r - K.oy) * P[2] * inv_fy;
            } else
                P[0] = kInvalidPoint;
        }
    ctx.lut_level = 1000 + level;
}

struct WarpPin {
    float X, Y, Z, inv_z;
    int r, c;
    bool visible;
};
inline WarpPin warp_pinhole(const PoseRT& T, const float* p, int nRows, int nCols, const PinholeK& K, int math_mode) {
    WarpPin w;
    float tr, tc;
    if (math_mode == 0) {       // RPI.h:701-708
        w.X = ((T.R[0] * p[0] + T.R[1] * p[1]) + T.R[2] * p[2]) + T.t[0];
        w.Y = ((T.R[3] * p[0] + T.R[4] * p[1]) + T.R[5] * p[2]) + T.t[1];
        w.Z = ((T.R[6] * p[0] + T.R[7] * p[1]) + T.R[8] * p[2]) + T.t[2];
        w.inv_z = 1.0 / w.Z;
        tc = (w.X * K.fx) * w.inv_z + K.ox;
        tr = (w.Y * K.fy) * w.inv_z + K.oy;
        if (!std::isfinite(tr) || !std::isfinite(tc)) { w.visible = false; w.r = w.c = -1; return w; }   // (int)round(inf) is UB in C++
        w.r = (int)roundf(tr);
        w.c = (int)roundf(tc);
    } else {                    // device arithmetic (occlusion-free pinhole kernels): fma rotation, fma projection, round half up
        w.X = fmaf(T.R[2], p[2], fmaf(T.R[1], p[1], fmaf(T.R[0], p[0], T.t[0])));
        w.Y = fmaf(T.R[5], p[2], fmaf(T.R[4], p[1], fmaf(T.R[3], p[0], T.t[1])));
        w.Z = fmaf(T.R[8], p[2], fmaf(T.R[7], p[1], fmaf(T.R[6], p[0], T.t[2])));
        w.inv_z = 1.f / w.Z;
        tc = fmaf(w.X * K.fx, w.inv_z, K.ox);
        tr = fmaf(w.Y * K.fy, w.inv_z, K.oy);
        if (!(fabsf(tr) < 1e9f) || !(fabsf(tc) < 1e9f)) { w.visible = false; w.r = w.c = -1; return w; }
        w.r = round_index(tr);
        w.c = round_index(tc);
    }
    w.visible = (w.r >= 0 && w.r < nRows) && (w.c >= 0 && w.c < nCols);
    return w;
}

// RPI.h:560-748 errorPhotoICP (else-branch :693-739: every valid LUT point, NO saliency test).  Both averages divide by
// nValidDepthPts (RPI.h:742-743): with PHOTO_CONSISTENCY alone the result is inf + NaN = NaN.
double errorPhotoICP(Ctx& ctx, int level, const float* pose, int method) {
    double PhotoResidual = 0.0, DepthResidual = 0.0;
    long nValidPhotoPts = 0, nValidDepthPts = 0;
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const PinholeK K = level_intrinsics(ctx, level);
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const float stdDevPhoto_inv = 1. / stdDevPhoto;
    const PoseRT T = split_pose(pose);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const long n = (long)nRows * nCols;
#pragma omp parallel for reduction(+ : PhotoResidual, DepthResidual, nValidPhotoPts, nValidDepthPts)
    for (long i = 0; i < n; ++i) {
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        const WarpPin w = warp_pinhole(T, p, nRows, nCols, K, ctx.p.math_mode);
        if (!w.visible) continue;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            float weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            float weightedErrorPhoto = weight_photo * photoDiff;
            PhotoResidual += weightedErrorPhoto * weightedErrorPhoto;
            ++nValidPhotoPts;
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            float depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                float depth1 = w.Z;
                float depthDiff = depth2 - depth1;
                float stdDev_depth1 = stdDevDepth * depth1;
                float weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                float weightedErrorDepth = weight_depth * depthDiff;
                DepthResidual += weightedErrorDepth * weightedErrorDepth;
                ++nValidDepthPts;
            }
        }
    }
    ctx.last_err2_photo = PhotoResidual; ctx.last_err2_depth = DepthResidual;
    ctx.last_nvalid_photo = nValidPhotoPts; ctx.last_nvalid_depth = nValidDepthPts;
    ctx.last_nvalid = nValidPhotoPts + nValidDepthPts;
    return sqrt(PhotoResidual / nValidDepthPts) + sqrt(DepthResidual / nValidDepthPts);
}

// RPI.h:754-1104 calcHessGrad: H += J^T J, g += J^T r per pixel (float, under `omp critical`: summation order = arrival
// order; reduce_mode 0 restates the index order, reduce_mode 1 accumulates the same float products in double).
void calcHessGrad(Ctx& ctx, int level, const float* pose, int method) {
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const long imgSize = (long)nRows * nCols;
    const PinholeK K = level_intrinsics(ctx, level);
    const float fx = K.fx, fy = K.fy;
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const float stdDevPhoto_inv = 1. / stdDevPhoto;
    const PoseRT T = split_pose(pose);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level], &dgx = ctx.dTrgGx[level], &dgy = ctx.dTrgGy[level];
    const float thrI = ctx.p.thres_sal_photo, thrD = ctx.p.thres_sal_depth;
    float Hf[36] = {0}, gf[6] = {0};
    double Hd[36] = {0}, gd[6] = {0};
    long rows_used = 0;
    auto add_row = [&](const float* J, float res) {
        for (int a = 0; a < 6; ++a) {
            for (int b = 0; b < 6; ++b) {
                const float prod = J[a] * J[b];
                Hf[b * 6 + a] += prod;
                Hd[b * 6 + a] += (double)prod;
            }
            const float pr = J[a] * res;
            gf[a] += pr;
            gd[a] += (double)pr;
        }
        ++rows_used;
    };
    for (long i = 0; i < imgSize; ++i) {
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        const WarpPin w = warp_pinhole(T, p, nRows, nCols, K, ctx.p.math_mode);
        if (!w.visible) continue;
        const float X = w.X, Y = w.Y, inv_transformedPz = w.inv_z;
        // jacobianWarpRt RPI.h:876-893
        float Jw0[6], Jw1[6];
        Jw0[0] = fx * inv_transformedPz;
        Jw1[0] = 0;
        Jw0[1] = 0;
        Jw1[1] = fy * inv_transformedPz;
        const float inv_transformedPz_2 = inv_transformedPz * inv_transformedPz;
        Jw0[2] = -fx * X * inv_transformedPz_2;
        Jw1[2] = -fy * Y * inv_transformedPz_2;
        Jw0[3] = -fx * Y * X * inv_transformedPz_2;
        Jw1[3] = -fy * (1 + Y * Y * inv_transformedPz_2);
        Jw0[4] = fx * (1 + X * X * inv_transformedPz_2);
        Jw1[4] = fy * X * Y * inv_transformedPz_2;
        Jw0[5] = -fx * Y * inv_transformedPz;
        Jw1[5] = fy * X * inv_transformedPz;
        float jacobianPhoto[6] = {0, 0, 0, 0, 0, 0}, jacobianDepth[6] = {0, 0, 0, 0, 0, 0};
        float weightedErrorPhoto = 0.f, weightedErrorDepth = 0.f;
        float depth2 = std::numeric_limits<float>::quiet_NaN();   // the reference leaves it uninitialised for PHOTO only; see note below
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            const float tgx = gx.at(w.r, w.c), tgy = gy.at(w.r, w.c);
            if (fabsf(tgx) < thrI && fabsf(tgy) < thrI) continue;
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            float weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            weightedErrorPhoto = weight_photo * photoDiff;
            const float wgx = weight_photo * tgx, wgy = weight_photo * tgy;
            for (int j = 0; j < 6; ++j) jacobianPhoto[j] = wgx * Jw0[j] + wgy * Jw1[j];
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            const float tdx = dgx.at(w.r, w.c), tdy = dgy.at(w.r, w.c);
            if (fabsf(tdx) < thrD && fabsf(tdy) < thrD) continue;       // RPI.h:929-930: before the finite test, skips the photo row too
            depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                float depthDiff = depth2 - w.Z;
                float stdDev_depth1 = stdDevDepth * w.Z;
                float weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                weightedErrorDepth = weight_depth * depthDiff;
                const float jacobianRt_z[6] = {0, 0, 1, Y, -X, 0};
                for (int j = 0; j < 6; ++j) jacobianDepth[j] = weight_depth * ((tdx * Jw0[j] + tdy * Jw1[j]) - jacobianRt_z[j]);
            }
        }
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) add_row(jacobianPhoto, weightedErrorPhoto);
        if ((method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) && std::isfinite(depth2)) add_row(jacobianDepth, weightedErrorDepth);
    }
    for (int k = 0; k < 36; ++k) {
        ctx.H[k] = ctx.p.reduce_mode == 0 ? Hf[k] : (float)Hd[k];
        ctx.H64[k] = Hd[k];
    }
    for (int a = 0; a < 6; ++a) {
        ctx.g[a] = ctx.p.reduce_mode == 0 ? gf[a] : (float)gd[a];
        ctx.g64[a] = gd[a];
    }
    ctx.n_visible = rows_used;
    ctx.sso = 0.f;
}

// RPI.h:401-425 calcGradientXY_saliency's pixel list: the gradient images are calcGradientXY's (same expressions), the list holds
// the interior pixels of the TARGET's gray image with |gx| > thresSaliency or |gy| > thresSaliency, in index order.
void buildSalientPixels(Ctx& ctx, int level) {
    if ((int)ctx.salient.size() < ctx.p.n_pyr) ctx.salient.resize(ctx.p.n_pyr);
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level];
    std::vector<int>& v = ctx.salient[level];
    v.clear();
    for (int r = 1; r < gx.rows - 1; ++r)
        for (int c = 1; c < gx.cols - 1; ++c)
            if (fabsf(gx.at(r, c)) > ctx.thres_saliency || fabsf(gy.at(r, c)) > ctx.thres_saliency) v.push_back(gx.cols * r + c);
}

// RPI.h:590-690: errorPhotoICP with bUseSalientPixels -- the same residuals over the pixels of vSalientPixels only.  The list was
// built from the TARGET's gradients (RPI.h:445-446) and is used here to index the SOURCE's LUT and intensities (RPI.h:613-634):
// restated as written.  calcHessGrad's corresponding branch is commented out (RPI.h:813-870): H, g use every pixel.
double errorPhotoICP_salient(Ctx& ctx, int level, const float* pose, int method) {
    double PhotoResidual = 0.0, DepthResidual = 0.0;
    long nValidPhotoPts = 0, nValidDepthPts = 0;
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const PinholeK K = level_intrinsics(ctx, level);
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const float stdDevPhoto_inv = 1. / stdDevPhoto;
    const PoseRT T = split_pose(pose);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    buildSalientPixels(ctx, level);
    for (int i : ctx.salient[level]) {
        const float* p = &ctx.lut[3 * (size_t)i];
        if (p[0] == kInvalidPoint) continue;
        const WarpPin w = warp_pinhole(T, p, nRows, nCols, K, ctx.p.math_mode);
        if (!w.visible) continue;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            float weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            float weightedErrorPhoto = weight_photo * photoDiff;
            PhotoResidual += weightedErrorPhoto * weightedErrorPhoto;
            ++nValidPhotoPts;
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            float depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                float depth1 = w.Z;
                float depthDiff = depth2 - depth1;
                float stdDev_depth1 = stdDevDepth * depth1;
                float weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                float weightedErrorDepth = weight_depth * depthDiff;
                DepthResidual += weightedErrorDepth * weightedErrorDepth;
                ++nValidDepthPts;
            }
        }
    }
    ctx.last_err2_photo = PhotoResidual; ctx.last_err2_depth = DepthResidual;
    ctx.last_nvalid_photo = nValidPhotoPts; ctx.last_nvalid_depth = nValidDepthPts;
    ctx.last_nvalid = nValidPhotoPts + nValidDepthPts;
    return sqrt(PhotoResidual / nValidDepthPts) + sqrt(DepthResidual / nValidDepthPts);       // RPI.h:742-744
}

// ------------------------------------------------------------------------------------
// Pinhole occlusion-aware variants (RPI.h:1107-2040; no application calls them: MethodsRegisterRGBD360.cpp:348 passes occlusion 0).
// As for the spherical ones the SEQUENTIAL semantics of the source are restated (pixels in index order; the OpenMP build races on
// the z-buffer).  Defects of the source, and what is done about each:
//   * errorPhotoICP_Occ2's outlier gate compares the target DEPTH with the transformed point's INVERSE depth (RPI.h:1687-1690):
//     restated as written.
//   * calcHessGrad_Occ1/2 sum a pixel's depth row only where its PHOTOMETRIC residual is non-zero (RPI.h:1530-1535, 2008-2013:
//     `residualsPhoto(i) != 0` in both loops), so DEPTH_CONSISTENCY alone yields H = 0 (-> ILL-POSED): restated as written.
//   * calcHessGrad_Occ2 writes mask_dynamic_occlusion, which only exists when visualizeIterations is set (RPI.h:1805, 1872-1876:
//     an out-of-bounds write otherwise), and asserts on a NaN target depth (RPI.h:1964-1965): neither has an effect on H, g;
//     the mask is not restated and the NaN case is the no-op it is under NDEBUG.
//   * numVisiblePixels counts a target pixel's first arrival twice (RPI.h:1421-1430, 1866-1879): restated as written.
// thresDepthOutliers: alignFrames(occlusion 2) sets it to maxDepthOutliers = 1 m (RPI.h:215, 4256-4260).
// ------------------------------------------------------------------------------------
constexpr float kPinThresDepthOutliers = 1.f;

// RPI.h:1107-1325 errorPhotoICP_Occ1 (occ 1), RPI.h:1547-1775 errorPhotoICP_Occ2 (occ 2): z-buffer and residuals indexed by the
// TARGET pixel; a source pixel at least as close as the z-buffer's entry overwrites the residual, the counters count every write.
double errorPhotoICP_Occ(Ctx& ctx, int level, const float* pose, int method, int occ, OccSums* out) {
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const long imgSize = (long)nRows * nCols;
    std::vector<float> residualsPhoto(imgSize, 0.f), residualsDepth(imgSize, 0.f), invDepthBuffer(imgSize, 0.f);
    const PinholeK K = level_intrinsics(ctx, level);
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const float stdDevPhoto_inv = 1. / stdDevPhoto;
    const PoseRT T = split_pose(pose);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level], &dgx = ctx.dTrgGx[level], &dgy = ctx.dTrgGy[level];
    const float thrI = ctx.p.thres_sal_photo, thrD = ctx.p.thres_sal_depth;
    long nValidPhotoPts = 0, nValidDepthPts = 0;
    for (long i = 0; i < imgSize; ++i) {
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        const WarpPin w = warp_pinhole(T, p, nRows, nCols, K, ctx.p.math_mode);
        if (!w.visible) continue;
        const float inv_transformedPz = w.inv_z;
        if (occ == 2) {
            float depth2 = depthTrg.at(w.r, w.c);
            float depthDiff = depth2 - inv_transformedPz;                              // RPI.h:1687-1690 (sic)
            if (fabsf(depthDiff) > kPinThresDepthOutliers) continue;
        }
        const long ii = (long)w.r * nCols + w.c;
        if (invDepthBuffer[ii] > 0 && inv_transformedPz < invDepthBuffer[ii]) continue;    // RPI.h:1248-1250, 1693-1695
        invDepthBuffer[ii] = inv_transformedPz;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            if (fabsf(gx.at(w.r, w.c)) < thrI && fabsf(gy.at(w.r, w.c)) < thrI) continue;
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            float weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            float weightedErrorPhoto = weight_photo * photoDiff;
            residualsPhoto[ii] = weightedErrorPhoto * weightedErrorPhoto;
            ++nValidPhotoPts;
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            float depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                if (fabsf(dgx.at(w.r, w.c)) < thrD && fabsf(dgy.at(w.r, w.c)) < thrD) continue;
                float depth1 = w.Z;
                float depthDiff = depth2 - depth1;
                float stdDev_depth1 = stdDevDepth * depth1;
                float weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                float weightedErrorDepth = weight_depth * depthDiff;
                residualsDepth[ii] = weightedErrorDepth * weightedErrorDepth;
                ++nValidDepthPts;
            }
        }
    }
    double PhotoResidual = 0.0, DepthResidual = 0.0;
    for (long i = 0; i < imgSize; ++i) {
        PhotoResidual += residualsPhoto[i];
        DepthResidual += residualsDepth[i];
    }
    if (out) { out->photo = PhotoResidual; out->depth = DepthResidual; out->nPhoto = nValidPhotoPts; out->nDepth = nValidDepthPts; }
    ctx.last_err2_photo = PhotoResidual; ctx.last_err2_depth = DepthResidual;
    ctx.last_nvalid_photo = nValidPhotoPts; ctx.last_nvalid_depth = nValidDepthPts;
    ctx.last_nvalid = nValidPhotoPts + nValidDepthPts;
    return sqrt(PhotoResidual / nValidPhotoPts) + sqrt(DepthResidual / nValidDepthPts);    // RPI.h:1314-1317, 1765-1768
}

// RPI.h:1328-1544 calcHessGrad_Occ1 (occ 1), RPI.h:1777-2030 calcHessGrad_Occ2 (occ 2): z-buffer by TARGET pixel, rows stored by
// SOURCE pixel (an accepted pixel's rows stay when a closer one arrives later); occ 2 adds the depth-outlier gate.
void calcHessGrad_Occ(Ctx& ctx, int level, const float* pose, int method, int occ) {
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const long imgSize = (long)nRows * nCols;
    const PinholeK K = level_intrinsics(ctx, level);
    const float fx = K.fx, fy = K.fy;
    std::vector<float> jacobiansPhoto((size_t)imgSize * 6, 0.f), jacobiansDepth((size_t)imgSize * 6, 0.f);
    std::vector<float> residualsPhoto(imgSize, 0.f), residualsDepth(imgSize, 0.f), invDepthBuffer(imgSize, 0.f);
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const float stdDevPhoto_inv = 1. / stdDevPhoto;
    const PoseRT T = split_pose(pose);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level], &dgx = ctx.dTrgGx[level], &dgy = ctx.dTrgGy[level];
    const float thrI = ctx.p.thres_sal_photo, thrD = ctx.p.thres_sal_depth;
    long numVisiblePixels = 0;
    for (long i = 0; i < imgSize; ++i) {
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        const WarpPin w = warp_pinhole(T, p, nRows, nCols, K, ctx.p.math_mode);
        if (!w.visible) continue;
        const float X = w.X, Y = w.Y, Z = w.Z, inv_transformedPz = w.inv_z;
        if (occ == 2) {
            float depth2 = depthTrg.at(w.r, w.c);
            float depthDiff = depth2 - Z;                                              // RPI.h:1857-1862
            if (fabsf(depthDiff) > kPinThresDepthOutliers) continue;
        }
        const long ii = (long)w.r * nCols + w.c;
        if (invDepthBuffer[ii] == 0)                                                   // RPI.h:1421-1430, 1866-1879
            ++numVisiblePixels;
        else if (inv_transformedPz < invDepthBuffer[ii])
            continue;
        ++numVisiblePixels;
        invDepthBuffer[ii] = inv_transformedPz;
        float Jw0[6], Jw1[6];                                                          // jacobianWarpRt RPI.h:1435-1452
        Jw0[0] = fx * inv_transformedPz;
        Jw1[0] = 0;
        Jw0[1] = 0;
        Jw1[1] = fy * inv_transformedPz;
        const float inv_transformedPz_2 = inv_transformedPz * inv_transformedPz;
        Jw0[2] = -fx * X * inv_transformedPz_2;
        Jw1[2] = -fy * Y * inv_transformedPz_2;
        Jw0[3] = -fx * Y * X * inv_transformedPz_2;
        Jw1[3] = -fy * (1 + Y * Y * inv_transformedPz_2);
        Jw0[4] = fx * (1 + X * X * inv_transformedPz_2);
        Jw1[4] = fy * X * Y * inv_transformedPz_2;
        Jw0[5] = -fx * Y * inv_transformedPz;
        Jw1[5] = fy * X * inv_transformedPz;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            const float tgx = gx.at(w.r, w.c), tgy = gy.at(w.r, w.c);
            if (fabsf(tgx) < thrI && fabsf(tgy) < thrI) continue;
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            float weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            float weightedErrorPhoto = weight_photo * photoDiff;
            const float wgx = weight_photo * tgx, wgy = weight_photo * tgy;
            for (int j = 0; j < 6; ++j) jacobiansPhoto[(size_t)i * 6 + j] = wgx * Jw0[j] + wgy * Jw1[j];
            residualsPhoto[i] = weightedErrorPhoto;
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            const float tdx = dgx.at(w.r, w.c), tdy = dgy.at(w.r, w.c);
            if (fabsf(tdx) < thrD && fabsf(tdy) < thrD) continue;
            float depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                float depthDiff = depth2 - Z;
                float stdDev_depth1 = stdDevDepth * Z;
                float weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                float weightedErrorDepth = weight_depth * depthDiff;
                const float jacobianRt_z[6] = {0, 0, 1, Y, -X, 0};
                for (int j = 0; j < 6; ++j) jacobiansDepth[(size_t)i * 6 + j] = weight_depth * ((tdx * Jw0[j] + tdy * Jw1[j]) - jacobianRt_z[j]);
                residualsDepth[i] = weightedErrorDepth;
            }
        }
    }
    float Hf[36] = {0}, gf[6] = {0};
    double Hd[36] = {0}, gd[6] = {0};
    long rows_used = 0;
    auto reduce_rows = [&](const std::vector<float>& Jm, const std::vector<float>& res) {
        for (long i = 0; i < imgSize; ++i)
            if (residualsPhoto[i] != 0) {                                              // RPI.h:1523, 1531 (both loops test the photo residual)
                const float* J = &Jm[(size_t)i * 6];
                for (int a = 0; a < 6; ++a) {
                    for (int b = 0; b < 6; ++b) {
                        const float prod = J[a] * J[b];
                        Hf[b * 6 + a] += prod;
                        Hd[b * 6 + a] += (double)prod;
                    }
                    const float pr = J[a] * res[i];
                    gf[a] += pr;
                    gd[a] += (double)pr;
                }
                ++rows_used;
            }
    };
    if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) reduce_rows(jacobiansPhoto, residualsPhoto);
    if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) reduce_rows(jacobiansDepth, residualsDepth);
    for (int k = 0; k < 36; ++k) {
        ctx.H[k] = ctx.p.reduce_mode == 0 ? Hf[k] : (float)Hd[k];
        ctx.H64[k] = Hd[k];
    }
    for (int a = 0; a < 6; ++a) {
        ctx.g[a] = ctx.p.reduce_mode == 0 ? gf[a] : (float)gd[a];
        ctx.g64[a] = gd[a];
    }
    ctx.n_visible = numVisiblePixels;
    if (occ == 2) ctx.sso = (float)numVisiblePixels / imgSize;                         // RPI.h:2016 (Occ1 leaves SSO alone)
}

// THIRD-PARTY (MRPT 1.x CPose3D::exp(mu, pseudo_exponential = false), RPI.h:4358, 4391): the SE(3) exponential with
// the translation coupled through V(w): t = u + B (w x u) + C (w x (w x u)); small-angle series below theta^2 < 1e-8 /
// 1e-6 as in MRPT's (TooN-derived) implementation.
void se3_exp(const double* v, double* M /*col-major 4x4*/) {
    const double ux = v[0], uy = v[1], uz = v[2], wx = v[3], wy = v[4], wz = v[5];
    const double theta_sq = wx * wx + wy * wy + wz * wz;
    const double theta = sqrt(theta_sq);
    const double cx = wy * uz - wz * uy, cy = wz * ux - wx * uz, cz = wx * uy - wy * ux;      // w x u
    double A, B, tx, ty, tz;
    if (theta_sq < 1e-8) {
        A = 1.0 - theta_sq / 6.0;
        B = 0.5;
        tx = ux + 0.5 * cx; ty = uy + 0.5 * cy; tz = uz + 0.5 * cz;
    } else {
        double C;
        if (theta_sq < 1e-6) {
            C = (1.0 / 6.0) * (1.0 - theta_sq / 20.0);
            A = 1.0 - theta_sq * C;
            B = 0.5 - 0.25 * (1.0 / 6.0) * theta_sq;
        } else {
            const double inv_theta = 1.0 / theta;
            A = sin(theta) * inv_theta;
            B = (1 - cos(theta)) * (inv_theta * inv_theta);
            C = (1 - A) * (inv_theta * inv_theta);
        }
        const double dx = wy * cz - wz * cy, dy = wz * cx - wx * cz, dz = wx * cy - wy * cx;  // w x (w x u)
        tx = ux + B * cx + C * dx; ty = uy + B * cy + C * dy; tz = uz + B * cz + C * dz;
    }
    // rodrigues_so3_exp(w, A, B)
    const double wx2 = wx * wx, wy2 = wy * wy, wz2 = wz * wz;
    double R[3][3];
    R[0][0] = 1.0 - B * (wy2 + wz2);
    R[1][1] = 1.0 - B * (wx2 + wz2);
    R[2][2] = 1.0 - B * (wx2 + wy2);
    { const double a = A * wz, b = B * (wx * wy); R[0][1] = b - a; R[1][0] = b + a; }
    { const double a = A * wy, b = B * (wx * wz); R[0][2] = b + a; R[2][0] = b - a; }
    { const double a = A * wx, b = B * (wy * wz); R[1][2] = b - a; R[2][1] = b + a; }
    for (int k = 0; k < 16; ++k) M[k] = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[j * 4 + i] = R[i][j];
    M[12] = tx; M[13] = ty; M[14] = tz;
    M[15] = 1;
}

// One Gauss-Newton step from (H, g) at pose: returns 0 ok / 1 ill-posed. RPI.h:4682-4697.
int gn_step(const float* H, const float* g, float lambda, const float* pose, float* pose_tmp, float* update) {
    float M[36];
    for (int k = 0; k < 36; ++k) M[k] = H[k];
    for (int i = 0; i < 6; ++i) M[i * 6 + i] = H[i * 6 + i] + lambda * H[i * 6 + i];
    if (rank6_colpiv_qr(M) != 6) return 1;
    float inv[36];
    if (!inverse6_partial_piv_lu(H, inv)) return 1;
    for (int r = 0; r < 6; ++r) {  // update = (-H^-1) * g
        float s = 0.f;
        for (int c = 0; c < 6; ++c) s += (-inv[c * 6 + r]) * g[c];
        update[r] = s;
    }
    double ud[6], E[16];
    for (int i = 0; i < 6; ++i) ud[i] = (double)update[i];
    se3_pseudo_exp(ud, E);
    float Ef[16];
    for (int k = 0; k < 16; ++k) Ef[k] = (float)E[k];
    mat4_mul_f32(Ef, pose, pose_tmp);
    return 0;
}

void prepare_level(Ctx& ctx, int level) {
    // RPI.h:4538-4549 (idempotent; the reference re-applies it on every call)
    if (ctx.p.mask_seams) {
        maskSeams(ctx.gTrgGx[level]);
        maskSeams(ctx.gTrgGy[level]);
        maskSeams(ctx.dTrgGx[level]);
        maskSeams(ctx.dTrgGy[level]);
    }
    buildLUT(ctx, level);
}

// RPI.h:4519-4784 alignFrames360; occlusion 0 / 1 / 2 selects the error and H,g functions (RPI.h:4597-4603, 4616-4622,
// 4701-4707)
int alignFrames360(Ctx& ctx, const float* pose_guess, int method, float* pose_out, Result* res, int occlusion = 0) {
    auto error_fn = [&](int level, const float* pose) -> double {
        if (occlusion == 1) return errorPhotoICP_sphereOcc1(ctx, level, pose, method, nullptr);
        if (occlusion == 2) return errorPhotoICP_sphereOcc2(ctx, level, pose, method, nullptr);
        return errorPhotoICP_sphere(ctx, level, pose, method);
    };
    auto hessgrad_fn = [&](int level, const float* pose) {
        if (occlusion == 0) calcHessGrad_sphere(ctx, level, pose, method);
        else calcHessGrad_sphereOcc(ctx, level, pose, method, occlusion);
    };
    ctx.trace.clear();
    memset(res, 0, sizeof(*res));
    float pose_estim[16], pose_estim_temp[16];
    memcpy(pose_estim, pose_guess, sizeof(pose_estim));
    double error = 0;
    memset(ctx.H, 0, sizeof(ctx.H));
    memset(ctx.g, 0, sizeof(ctx.g));
    for (int level = ctx.p.n_pyr - 1; level >= 0; --level) {
        prepare_level(ctx, level);
        double lambda = 1.0;  // RPI.h:4589 double lambda = 1e0, lambda /= step in double; converted to float where Eigen scales the matrix
        const double step = 5;
        int it = 0;
        const int maxIters = ctx.p.max_iters;
        const double tol_residual = ctx.p.tol_residual, tol_update = ctx.p.tol_update;
        float update_pose[6] = {1, 1, 1, 1, 1, 1};
        error = error_fn(level, pose_estim);
        if (ctx.last_nvalid == 0 || error != error) {      // no residuals (occlusion modes: NaN from an unused modality)
            memcpy(pose_out, pose_estim, sizeof(pose_estim));
            res->status = 2;
            return 2;
        }
        {
            IterTrace t{};
            t.level = level; t.it = -1; t.accepted = 1; t.error = error; t.new_error = error; t.n_valid = ctx.last_nvalid;
            memcpy(t.pose, pose_estim, sizeof(t.pose));
            ctx.trace.push_back(t);
        }
        double diff_error = error;
        auto unorm = [&]() {
            float s = 0;
            for (int i = 0; i < 6; ++i) s += update_pose[i] * update_pose[i];
            return sqrtf(s);
        };
        while (it < maxIters && unorm() > tol_update && diff_error > tol_residual) {
            hessgrad_fn(level, pose_estim);
            if (gn_step(ctx.H, ctx.g, (float)lambda, pose_estim, pose_estim_temp, update_pose) != 0) {
                memcpy(pose_out, pose_estim, sizeof(pose_estim));  // relPose = pose_estim; avResidual = 0; return
                res->status = 1;
                for (int k = 0; k < 36; ++k) res->hessian[k] = ctx.H[k];
                for (int k = 0; k < 6; ++k) res->gradient[k] = ctx.g[k];
                res->sso = ctx.sso;
                return 1;
            }
            double new_error = error_fn(level, pose_estim_temp);
            diff_error = error - new_error;
            IterTrace t{};
            t.level = level; t.it = it; t.error = error; t.new_error = new_error; t.n_valid = ctx.last_nvalid;
            memcpy(t.pose, pose_estim_temp, sizeof(t.pose));
            memcpy(t.update, update_pose, sizeof(t.update));
            if (diff_error > tol_residual) {
                lambda /= step;
                memcpy(pose_estim, pose_estim_temp, sizeof(pose_estim));
                error = new_error;
                it = it + 1;
                t.accepted = 1;
            }
            ctx.trace.push_back(t);
        }
        res->iters[level] = it;
    }
    memcpy(pose_out, pose_estim, sizeof(pose_estim));
    // The reference never writes avPhotoResidual/avDepthResidual on this path;
    // defined here as the photo / depth RMS of the error pass at the returned pose.
    double e = error_fn(0, pose_estim);
    res->err_final = e;
    res->rms_photo = ctx.last_nvalid_photo ? sqrt(ctx.last_err2_photo / ctx.last_nvalid_photo) : 0.0;
    res->rms_depth = ctx.last_nvalid_depth ? sqrt(ctx.last_err2_depth / ctx.last_nvalid_depth) : 0.0;
    res->sso = ctx.sso;
    for (int k = 0; k < 36; ++k) res->hessian[k] = ctx.H[k];
    for (int k = 0; k < 6; ++k) res->gradient[k] = ctx.g[k];
    res->status = 0;
    return 0;
}

// RPI.h:4254-4512 alignFrames (pinhole, Levenberg-Marquardt damping); occlusion 0 / 1 / 2 selects the error and H,g functions
// (RPI.h:4311-4316, 4335-4340, 4362-4367, 4393-4398).
int alignFrames(Ctx& ctx, const float* pose_guess, int method, float* pose_out, Result* res, int occlusion = 0) {
    ctx.trace.clear();
    memset(res, 0, sizeof(*res));
    float pose_estim[16], pose_estim_temp[16];
    memcpy(pose_estim, pose_guess, sizeof(pose_estim));
    memset(ctx.H, 0, sizeof(ctx.H));
    memset(ctx.g, 0, sizeof(ctx.g));
    double last_eval = 0, last_eval_photo = 0, last_eval_depth = 0;       // avResidual & co as the members hold them
    double avResidual_temp = 0, avPhoto_temp = 0, avDepth_temp = 0;
    bool any_iteration = false;
    double final_error = 0;
    auto eval = [&](int level, const float* pose) {
        double e;
        if (occlusion == 0) {
            e = ctx.use_saliency ? errorPhotoICP_salient(ctx, level, pose, method) : errorPhotoICP(ctx, level, pose, method);
            last_eval_photo = sqrt(ctx.last_err2_photo / ctx.last_nvalid_depth);
            last_eval_depth = sqrt(ctx.last_err2_depth / ctx.last_nvalid_depth);
        } else {
            e = errorPhotoICP_Occ(ctx, level, pose, method, occlusion, nullptr);
            last_eval_photo = sqrt(ctx.last_err2_photo / ctx.last_nvalid_photo);
            last_eval_depth = sqrt(ctx.last_err2_depth / ctx.last_nvalid_depth);
        }
        last_eval = e;
        return e;
    };
    auto hessgrad = [&](int level, const float* pose) {
        if (occlusion == 0) calcHessGrad(ctx, level, pose, method);
        else calcHessGrad_Occ(ctx, level, pose, method, occlusion);
    };
    auto lm_update = [&](float lambda_or_neg, float* update_pose) -> bool {     // lambda < 0: plain -H^-1 g (RPI.h:4355)
        float M[36];
        for (int k = 0; k < 36; ++k) M[k] = ctx.H[k];
        if (lambda_or_neg >= 0)
            for (int i = 0; i < 6; ++i) M[i * 6 + i] = ctx.H[i * 6 + i] + lambda_or_neg * ctx.H[i * 6 + i];
        float inv[36];
        if (!inverse6_partial_piv_lu(M, inv)) return false;
        for (int r = 0; r < 6; ++r) {
            float s = 0.f;
            for (int c = 0; c < 6; ++c) s += (-inv[c * 6 + r]) * ctx.g[c];
            update_pose[r] = s;
        }
        double ud[6], E[16];
        for (int i = 0; i < 6; ++i) ud[i] = (double)update_pose[i];
        se3_exp(ud, E);
        float Ef[16];
        for (int k = 0; k < 16; ++k) Ef[k] = (float)E[k];
        mat4_mul_f32(Ef, pose_estim, pose_estim_temp);
        return true;
    };
    for (int level = ctx.p.n_pyr - 1; level >= 0; --level) {
        buildLUT_pinhole(ctx, level);
        float lambda = 0.01f;            // double lambda = 0.01, used as float scalar by Eigen
        const double step = 10;
        const unsigned LM_maxIters = 1;
        int it = 0;
        const int maxIters = 10;
        const double tol_residual = 1e-4, tol_update = 1e-4;
        float update_pose[6] = {1, 1, 1, 1, 1, 1};
        double error = eval(level, pose_estim), new_error;
        double diff_error = error;
        {
            IterTrace t{};
            t.level = level; t.it = -1; t.accepted = 1; t.error = error; t.new_error = error; t.n_valid = ctx.last_nvalid;
            memcpy(t.pose, pose_estim, sizeof(t.pose));
            ctx.trace.push_back(t);
        }
        auto unorm = [&]() {
            float s = 0;
            for (int i = 0; i < 6; ++i) s += update_pose[i] * update_pose[i];
            return sqrtf(s);
        };
        while (it < maxIters && unorm() > tol_update && diff_error > tol_residual) {
            any_iteration = true;
            avResidual_temp = last_eval; avPhoto_temp = last_eval_photo; avDepth_temp = last_eval_depth;
            hessgrad(level, pose_estim);
            float M[36];
            for (int k = 0; k < 36; ++k) M[k] = ctx.H[k];
            for (int i = 0; i < 6; ++i) M[i * 6 + i] = ctx.H[i * 6 + i] + lambda * ctx.H[i * 6 + i];
            if (rank6_colpiv_qr(M) != 6 || !lm_update(-1.f, update_pose)) {
                memcpy(pose_out, pose_estim, sizeof(pose_estim));      // relPose = pose_estim; return
                res->status = 1;
                for (int k = 0; k < 36; ++k) res->hessian[k] = ctx.H[k];
                for (int k = 0; k < 6; ++k) res->gradient[k] = ctx.g[k];
                return 1;
            }
            new_error = eval(level, pose_estim_temp);
            diff_error = error - new_error;
            IterTrace t{};
            t.level = level; t.it = it; t.error = error; t.new_error = new_error; t.n_valid = ctx.last_nvalid;
            memcpy(t.pose, pose_estim_temp, sizeof(t.pose));
            memcpy(t.update, update_pose, sizeof(t.update));
            if (diff_error > 0) {
                lambda /= step;
                memcpy(pose_estim, pose_estim_temp, sizeof(pose_estim));
                error = new_error;
                it = it + 1;
                t.accepted = 1;
                ctx.trace.push_back(t);
            } else {
                ctx.trace.push_back(t);
                unsigned LM_it = 0;
                while (LM_it < LM_maxIters && diff_error < 0) {
                    lambda = lambda * step;
                    if (!lm_update(lambda, update_pose)) break;        // singular damped system: Eigen would return inf/NaN
                    new_error = eval(level, pose_estim_temp);
                    diff_error = error - new_error;
                    IterTrace t2{};
                    t2.level = level; t2.it = it; t2.error = error; t2.new_error = new_error; t2.n_valid = ctx.last_nvalid;
                    memcpy(t2.pose, pose_estim_temp, sizeof(t2.pose));
                    memcpy(t2.update, update_pose, sizeof(t2.update));
                    if (diff_error > 0) {
                        memcpy(pose_estim, pose_estim_temp, sizeof(pose_estim));
                        error = new_error;
                        it = it + 1;
                        t2.accepted = 1;
                    } else
                        LM_it = LM_it + 1;
                    ctx.trace.push_back(t2);
                }
            }
        }
        res->iters[level] = it;
        final_error = error;
    }
    memcpy(pose_out, pose_estim, sizeof(pose_estim));
    // RPI.h:4507-4509: avResidual = avResidual_temp (the value at the top of the last loop trip; the reference leaves it
    // uninitialised when no trip ran -- defined here as the last evaluated error)
    res->err_final = any_iteration ? avResidual_temp : last_eval;
    res->rms_photo = any_iteration ? avPhoto_temp : last_eval_photo;
    res->rms_depth = any_iteration ? avDepth_temp : last_eval_depth;
    res->sso = (occlusion == 2 && any_iteration) ? ctx.sso : 0.f;      // only calcHessGrad_Occ2 sets SSO on this path (RPI.h:2016)
    for (int k = 0; k < 36; ++k) res->hessian[k] = ctx.H[k];
    for (int k = 0; k < 6; ++k) res->gradient[k] = ctx.g[k];
    res->status = (final_error != final_error) ? 2 : 0;       // NaN error (no depth-valid pixel): nothing was optimised
    return res->status;
}

// ====================================================================================
// 8-sensor rig: RegisterRGBD360::RegisterDensePhotoICP (RegisterRGBD360.h:344-520) over calcPhotoICPError_robot
// (RPI.h:4905-5076) and calcHessianGradient_robot (RPI.h:5083-5407), bUseSalientPixels false (constructor default).
// The unknown is the RIG's relative pose (p_rig1 = T p_rig2); sensor s sees it through its extrinsic Rt_s (sensor -> rig) as
// relPoseCam = Rt_s^-1 T Rt_s.  One RegisterPhotoICP context per sensor (source = frame 2's sensor image, target = frame 1's).
//
// SURVEY.md 8f rank 3 asks for this function "with the reference's bugs fixed"; three defects are fixed, each marked FIX below:
//   A  RegisterRGBD360.h:462, 488 evaluate new_error at pose_estim instead of pose_estim_temp: diff_error is then 0, no step is
//      ever accepted and the function returns its input.                                   -> new_error at pose_estim_temp.
//   B  RPI.h:5226-5228, 5372-5374: jacobianRt_z is declared, `jacobianT36.block(2,0,1,6);` is a statement without effect, and the
//      uninitialised row enters the depth Jacobian.                                         -> jacobianRt_z = jacobianT36.row(2).
//   C  RPI.h:5037-5040, 5213-5216, 5358-5362: the depth residual compares the target depth with the source pixel's ORIGINAL depth
//      instead of the transformed point's (what the single-sensor errorPhotoICP / calcHessGrad, RPI.h:722-735, 935-947, and the
//      Jacobian's -jacobianRt_z term both use): at the true pose a camera that moved along its axis keeps a non-zero residual.
//                                                                                           -> depth1 = transformedPoint3D(2).
// Kept as written: the error is the SUM of squared weighted residuals over the 8 sensors (no averaging, no saliency test), the
// H,g pass applies the saliency `continue`s (a flat depth gradient drops the pixel's photometric row too, RPI.h:5352-5353), LM with
// lambda 0.001, step 10, one retry, tolerances 0.1 (on the sum) / 1e-6, full SE(3) exponential.
// THIRD-PARTY: Eigen's general Matrix4f::inverse() of the extrinsic is restated as the rigid inverse [R^T | -R^T t] in float.
// ====================================================================================
inline void rigid_inverse_f32(const float* M /*col-major*/, float* Inv) {
    for (int k = 0; k < 16; ++k) Inv[k] = 0.f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Inv[j * 4 + i] = M[i * 4 + j];
    for (int i = 0; i < 3; ++i) Inv[12 + i] = -((Inv[0 * 4 + i] * M[12] + Inv[1 * 4 + i] * M[13]) + Inv[2 * 4 + i] * M[14]);
    Inv[15] = 1.f;
}
inline void xform_f32(const float* M /*col-major 4x4*/, const float* p, float* q, bool fma_mode) {
    for (int i = 0; i < 3; ++i)
        q[i] = fma_mode ? fmaf(M[8 + i], p[2], fmaf(M[4 + i], p[1], fmaf(M[i], p[0], M[12 + i])))
                        : ((M[i] * p[0] + M[4 + i] * p[1]) + M[8 + i] * p[2]) + M[12 + i];
}
struct RobotWarp {
    float q[3];       // point in the rig frame after the motion: poseGuess * Rt * p   (point3D_robot2)
    float P[3];       // the same point in the target sensor's frame                    (transformedPoint3D)
    float inv_z;
    int r, c;
    bool visible;
};
// which = 0: the chain of calcPhotoICPError_robot (relPoseCam * p, double projection); 1: that of calcHessianGradient_robot
// (Rt^-1 * (poseGuess * (Rt * p)), double intrinsics).  math_mode 1 = the device definition, one chain for both passes:
// q = (poseGuess * Rt) p and P = Rt^-1 q with fused multiply-adds, correctly rounded 1/Z, fma projection, round half up.
inline RobotWarp warp_robot(const float* poseGuess, const float* Rt, const float* Rt_inv, const float* p, int nRows, int nCols,
                            const PinholeK& K, int math_mode, int which) {
    RobotWarp w;
    float tr, tc;
    if (math_mode == 0) {
        float pr[3];
        xform_f32(Rt, p, pr, false);
        xform_f32(poseGuess, pr, w.q, false);
        if (which == 0) {
            float A[16], C[16];
            mat4_mul_f32(Rt_inv, poseGuess, A);
            mat4_mul_f32(A, Rt, C);                       // relPoseCam = poseCamRobot_inv * poseGuess * poseCamRobot
            xform_f32(C, p, w.P, false);
        } else {
            xform_f32(Rt_inv, w.q, w.P, false);
        }
        const double inv_transformedPz = 1.0 / w.P[2];
        w.inv_z = (float)inv_transformedPz;
        const double dc = which == 0 ? (double)(w.P[0] * K.fx) * inv_transformedPz + (double)K.ox
                                     : ((double)w.P[0] * (double)K.fx) * inv_transformedPz + (double)K.ox;
        const double dr = which == 0 ? (double)(w.P[1] * K.fy) * inv_transformedPz + (double)K.oy
                                     : ((double)w.P[1] * (double)K.fy) * inv_transformedPz + (double)K.oy;
        if (!std::isfinite(dr) || !std::isfinite(dc) || fabs(dr) > 1e9 || fabs(dc) > 1e9) { w.visible = false; w.r = w.c = -1; return w; }
        w.r = (int)round(dr);
        w.c = (int)round(dc);
    } else {
        float M[16];
        mat4_mul_f32(poseGuess, Rt, M);
        xform_f32(M, p, w.q, true);
        xform_f32(Rt_inv, w.q, w.P, true);
        w.inv_z = 1.f / w.P[2];
        tc = fmaf(w.P[0] * K.fx, w.inv_z, K.ox);
        tr = fmaf(w.P[1] * K.fy, w.inv_z, K.oy);
        if (!(fabsf(tr) < 1e9f) || !(fabsf(tc) < 1e9f)) { w.visible = false; w.r = w.c = -1; return w; }
        w.r = round_index(tr);
        w.c = round_index(tc);
    }
    w.visible = (w.r >= 0 && w.r < nRows) && (w.c >= 0 && w.c < nCols);
    return w;
}

// RPI.h:4905-5076, else-branch :4990-5072.  Returns error2 (the sum); the per-modality sums and counts go to ctx.last_*.
// bUseSalientPixels on this path (RPI.h:4930-5003, 5121-5262): the same loop bodies over vSalientPixels -- membership of pixel i
// in the list calcGradientXY_saliency builds from the TARGET's gray gradients (RPI.h:420-424; border gradients are zero).
inline bool in_salient_list(const Ctx& ctx, int level, long i) {
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level];
    const int r = (int)(i / gx.cols), c = (int)(i % gx.cols);
    if (r < 1 || r >= gx.rows - 1 || c < 1 || c >= gx.cols - 1) return false;
    return fabsf(gx.d[i]) > ctx.thres_saliency || fabsf(gy.d[i]) > ctx.thres_saliency;
}

double calcPhotoICPError_robot(Ctx& ctx, int level, const float* poseGuess, const float* Rt, int method) {
    double e2p = 0.0, e2d = 0.0;
    long nP = 0, nD = 0;
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const PinholeK K = level_intrinsics(ctx, level);
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const double stdDevPhoto_inv = 1. / stdDevPhoto;
    float Rt_inv[16];
    rigid_inverse_f32(Rt, Rt_inv);
    if (ctx.lut_level != 1000 + level) buildLUT_pinhole(ctx, level);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const long n = (long)nRows * nCols;
    // (serial: the sensor images are small, and a 256-thread OpenMP team per sensor and evaluation costs more than the loop)
    for (long i = 0; i < n; ++i) {
        if (ctx.use_saliency && !in_salient_list(ctx, level, i)) continue;
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        const RobotWarp w = warp_robot(poseGuess, Rt, Rt_inv, p, nRows, nCols, K, ctx.p.math_mode, 0);
        if (!w.visible) continue;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            double weight_photo = weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv;
            float weightedErrorPhoto = weight_photo * photoDiff;
            e2p += weightedErrorPhoto * weightedErrorPhoto;
            ++nP;
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            float depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                float depth1 = w.P[2];                                   // FIX C (reference: depthSrcPyr(r, c))
                float depthDiff = depth2 - depth1;
                float stdDev_depth1 = stdDevDepth * depth1;
                double weight_depth = weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1;
                float weightedErrorDepth = weight_depth * depthDiff;
                e2d += weightedErrorDepth * weightedErrorDepth;
                ++nD;
            }
        }
    }
    ctx.last_err2_photo = e2p; ctx.last_err2_depth = e2d;
    ctx.last_nvalid_photo = nP; ctx.last_nvalid_depth = nD;
    ctx.last_nvalid = nP + nD;
    return e2p + e2d;
}

// RPI.h:5083-5407, else-branch :5264-5404.  H, g in the rig's left-perturbation coordinates [t; w].
void calcHessianGradient_robot(Ctx& ctx, int level, const float* poseGuess, const float* Rt, int method) {
    const Image& graySrc = ctx.graySrc[level];
    const int nRows = graySrc.rows, nCols = graySrc.cols;
    const long imgSize = (long)nRows * nCols;
    const PinholeK K = level_intrinsics(ctx, level);
    const float stdDevPhoto = ctx.p.sigma_photo, stdDevDepth = ctx.p.sigma_depth;
    const double stdDevPhoto_inv = 1. / stdDevPhoto;
    float Rt_inv[16];
    rigid_inverse_f32(Rt, Rt_inv);
    if (ctx.lut_level != 1000 + level) buildLUT_pinhole(ctx, level);
    const Image &grayTrg = ctx.grayTrg[level], &depthTrg = ctx.depthTrg[level];
    const Image &gx = ctx.gTrgGx[level], &gy = ctx.gTrgGy[level], &dgx = ctx.dTrgGx[level], &dgy = ctx.dTrgGy[level];
    const float thrI = ctx.p.thres_sal_photo, thrD = ctx.p.thres_sal_depth;
    float Hf[36] = {0}, gf[6] = {0};
    double Hd[36] = {0}, gd[6] = {0};
    long rows_used = 0;
    auto add_row = [&](const float* J, float res) {
        for (int a = 0; a < 6; ++a) {
            for (int b = 0; b < 6; ++b) {
                const float prod = J[a] * J[b];
                Hf[b * 6 + a] += prod;
                Hd[b * 6 + a] += (double)prod;
            }
            const float pr = J[a] * res;
            gf[a] += pr;
            gd[a] += (double)pr;
        }
        ++rows_used;
    };
    for (long i = 0; i < imgSize; ++i) {
        if (ctx.use_saliency && !in_salient_list(ctx, level, i)) continue;
        const float* p = &ctx.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        const RobotWarp w = warp_robot(poseGuess, Rt, Rt_inv, p, nRows, nCols, K, ctx.p.math_mode, 1);
        if (!w.visible) continue;
        // jacobianT36 = R_inv [I | -skew(point3D_robot2)]   (RPI.h:5298-5302)
        const float* q = w.q;
        const float S[3][3] = {{0, -q[2], q[1]}, {q[2], 0, -q[0]}, {-q[1], q[0], 0}};      // skew(q)
        float JT[3][6];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                JT[r][c] = Rt_inv[c * 4 + r];                                                  // R_inv * I
                JT[r][3 + c] = (Rt_inv[0 * 4 + r] * (-S[0][c]) + Rt_inv[1 * 4 + r] * (-S[1][c])) + Rt_inv[2 * 4 + r] * (-S[2][c]);
            }
        // jacobianProj23 (RPI.h:5304-5313)
        const float iz = w.inv_z;
        const float P00 = K.fx * iz, P11 = K.fy * iz, P02 = -K.fx * w.P[0] * iz * iz, P12 = -K.fy * w.P[1] * iz * iz;
        float Jw0[6], Jw1[6];
        for (int c = 0; c < 6; ++c) {
            Jw0[c] = P00 * JT[0][c] + P02 * JT[2][c];
            Jw1[c] = P11 * JT[1][c] + P12 * JT[2][c];
        }
        float jacobianPhoto[6] = {0, 0, 0, 0, 0, 0}, jacobianDepth[6] = {0, 0, 0, 0, 0, 0};
        float weightedErrorPhoto = 0.f, weightedErrorDepth = 0.f;
        bool have_depth_row = false;
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) {
            const float tgx = gx.at(w.r, w.c), tgy = gy.at(w.r, w.c);
            if (fabsf(tgx) < thrI && fabsf(tgy) < thrI) continue;                              // RPI.h:5331-5332
            float photoDiff = grayTrg.at(w.r, w.c) - graySrc.d[i];
            const float weight_photo = (float)(weightHuber(photoDiff, stdDevPhoto) * stdDevPhoto_inv);
            weightedErrorPhoto = weight_photo * photoDiff;
            const float wgx = weight_photo * tgx, wgy = weight_photo * tgy;
            for (int j = 0; j < 6; ++j) jacobianPhoto[j] = wgx * Jw0[j] + wgy * Jw1[j];
        }
        if (method == METHOD_DEPTH || method == METHOD_PHOTO_DEPTH) {
            const float depth2 = depthTrg.at(w.r, w.c);
            if (std::isfinite(depth2)) {
                const float tdx = dgx.at(w.r, w.c), tdy = dgy.at(w.r, w.c);
                if (fabsf(tdx) < thrD && fabsf(tdy) < thrD) continue;                          // RPI.h:5352-5353: drops the photo row too
                const float depth1 = w.P[2];                                                   // FIX C
                float depthDiff = depth2 - depth1;
                float stdDev_depth1 = stdDevDepth * depth1;
                const float weight_depth = (float)((double)weightHuber(depthDiff, stdDev_depth1) / stdDev_depth1);
                weightedErrorDepth = weight_depth * depthDiff;
                for (int j = 0; j < 6; ++j) jacobianDepth[j] = weight_depth * ((tdx * Jw0[j] + tdy * Jw1[j]) - JT[2][j]);      // FIX B
                have_depth_row = true;
            }
        }
        if (method == METHOD_PHOTO || method == METHOD_PHOTO_DEPTH) add_row(jacobianPhoto, weightedErrorPhoto);
        if (have_depth_row) add_row(jacobianDepth, weightedErrorDepth);
    }
    for (int k = 0; k < 36; ++k) {
        ctx.H[k] = ctx.p.reduce_mode == 0 ? Hf[k] : (float)Hd[k];
        ctx.H64[k] = Hd[k];
    }
    for (int a = 0; a < 6; ++a) {
        ctx.g[a] = ctx.p.reduce_mode == 0 ? gf[a] : (float)gd[a];
        ctx.g64[a] = gd[a];
    }
    ctx.n_visible = rows_used;
}

struct RigTrace {
    int level, it, accepted;
    double error, new_error;
};
struct Rig {
    std::vector<Ctx*> sensors;
    std::vector<float> Rt;          // n x 16, col-major, sensor -> rig
    std::vector<RigTrace> trace;
};
// RegisterRGBD360.h:383-500.  Returns 0 ok / 1 ill-posed (rigidTransf = pose_estim, return false).
int RegisterDensePhotoICP(Rig& rig, const float* pose_guess, int method, float* pose_out, float* H_out /*36*/, int* iters /*8*/) {
    const int S = (int)rig.sensors.size();
    rig.trace.clear();
    float pose_estim[16], pose_estim_temp[16];
    memcpy(pose_estim, pose_guess, sizeof(pose_estim));
    float Hessian[36] = {0}, Gradient[6] = {0};
    for (int k = 0; k < 8; ++k) iters[k] = 0;
    auto total_error = [&](int level, const float* pose) {
        double e = 0.0;
        for (int s = 0; s < S; ++s) e += calcPhotoICPError_robot(*rig.sensors[s], level, pose, &rig.Rt[16 * s], method);
        return e;
    };
    auto lm_update = [&](float lambda, float* update_pose) -> bool {
        float M[36];
        for (int k = 0; k < 36; ++k) M[k] = Hessian[k];
        for (int i = 0; i < 6; ++i) M[i * 6 + i] = Hessian[i * 6 + i] + lambda * Hessian[i * 6 + i];
        float inv[36];
        if (!inverse6_partial_piv_lu(M, inv)) return false;
        for (int r = 0; r < 6; ++r) {
            float sacc = 0.f;
            for (int c = 0; c < 6; ++c) sacc += (-inv[c * 6 + r]) * Gradient[c];
            update_pose[r] = sacc;
        }
        double ud[6], E[16];
        for (int i = 0; i < 6; ++i) ud[i] = (double)update_pose[i];
        se3_exp(ud, E);
        float Ef[16];
        for (int k = 0; k < 16; ++k) Ef[k] = (float)E[k];
        mat4_mul_f32(Ef, pose_estim, pose_estim_temp);
        return true;
    };
    const int n_pyr = rig.sensors[0]->p.n_pyr;
    for (int level = n_pyr - 1; level >= 0; --level) {
        float lambda = 0.001f;
        const double step = 10;
        const unsigned LM_maxIters = 1;
        int it = 0;
        const int maxIters = 10;
        const double tol_residual = pow(10, -1), tol_update = pow(10, -6);
        float update_pose[6] = {1, 1, 1, 1, 1, 1};
        double error = total_error(level, pose_estim);
        double diff_error = error;
        rig.trace.push_back({level, -1, 1, error, error});
        auto unorm = [&]() {
            float sacc = 0;
            for (int i = 0; i < 6; ++i) sacc += update_pose[i] * update_pose[i];
            return sqrtf(sacc);
        };
        while (it < maxIters && unorm() > tol_update && diff_error > tol_residual) {
            for (int k = 0; k < 36; ++k) Hessian[k] = 0.f;
            for (int k = 0; k < 6; ++k) Gradient[k] = 0.f;
            for (int s = 0; s < S; ++s) {
                Ctx& c = *rig.sensors[s];
                calcHessianGradient_robot(c, level, pose_estim, &rig.Rt[16 * s], method);
                for (int k = 0; k < 36; ++k) Hessian[k] += c.H[k];
                for (int k = 0; k < 6; ++k) Gradient[k] += c.g[k];
            }
            float M[36];
            for (int k = 0; k < 36; ++k) M[k] = Hessian[k];
            for (int i = 0; i < 6; ++i) M[i * 6 + i] = Hessian[i * 6 + i] + lambda * Hessian[i * 6 + i];
            if (rank6_colpiv_qr(M) != 6 || !lm_update(lambda, update_pose)) {
                memcpy(pose_out, pose_estim, sizeof(pose_estim));
                memcpy(H_out, Hessian, sizeof(Hessian));
                return 1;
            }
            double new_error = total_error(level, pose_estim_temp);                            // FIX A (reference: pose_estim)
            diff_error = error - new_error;
            if (diff_error > 0) {
                rig.trace.push_back({level, it, 1, error, new_error});
                lambda /= step;
                memcpy(pose_estim, pose_estim_temp, sizeof(pose_estim));
                error = new_error;
                it = it + 1;
            } else {
                rig.trace.push_back({level, it, 0, error, new_error});
                unsigned LM_it = 0;
                while (LM_it < LM_maxIters && diff_error < 0) {
                    lambda = lambda * step;
                    if (!lm_update(lambda, update_pose)) break;
                    new_error = total_error(level, pose_estim_temp);                           // FIX A
                    diff_error = error - new_error;
                    if (diff_error > 0) {
                        rig.trace.push_back({level, it, 1, error, new_error});
                        memcpy(pose_estim, pose_estim_temp, sizeof(pose_estim));
                        error = new_error;
                        it = it + 1;
                    } else {
                        rig.trace.push_back({level, it, 0, error, new_error});
                    }
                    LM_it = LM_it + 1;
                }
            }
        }
        iters[level] = it;
    }
    memcpy(pose_out, pose_estim, sizeof(pose_estim));
    memcpy(H_out, Hessian, sizeof(Hessian));
    return 0;
}

void set_frame(Ctx& ctx, bool target, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t d_step,
               int depth_type, int rows, int cols) {
    Image gray;
    rgb_to_gray_f32(rgb, rgb_step, rows, cols, gray);
    if (target) {  // RPI.h:498-516
        buildPyramid(gray, ctx.grayTrg, ctx.p.n_pyr);
        buildPyramidRange(depth, d_step, depth_type, rows, cols, ctx.p, ctx.depthTrg);
        // RPI.h:429-477 buildGradientPyramids
        ctx.gTrgGx.resize(ctx.p.n_pyr); ctx.gTrgGy.resize(ctx.p.n_pyr);
        ctx.dTrgGx.resize(ctx.p.n_pyr); ctx.dTrgGy.resize(ctx.p.n_pyr);
        for (int l = 0; l < ctx.p.n_pyr; ++l) {
            calcGradientXY(ctx.grayTrg[l], ctx.gTrgGx[l], ctx.gTrgGy[l]);
            calcGradientXY(ctx.depthTrg[l], ctx.dTrgGx[l], ctx.dTrgGy[l]);
        }
    } else {  // RPI.h:480-494 (the colour pyramid is visualisation-only and omitted)
        buildPyramid(gray, ctx.graySrc, ctx.p.n_pyr);
        buildPyramidRange(depth, d_step, depth_type, rows, cols, ctx.p, ctx.depthSrc);
    }
    ctx.lut_level = -1;
}

}  // namespace

// ======================================================================================
// C interface for the Python harness (ctypes)
// ======================================================================================
extern "C" {

typedef Params oracle_params;
typedef Result oracle_result;
typedef IterTrace oracle_trace;

void oracle_default_params(oracle_params* p) {
    p->n_pyr = 4;
    p->min_depth = 0.3f;
    p->max_depth = 6.0f;
    p->sigma_photo = (float)(6. / 255);
    p->sigma_depth = (float)0.2;
    p->thres_sal_photo = 0.01f;
    p->thres_sal_depth = 0.01f;
    p->max_iters = 10;
    p->tol_residual = 1e-3f;
    p->tol_update = 1e-4f;
    p->mask_seams = 1;
    p->math_mode = 0;
    p->reduce_mode = 0;
}

void* oracle_create(const oracle_params* p) {
    Ctx* c = new Ctx();
    c->p = *p;
    return c;
}
void oracle_destroy(void* h) { delete (Ctx*)h; }
void oracle_set_modes(void* h, int math_mode, int reduce_mode) {
    ((Ctx*)h)->p.math_mode = math_mode;
    ((Ctx*)h)->p.reduce_mode = reduce_mode;
}

void oracle_set_target(void* h, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t d_step, int depth_type,
                       int rows, int cols) {
    set_frame(*(Ctx*)h, true, rgb, rgb_step, depth, d_step, depth_type, rows, cols);
}
void oracle_set_source(void* h, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t d_step, int depth_type,
                       int rows, int cols) {
    set_frame(*(Ctx*)h, false, rgb, rgb_step, depth, d_step, depth_type, rows, cols);
}

int oracle_align360(void* h, const float* guess, int method, float* pose_out, oracle_result* res) {
    return alignFrames360(*(Ctx*)h, guess, method, pose_out, res);
}

int oracle_align360_occ(void* h, const float* guess, int method, int occlusion, float* pose_out, oracle_result* res) {
    return alignFrames360(*(Ctx*)h, guess, method, pose_out, res, occlusion);
}
// Occlusion-mode error pass: sums[4] = {sum photo, sum depth, n photo, n depth}; returns avPhoto + avDepth.
double oracle_error_occ(void* h, int level, const float* pose, int method, int occlusion, double* sums) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != level) prepare_level(c, level);
    OccSums o;
    double e = occlusion == 1 ? errorPhotoICP_sphereOcc1(c, level, pose, method, &o) : errorPhotoICP_sphereOcc2(c, level, pose, method, &o);
    if (sums) { sums[0] = o.photo; sums[1] = o.depth; sums[2] = (double)o.nPhoto; sums[3] = (double)o.nDepth; }
    return e;
}
void oracle_hessgrad_occ(void* h, int level, const float* pose, int method, int occlusion, float* H36, float* g6, double* H36d,
                         double* g6d, long* n_visible) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != level) prepare_level(c, level);
    calcHessGrad_sphereOcc(c, level, pose, method, occlusion);
    if (H36) memcpy(H36, c.H, sizeof(c.H));
    if (g6) memcpy(g6, c.g, sizeof(c.g));
    if (H36d) memcpy(H36d, c.H64, sizeof(c.H64));
    if (g6d) memcpy(g6d, c.g64, sizeof(c.g64));
    if (n_visible) *n_visible = c.n_visible;
}

// ---- pinhole single-sensor path ----
void oracle_set_camera(void* h, float fx, float fy, float ox, float oy) {
    Ctx& c = *(Ctx*)h;
    c.cam[0] = fx; c.cam[1] = fy; c.cam[2] = ox; c.cam[3] = oy;
    c.have_cam = true;
}
int oracle_align_pinhole(void* h, const float* guess, int method, float* pose_out, oracle_result* res) {
    return alignFrames(*(Ctx*)h, guess, method, pose_out, res);
}
int oracle_align_pinhole_occ(void* h, const float* guess, int method, int occlusion, float* pose_out, oracle_result* res) {
    return alignFrames(*(Ctx*)h, guess, method, pose_out, res, occlusion);
}
// useSaliency(bool) RPI.h:266-269 (+ thresSaliency RPI.h:217)
void oracle_use_saliency(void* h, int on, float thres_saliency) {
    Ctx& c = *(Ctx*)h;
    c.use_saliency = on != 0;
    c.thres_saliency = thres_saliency;
}
// vSalientPixels of a level (out may be null: returns the count)
int oracle_salient_pixels(void* h, int level, int* out) {
    Ctx& c = *(Ctx*)h;
    buildSalientPixels(c, level);
    if (out) memcpy(out, c.salient[level].data(), c.salient[level].size() * sizeof(int));
    return (int)c.salient[level].size();
}
double oracle_error_pinhole_salient(void* h, int level, const float* pose, int method, double* sums) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != 1000 + level) buildLUT_pinhole(c, level);
    const double e = errorPhotoICP_salient(c, level, pose, method);
    if (sums) { sums[0] = c.last_err2_photo; sums[1] = c.last_err2_depth; sums[2] = (double)c.last_nvalid_photo; sums[3] = (double)c.last_nvalid_depth; }
    return e;
}
// sums[4] = {sum photo, sum depth, n photo, n depth}; returns avPhoto + avDepth
double oracle_error_pinhole_occ(void* h, int level, const float* pose, int method, int occlusion, double* sums) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != 1000 + level) buildLUT_pinhole(c, level);
    OccSums o;
    const double e = errorPhotoICP_Occ(c, level, pose, method, occlusion, &o);
    if (sums) { sums[0] = o.photo; sums[1] = o.depth; sums[2] = (double)o.nPhoto; sums[3] = (double)o.nDepth; }
    return e;
}
void oracle_hessgrad_pinhole_occ(void* h, int level, const float* pose, int method, int occlusion, float* H36, float* g6, double* H36d,
                                 double* g6d, long* n_visible) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != 1000 + level) buildLUT_pinhole(c, level);
    calcHessGrad_Occ(c, level, pose, method, occlusion);
    if (H36) memcpy(H36, c.H, sizeof(c.H));
    if (g6) memcpy(g6, c.g, sizeof(c.g));
    if (H36d) memcpy(H36d, c.H64, sizeof(c.H64));
    if (g6d) memcpy(g6d, c.g64, sizeof(c.g64));
    if (n_visible) *n_visible = c.n_visible;
}
// sums[4] = {sum photo, sum depth, n photo, n depth}; returns avPhoto + avDepth (both / n depth)
double oracle_error_pinhole(void* h, int level, const float* pose, int method, double* sums) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != 1000 + level) buildLUT_pinhole(c, level);
    const double e = errorPhotoICP(c, level, pose, method);
    if (sums) { sums[0] = c.last_err2_photo; sums[1] = c.last_err2_depth; sums[2] = (double)c.last_nvalid_photo; sums[3] = (double)c.last_nvalid_depth; }
    return e;
}
void oracle_hessgrad_pinhole(void* h, int level, const float* pose, int method, float* H36, float* g6, double* H36d, double* g6d,
                             long* n_rows) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != 1000 + level) buildLUT_pinhole(c, level);
    calcHessGrad(c, level, pose, method);
    if (H36) memcpy(H36, c.H, sizeof(c.H));
    if (g6) memcpy(g6, c.g, sizeof(c.g));
    if (H36d) memcpy(H36d, c.H64, sizeof(c.H64));
    if (g6d) memcpy(g6d, c.g64, sizeof(c.g64));
    if (n_rows) *n_rows = c.n_visible;
}
int oracle_get_lut_pinhole(void* h, int level, float* out_xyz) {
    Ctx& c = *(Ctx*)h;
    buildLUT_pinhole(c, level);
    memcpy(out_xyz, c.lut.data(), c.lut.size() * sizeof(float));
    return (int)(c.lut.size() / 3);
}
void oracle_se3_exp(const double* v, double* M) { se3_exp(v, M); }
// Per-pixel pinhole warp indices of a level: out_rc[2*i] = r', [2*i+1] = c', -1 if skipped.
void oracle_warp_indices_pinhole(void* h, int level, const float* pose, int* out_rc) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != 1000 + level) buildLUT_pinhole(c, level);
    const int nRows = c.graySrc[level].rows, nCols = c.graySrc[level].cols;
    const PinholeK K = level_intrinsics(c, level);
    const PoseRT T = split_pose(pose);
    for (long i = 0; i < (long)nRows * nCols; ++i) {
        out_rc[2 * i] = out_rc[2 * i + 1] = -1;
        const float* p = &c.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        const WarpPin w = warp_pinhole(T, p, nRows, nCols, K, c.p.math_mode);
        if (w.visible) { out_rc[2 * i] = w.r; out_rc[2 * i + 1] = w.c; }
    }
}

// ---- 8-sensor rig (RegisterDensePhotoICP with the reference's defects fixed, see above) ----
void* oracle_rig_create(const oracle_params* p, int n_sensors, const float* Rt /*n x 16 col-major*/, float fx, float fy, float ox, float oy) {
    Rig* r = new Rig();
    for (int s = 0; s < n_sensors; ++s) {
        Ctx* c = new Ctx();
        c->p = *p;
        c->cam[0] = fx; c->cam[1] = fy; c->cam[2] = ox; c->cam[3] = oy;
        r->sensors.push_back(c);
    }
    r->Rt.assign(Rt, Rt + 16 * (size_t)n_sensors);
    return r;
}
void oracle_rig_destroy(void* h) {
    Rig* r = (Rig*)h;
    if (!r) return;
    for (Ctx* c : r->sensors) delete c;
    delete r;
}
void oracle_rig_set_modes(void* h, int math_mode, int reduce_mode) {
    for (Ctx* c : ((Rig*)h)->sensors) { c->p.math_mode = math_mode; c->p.reduce_mode = reduce_mode; }
}
void oracle_rig_use_saliency(void* h, int on, float thres_saliency) {
    for (Ctx* c : ((Rig*)h)->sensors) { c->use_saliency = on != 0; c->thres_saliency = thres_saliency; }
}
void oracle_rig_set_frame(void* h, int sensor, int target, const uint8_t* rgb, size_t rgb_step, const void* depth, size_t d_step,
                          int depth_type, int rows, int cols) {
    set_frame(*((Rig*)h)->sensors[sensor], target != 0, rgb, rgb_step, depth, d_step, depth_type, rows, cols);
}
// error2 of one evaluation at `pose` summed over the sensors; sums[0..1] = photo / depth parts, sums[2..3] = their pixel counts
double oracle_rig_error(void* h, int level, const float* pose, int method, double* sums) {
    Rig& r = *(Rig*)h;
    double e = 0, s4[4] = {0, 0, 0, 0};
    for (size_t s = 0; s < r.sensors.size(); ++s) {
        Ctx& c = *r.sensors[s];
        e += calcPhotoICPError_robot(c, level, pose, &r.Rt[16 * s], method);
        s4[0] += c.last_err2_photo; s4[1] += c.last_err2_depth; s4[2] += (double)c.last_nvalid_photo; s4[3] += (double)c.last_nvalid_depth;
    }
    if (sums) memcpy(sums, s4, sizeof(s4));
    return e;
}
void oracle_rig_hessgrad(void* h, int level, const float* pose, int method, float* H36, float* g6, double* H36d, double* g6d, long* rows_used) {
    Rig& r = *(Rig*)h;
    float H[36] = {0}, g[6] = {0};
    double Hd[36] = {0}, gd[6] = {0};
    long n = 0;
    for (size_t s = 0; s < r.sensors.size(); ++s) {
        Ctx& c = *r.sensors[s];
        calcHessianGradient_robot(c, level, pose, &r.Rt[16 * s], method);
        for (int k = 0; k < 36; ++k) { H[k] += c.H[k]; Hd[k] += c.H64[k]; }
        for (int k = 0; k < 6; ++k) { g[k] += c.g[k]; gd[k] += c.g64[k]; }
        n += c.n_visible;
    }
    if (H36) memcpy(H36, H, sizeof(H));
    if (g6) memcpy(g6, g, sizeof(g));
    if (H36d) memcpy(H36d, Hd, sizeof(Hd));
    if (g6d) memcpy(g6d, gd, sizeof(gd));
    if (rows_used) *rows_used = n;
}
int oracle_rig_align(void* h, const float* guess, int method, float* pose_out, float* H36, int* iters8) {
    return RegisterDensePhotoICP(*(Rig*)h, guess, method, pose_out, H36, iters8);
}
int oracle_rig_trace_len(void* h) { return (int)((Rig*)h)->trace.size(); }
void oracle_rig_trace_get(void* h, int i, int* level, int* it, int* accepted, double* error, double* new_error) {
    const RigTrace& t = ((Rig*)h)->trace[i];
    *level = t.level; *it = t.it; *accepted = t.accepted; *error = t.error; *new_error = t.new_error;
}

int oracle_trace_len(void* h) { return (int)((Ctx*)h)->trace.size(); }
void oracle_trace_get(void* h, int i, oracle_trace* out) { *out = ((Ctx*)h)->trace[i]; }

// which: 0 graySrc 1 grayTrg 2 depthSrc 3 depthTrg 4 gx 5 gy 6 dgx 7 dgy
int oracle_level_dims(void* h, int level, int* rows, int* cols) {
    Ctx& c = *(Ctx*)h;
    if (level < 0 || level >= (int)c.grayTrg.size()) return -1;
    *rows = c.grayTrg[level].rows;
    *cols = c.grayTrg[level].cols;
    return 0;
}
int oracle_get_plane(void* h, int which, int level, float* out) {
    Ctx& c = *(Ctx*)h;
    std::vector<Image>* v[8] = {&c.graySrc, &c.grayTrg, &c.depthSrc, &c.depthTrg, &c.gTrgGx, &c.gTrgGy, &c.dTrgGx, &c.dTrgGy};
    if (which < 0 || which > 7 || level < 0 || level >= (int)v[which]->size()) return -1;
    const Image& im = (*v[which])[level];
    memcpy(out, im.d.data(), im.d.size() * sizeof(float));
    return 0;
}
// Applies the seam mask and builds the LUT of `level` (what alignFrames360 does on entering a level).
void oracle_prepare_level(void* h, int level) { prepare_level(*(Ctx*)h, level); }
int oracle_get_lut(void* h, float* out_xyz) {
    Ctx& c = *(Ctx*)h;
    memcpy(out_xyz, c.lut.data(), c.lut.size() * sizeof(float));
    return (int)(c.lut.size() / 3);
}
// Error pass at `pose` on a prepared level. Returns rms; outputs raw sums.
double oracle_error(void* h, int level, const float* pose, int method, double* err2, long* n_valid) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != level) prepare_level(c, level);
    double e = errorPhotoICP_sphere(c, level, pose, method);
    if (err2) *err2 = c.last_err2;
    if (n_valid) *n_valid = c.last_nvalid;
    return e;
}
// H,g pass at `pose` on a prepared level.
void oracle_hessgrad(void* h, int level, const float* pose, int method, float* H36, float* g6, double* H36d, double* g6d,
                     long* n_visible) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != level) prepare_level(c, level);
    calcHessGrad_sphere(c, level, pose, method);
    if (H36) memcpy(H36, c.H, sizeof(c.H));
    if (g6) memcpy(g6, c.g, sizeof(c.g));
    if (H36d) memcpy(H36d, c.H64, sizeof(c.H64));
    if (g6d) memcpy(g6d, c.g64, sizeof(c.g64));
    if (n_visible) *n_visible = c.n_visible;
}
// One GN step from given H,g: returns 0 / 1 (ill-posed).
int oracle_gn_step(const float* H36, const float* g6, float lambda, const float* pose, float* pose_tmp, float* update6) {
    return gn_step(H36, g6, lambda, pose, pose_tmp, update6);
}
// Forced schedule used for the CPU baseline timing: n_iters x { H,g pass; solve; error pass },
// step applied regardless of the accept rule.  Returns the last error.
double oracle_forced_iters(void* h, int level, const float* pose0, int method, int n_iters, float* pose_out) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != level) prepare_level(c, level);
    float pose[16], tmp[16], upd[6];
    memcpy(pose, pose0, sizeof(pose));
    double e = 0;
    for (int k = 0; k < n_iters; ++k) {
        calcHessGrad_sphere(c, level, pose, method);
        if (gn_step(c.H, c.g, 1.f, pose, tmp, upd) != 0) break;
        e = errorPhotoICP_sphere(c, level, tmp, method);
        memcpy(pose, tmp, sizeof(pose));
    }
    if (pose_out) memcpy(pose_out, pose, sizeof(pose));
    return e;
}
// Per-pixel warp indices for a prepared level (index parity checks): out_rc[2*i] = r', [2*i+1] = c', -1 if skipped.
void oracle_warp_indices(void* h, int level, const float* pose, int* out_rc) {
    Ctx& c = *(Ctx*)h;
    if (c.lut_level != level) prepare_level(c, level);
    const int nRows = c.graySrc[level].rows, nCols = c.graySrc[level].cols;
    const float angle_res = 2 * kPI / nCols;
    const float angle_res_inv = 1 / angle_res;
    const float half_nRows = 0.5 * nRows - 0.5;
    PoseRT T = split_pose(pose);
    const long n = (long)nRows * nCols;
#pragma omp parallel for
    for (long i = 0; i < n; ++i) {
        out_rc[2 * i] = out_rc[2 * i + 1] = -1;
        const float* p = &c.lut[3 * i];
        if (p[0] == kInvalidPoint) continue;
        Warp w = warp_pixel(T, p, nRows, nCols, half_nRows, angle_res_inv, c.p.math_mode);
        if (!w.visible) continue;
        out_rc[2 * i] = w.r;
        out_rc[2 * i + 1] = w.c;
    }
}
// ------------------------------------------------------------------------------------
// Frame360 sphere clouds.  xyz out: rows*cols x 3, NaN where the reference writes NaN.
//   convention 0: Frame360::buildSphereCloud_fromImage        Frame360.h:555-612   (u16 mm, phi offset 31.5 deg)
//   convention 1: Frame360_stereo::buildSphereCloud           Frame360_stereo.h:454-512 (f32 m, valid in (0,15))
//   convention 2: the RegisterPhotoICP LUT convention          RPI.h:4556-4582 without the depth band
// ------------------------------------------------------------------------------------
void oracle_sphere_cloud(const void* depth, size_t step, int depth_type, int rows, int cols, int convention, float* xyz) {
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    for (int r = 0; r < rows; ++r) {
        const uint8_t* row = (const uint8_t*)depth + (size_t)r * step;
        for (int c = 0; c < cols; ++c) {
            float* o = xyz + 3 * ((size_t)r * cols + c);
            o[0] = o[1] = o[2] = qnan;
            if (convention == 0) {
                const float angle_pixel(cols / (2 * kPI));
                const float angle_pixel_inv(1 / angle_pixel);
                const float offset_phi = kPI * 31.5 / 180;
                const float phi_i = offset_phi - r * angle_pixel_inv;
                const float sin_phi = sinf(phi_i), cos_phi = cosf(phi_i);   // float arguments -> float overloads (SURVEY.md 3.4 gotcha 2)
                const float theta_i = c * angle_pixel_inv;
                const float d = 0.001f * ((const uint16_t*)row)[c];
                if (d != 0) {
                    o[0] = sin_phi * d;
                    o[1] = -cos_phi * sinf(theta_i) * d;
                    o[2] = -cos_phi * cosf(theta_i) * d;
                }
            } else if (convention == 1) {
                const float step_theta = 2 * kPI / cols;
                const float step_phi = step_theta;
                const int start_phi = 166;
                const float phi = (r + start_phi) * step_phi - kPI / 2;
                const float cos_phi = cosf(phi), sin_phi = sinf(phi);
                const float d = ((const float*)row)[c];
                if (d > 0.f && d < 15.f) {
                    const float theta = c * step_theta - kPI;
                    o[0] = sinf(theta) * cos_phi * d;
                    o[1] = sin_phi * d;
                    o[2] = cosf(theta) * cos_phi * d;
                }
            } else {
                const float angle_res = 2 * kPI / cols;
                const float half_nRows = 0.5 * rows - 0.5;
                const float theta = c * angle_res;
                const float phi = (half_nRows - r) * angle_res;
                const float d = depth_type == 0 ? (float)((const uint16_t*)row)[c] * 0.001f : ((const float*)row)[c];
                if (d != 0) {
                    o[0] = d * sinf(phi);
                    o[1] = -d * cosf(phi) * sinf(theta);
                    o[2] = -d * cosf(phi) * cosf(theta);
                }
            }
        }
    }
}

// Analytic warp Jacobian at a transformed point (finite-difference tests): rows d c'/d delta, d r'/d delta.
void oracle_warp_jacobian(const float* p, int nCols, float* Jw0, float* Jw1) {
    const float angle_res = 2 * kPI / nCols;
    const float angle_res_inv = 1 / angle_res;
    const float dist = sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
    warp_jacobian(p[0], p[1], p[2], 1.f / dist, angle_res_inv, Jw0, Jw1);
}

// Scalar probes for unit tests.
float oracle_asinf_poly(float x) { return asinf_poly(x); }
float oracle_atan2f_poly(float y, float x) { return atan2f_poly(y, x); }
float oracle_round_half_away(float x) { return round_half_away(x); }
int oracle_round_index(float x) { return round_index(x); }
float oracle_weight_huber(float e, float k) { return weightHuber(e, k); }
int oracle_rank6(const float* M) { return rank6_colpiv_qr(M); }
int oracle_inverse6(const float* M, float* inv) { return inverse6_partial_piv_lu(M, inv) ? 0 : 1; }
void oracle_se3_pseudo_exp(const double* v, double* M) { se3_pseudo_exp(v, M); }
void oracle_set_num_threads(int n) {
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}
int oracle_num_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

}  // extern "C"
