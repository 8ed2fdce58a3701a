// warp_images.h -- the source frame warped into the target frame at one pose, and the two difference images: the per-pixel
// product of RegisterPhotoICP's visualisation path, without its windows.
//   warped_source_grayImage / warped_source_depthImage    RPI.h:163-166; filled inside calcHessGrad_sphere RPI.h:2779-2785, 3032-3033,
//                                                         3066-3067 and calcHessGrad RPI.h:805-811, 1025-1026, 1050-1051
//   imgDiff / depthDiff (cv::absdiff)                     RPI.h:4664-4676
//
// The reference's loop runs the source index i ascending and every write overwrites (RPI.h:2953; its OpenMP build races on the
// same element): the LARGEST source index that lands on a target pixel wins.  Two passes, the kernel boundary between them the
// only synchronisation:
//   k_warp_winner   one lane per SOURCE pixel: the warp of the per-pixel pass (warp_pixel / warp_pinhole, unchanged, either index
//                   arithmetic), and an integer atomicMax of the lane's index into the int32 winner plane (cleared to -1 on the
//                   stream beforehand).  An integer maximum does not depend on the order of arrival: the plane is the same
//                   from run to run.
//   k_warp_resolve  one lane per TARGET pixel: reads the winner, gathers that source record and warps it again through the same
//                   function (same bits) for the point's range, reads the pixel's two target records for the eligibility tests
//                   and the differences, and stores every requested plane (consecutive lanes, consecutive addresses).
// Whether a target pixel takes a depth write depends on the target pixel alone (finite target depth, RPI.h:3064; with PHOTO_DEPTH
// also the `continue` of the photometric saliency test, RPI.h:3038-3039 / 1031-1032, which skips the depth block), so the winner
// of the depth plane is the winner of the gray plane wherever depth is written.
#pragma once
#include "pinhole_kernels.h"

namespace r360 {

constexpr int kPixelThreads = 256;      // block of the one-lane-per-pixel stage kernels (grid: level_pixel_grid, level_geom.h)

struct WarpImagesOut {                  // any pointer may be null (the winner plane is the caller's buffer or the context's, never copied)
    float *warped_gray, *warped_depth, *diff_gray, *diff_depth;
};

// The warp of source record s as k_warp_indices / k_warp_indices_pinhole run it: visibility, the flat target index, and the value
// the depth plane takes (spherical: dist = |R p + t|, RPI.h:2976; pinhole: the transformed z, RPI.h:1051).
template <bool PINHOLE>
__device__ __forceinline__ bool warp_images_point(const LevelDev& lv, const PinK& K, const PoseRT& T, const float4 s, unsigned& ti,
                                                  float& range) {
    bool vis;
    if (PINHOLE) {
        float X, Y, Z, iz;
        ti = warp_pinhole(T, s.x, s.y, s.z, K, lv.rows, lv.cols, X, Y, Z, iz, vis, lv.libm);
        range = Z;
    } else {
        float X, Y, Z, rho2, d2;
        const WarpConsts wc = {T.tx, T.ty, T.tz, lv.half_nRows, lv.pi_k};
        ti = warp_pixel(T, wc, s.x, s.y, s.z, lv, X, Y, Z, rho2, d2, vis);
        // arithmetic 1: d2 = (X X + Y Y) + Z Z without fused operations and the root warp_pixel_libm itself takes (Eigen's norm());
        // arithmetic 0: d2 of the device definition (fused) and its correctly rounded root
        range = lv.libm ? libm32::sqrt32(d2) : sqrt_rn(d2);
    }
    return vis && s.x != kInvalidPoint;
}

template <bool PINHOLE>
__global__ __launch_bounds__(kPixelThreads) void k_warp_winner(LevelDev lv, PinK K, Pose16 pose, int32_t* __restrict__ winner) {
    const int i = blockIdx.x * kPixelThreads + threadIdx.x;
    const PoseRT T = load_pose(pose.v);
    // (no branch around the warp: its predicates are whole-wave lane masks; a lane past the end warps the last record and drops out below)
    const float4 s = lv.src[min(i, lv.n - 1)];
    unsigned ti;
    float range;
    const bool vis = warp_images_point<PINHOLE>(lv, K, T, s, ti, range);
    if (vis && i < lv.n && ti < (unsigned)lv.n) atomicMax(&winner[ti], i);
}

// method: 0 photo, 1 depth, 2 photo + depth (uniform)
template <bool PINHOLE>
__global__ __launch_bounds__(kPixelThreads) void k_warp_resolve(LevelDev lv, PinK K, Pose16 pose, int method, float thr_photo,
                                                                const int32_t* __restrict__ winner, WarpImagesOut out) {
    const int j = blockIdx.x * kPixelThreads + threadIdx.x;
    const PoseRT T = load_pose(pose.v);
    const int jc = min(j, lv.n - 1);
    const int w = winner[jc];
    const bool hit = w >= 0 && w < lv.n;
    const float4 s = lv.src[hit ? w : 0];
    unsigned ti;
    float range;
    (void)warp_images_point<PINHOLE>(lv, K, T, s, ti, range);
    if (j >= lv.n) return;
    const F3 tp = lv.trgP[j], td = lv.trgD[j];
    const bool photo = method != 1, depth = method != 0;
    // RPI.h:3033 / 1026: the gray write precedes the saliency test, so non-salient target pixels take a value too
    const float wg = (photo && hit) ? s.w : 0.f;
    // RPI.h:3038-3039 / 1031-1032: with PHOTO_DEPTH a non-salient target pixel `continue`s past the depth block
    const bool salient = !(fabsf(tp.b) < thr_photo && fabsf(tp.c) < thr_photo);
    // RPI.h:3064: the spherical pass writes only where the target has depth; RPI.h:1051: the pinhole pass does not test
    const bool takes_depth = depth && hit && (PINHOLE || isfinite(td.a)) && (method == 1 || salient);
    const float wd = takes_depth ? range : 0.f;
    if (out.warped_gray) out.warped_gray[j] = wg;
    if (out.warped_depth) out.warped_depth[j] = wd;
    // RPI.h:4664-4676: cv::absdiff over the whole level, holes included; each inside its method's branch
    if (out.diff_gray) out.diff_gray[j] = photo ? fabsf(tp.a - wg) : 0.f;
    if (out.diff_depth) out.diff_depth[j] = depth ? fabsf(td.a - wd) : 0.f;
}

}  // namespace r360
