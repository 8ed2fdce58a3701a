// wave_scan.h -- the inclusive scan over the 64 lanes of a wave on the VALU's data-parallel-primitive paths, for both device translation
// units (occlusion_kernels.h, frame360_kernels.h): shifts by 1, 2, 4, 8 inside the rows of 16 lanes (row_shr), then lane 15 of a row to
// the next row (row_bcast:15 into rows 1 and 3) and lane 31 to the upper half (row_bcast:31 into rows 2 and 3).  Twelve vector
// instructions for a 32-bit max-scan; six __shfl_up steps are six trips through the LDS crossbar (~100 cycles each for a wave that has
// the SIMD to itself).  The six (control, row mask) pairs are written in wave_scan_fold; a scan is its combine step.  The running
// value goes through the steps BY VALUE: a functor that captures it by reference compiles the multi-word scans to other machine code
// than their hand-written ladders did.  NOT on it (docs/HISTORY.md): f360::wave_sum_ll, whose 64-bit sum comes out as two 64-bit adds
// per step instead of one in either form.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace r360 {

// x of the lane the path names, as an int; a lane without a source, or in a row outside the mask, gets old_.  The builtin needs
// immediates: a step functor passes the std::integral_constant pair (dispatch.h's idiom) it is handed as ctrl.value, rows.value.
#define R360_DPP(old_, src_, ctrl_, rows_) __builtin_amdgcn_update_dpp((int)(old_), (int)(src_), ctrl_, rows_, 0xF, false)

// s = step(s, control, row mask) for the six steps of the scan, in order: `step` reads its source lane through R360_DPP and returns
// the running value folded with it (always_inline on the lambda: inlined before the optimiser looks at it, like a __forceinline__)
template <class S, class Step>
__device__ __forceinline__ S wave_scan_fold(S s, Step step) {
    constexpr std::integral_constant<int, 0xF> all_rows{};
    s = step(s, std::integral_constant<int, 0x111>{}, all_rows);                                    // row_shr:1
    s = step(s, std::integral_constant<int, 0x112>{}, all_rows);                                    // row_shr:2
    s = step(s, std::integral_constant<int, 0x114>{}, all_rows);                                    // row_shr:4
    s = step(s, std::integral_constant<int, 0x118>{}, all_rows);                                    // row_shr:8
    s = step(s, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{});          // row_bcast:15 -> rows 1, 3
    s = step(s, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{});          // row_bcast:31 -> rows 2, 3
    return s;
}

// inclusive max-scan of values >= -1 (lanes without a source take -1)
__device__ __forceinline__ int wave_scan_max(int x) {
    return wave_scan_fold(x, [](int x, auto ctrl, auto rows) __attribute__((always_inline)) {
        const int t = R360_DPP(-1, x, ctrl.value, rows.value);
        return t > x ? t : x;
    });
}
// inclusive add-scan for small non-negative counts (lanes without a source add 0)
__device__ __forceinline__ int wave_scan_add(int x) {
    return wave_scan_fold(x, [](int x, auto ctrl, auto rows) __attribute__((always_inline)) { return x + R360_DPP(0, x, ctrl.value, rows.value); });
}

}  // namespace r360
