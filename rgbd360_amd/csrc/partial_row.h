// partial_row.h -- the layout of one row of reduced sums (32 doubles), shared by the evaluation kernels that write it
// (photo_icp_kernels.h) and the host code that unpacks it (lm_host.h); no HIP needed.
#pragma once

namespace r360 {

constexpr int    kNumPartials = 32;             // doubles per block partial
// partial slots
enum { P_H = 0 /*21*/, P_G = 21 /*6*/, P_E2P = 27, P_E2D = 28, P_NP = 29, P_ND = 30, P_NVIS = 31 };

}  // namespace r360
