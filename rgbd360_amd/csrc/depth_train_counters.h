// depth_train_counters.h -- the counters of a pixel's wave (rgbd360_depth_train_stats) through ballots, one add per wave and counter,
// included INSIDE k_depth_train (depth_train.h) and k_depth_eval (depth_apply.h) behind depth_train_gates.h: one text for both kernels.
// No include guard.  The including kernel provides J, lane, in and cat.
    unsigned long long b[kTrWords];
#pragma unroll
    for (int q = 1; q < kTrWords; ++q) b[q] = __ballot(in && cat == q);
    b[kTrPixels] = __ballot(in);
    if (lane == 0 && b[kTrPixels]) {      // one add per wave and counter
#pragma unroll
        for (int q = 0; q < kTrWords; ++q)
            if (b[q]) atomicAdd(J.stats + q, (unsigned long long)__popcll(b[q]));
    }
