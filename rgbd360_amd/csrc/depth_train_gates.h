// depth_train_gates.h -- steps "measurement ... multiplier" of a pixel of the map or image route (and, behind them, the bin and the three
// terms of an example), included INSIDE k_depth_train (depth_train.h) and k_depth_eval (depth_apply.h): one text, so that the evaluation
// judges a model on exactly the trainer's examples, and the trainer's machine code is what it was before the evaluation existed (an
// inlined function changed its schedule; see map_align_eval_tile.h).  No include guard.  The including kernel provides, under these
// names: J (vmap::TrainJob), v, u, in (the pixel and whether it lies in the image), MAP and LAYER.  It leaves: meas32, gt32, cat (the one
// counter of the pixel), reached (step 2 onwards), example, bin and term[3].
    const float meas32 = in ? train_depth_at(J.meas, J.meas_step, J.depth_type, v, u) : 0.f;
    const bool measured = in && __builtin_isfinite(meas32) && meas32 > 0.f;
    int cat = kTrNoMeas;                 // the one counter of this pixel
    float gt32 = 0.f;
    if (MAP) {
        if (measured) {
            const float fx = ((float)u - J.cx) / J.fx, fy = ((float)v - J.cy) / J.fy, fz = 1.f;
            float o[3], d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                d[k] = (J.pose[k] * fx + J.pose[k + 4] * fy) + J.pose[k + 8] * fz;
                o[k] = J.pose[12 + k];
            }
            RayResult H;
            cast_ray<LAYER>(J.G, J.P, o, d, H);
            cat = kTrNoHit;
            if (H.status == kRayHit) {
                const uint4 rec = J.normals[(H.rec - J.G.table) / kFields];
                float c[3], nrm[3];
                centroid(H.rec, H.rec[1], c);
                double t = H.t;
                const bool on_plane = surface_step(rec, c, o, d, J.P.t_min, (double)J.P.inv_leaf, J.shift2_max, nrm, t);
                cat = kTrExamples;
                if (J.require_plane && !on_plane) {
                    cat = kTrOffPlane;
                } else if (J.min_cos > 0.0) {
                    const NormalRec R = normal_unpack(rec);
                    const double q = ((double)R.n[0] * (double)d[0] + (double)R.n[1] * (double)d[1]) + (double)R.n[2] * (double)d[2];
                    const double dd = ((double)d[0] * (double)d[0] + (double)d[1] * (double)d[1]) + (double)d[2] * (double)d[2];
                    if (R.status != kClassKept || fabs(q) < J.min_cos * sqrt(dd)) cat = kTrGrazing;
                }
                if (cat == kTrExamples) gt32 = (float)t;
            }
        }
    } else if (in) {
        const float g = train_depth_at(J.gt, J.gt_step, J.depth_type, v, u);
        if (!(__builtin_isfinite(g) && g > 0.f)) cat = kTrNoHit;
        else if (measured) cat = kTrExamples, gt32 = g;
    }
    const bool reached = in && cat == kTrExamples;      // step 2 onwards
    long long term[3] = {0ll, 0ll, 0ll};
    int bin = 0;
    if (reached) {
        const double gt = (double)gt32, meas = (double)meas32;
        const double mult = gt / meas;
        if (meas > J.max_range || gt > J.max_range) {
            cat = kTrRange;
        } else if (mult > J.max_mult || mult < J.min_mult) {
            cat = kTrMult;
        } else {
            const double sl = __builtin_floor(meas / J.bin_depth);
            const int idx = sl < (double)(J.nb - 1) ? (int)sl : J.nb - 1;
            const int by = min(v / J.bin_height, J.nby - 1), bx = min(u / J.bin_width, J.nbx - 1);
            bin = (by * J.nbx + bx) * J.nb + idx;
            term[0] = 1ll;
            term[1] = __double2ll_rn(gt * gt * 1048576.0);
            term[2] = __double2ll_rn(gt * meas * 1048576.0);
        }
    }
    const bool example = reached && cat == kTrExamples;
