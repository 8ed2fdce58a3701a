// lm_host.h -- the Levenberg-Marquardt loop that runs on the host, one device evaluation per candidate pose, written once for the two
// alignments that have it: the pinhole single-sensor path (rgbd360_align_pinhole, RPI.h:4254-4512) and the 8-sensor rig
// (rgbd360_rig_align, RegisterRGBD360.h:383-500).  Host only, no HIP: the sums of one evaluation, the schedule of a path as data, and the
// driver over the pyramid.  Everything in which the two paths differ is a field of their Schedule or one of the callables they hand in.
#pragma once
#include <math.h>
#include <string.h>

#include "gn_math.h"
#include "partial_row.h"

namespace lm {

// The sums of one evaluation at one pose: the rows of totals the device published (partial_row.h), added in the order given.
struct Sums {
    double e2p = 0, e2d = 0;
    long long np = 0, nd = 0, rows = 0;
    float H[36] = {0}, g[6] = {0};              // each row's entry cast to float, then added: `Hessian += alignSensorID[s].getHessian()`
    double H64[36] = {0}, g64[6] = {0};         //     (RegisterRGBD360.h:435-440); the pinhole path is the one-row case

    void add_row(const double* tot) {
        using namespace r360;
        e2p += tot[P_E2P]; e2d += tot[P_E2D];
        np += (long long)tot[P_NP]; nd += (long long)tot[P_ND]; rows += (long long)tot[P_NVIS];
        int k = 0;
        for (int a = 0; a < 6; ++a)
            for (int c = a; c < 6; ++c, ++k) {
                const float v = (float)tot[P_H + k];
                H[c * 6 + a] += v;
                H64[c * 6 + a] += tot[P_H + k];
                if (c != a) {
                    H[a * 6 + c] += v;
                    H64[a * 6 + c] += tot[P_H + k];
                }
            }
        for (int a = 0; a < 6; ++a) {
            g[a] += (float)tot[P_G + a];
            g64[a] += tot[P_G + a];
        }
    }

    // the out-parameter block of the evaluation entries (rgbd360_eval_occ, rgbd360_eval_pinhole_occ, rgbd360_rig_eval); null = not wanted
    void write(double err2_split[2], long long n_split[2], float H_out[36], float g_out[6], double H64_out[36], double g64_out[6],
               long long* n_rows) const {
        if (err2_split) { err2_split[0] = e2p; err2_split[1] = e2d; }
        if (n_split) { n_split[0] = np; n_split[1] = nd; }
        if (H_out) memcpy(H_out, H, sizeof(H));
        if (g_out) memcpy(g_out, g, sizeof(g));
        if (H64_out) memcpy(H64_out, H64, sizeof(H64));
        if (g64_out) memcpy(g64_out, g64, sizeof(g64));
        if (n_rows) *n_rows = rows;
    }
};

// What the reference hard-codes per path.  (Its sixth difference, how the error is taken from the sums, is the paths' error callable.)
struct Schedule {
    float lambda0;                  // damping at the start of every level (a double in the reference, used as a float scalar by Eigen)
    double step;                    // lambda /= step after an accepted first candidate, *= step before a retry
    int maxIters;                   // accepted steps per level
    unsigned LM_maxIters;           // retries per trip
    double tol_residual, tol_update;
    bool undamped_first;            // a trip's first candidate is the Gauss-Newton step (gn::lm_update with lambda < 0); retries always damp
    bool ill_posed_records_iters;   // an ILL-POSED level writes its `iters` entry and the final error before the pyramid is left
};
// RPI.h:4303-4308 (the pinhole driver hard-codes its own limits), 4355-4358 (undamped), 4346-4353 (ILL-POSED: return at once)
inline Schedule pinhole_schedule() { return {0.01f, 10, 10, 1, 1e-4, 1e-4, true, false}; }
// RegisterRGBD360.h:389-395, 452-455 (lambda is never negative: always damped), 443-449
inline Schedule rig_schedule() { return {0.001f, 10, 10, 1, pow(10, -1), pow(10, -6), false, true}; }

// One trip as the observer sees it: after the first candidate's evaluation, before it is accepted or retried.
struct Trip {
    int level, it;
    float lambda;
    double error, new_error;        // at the pose, at the candidate
    const float *update, *H, *g;    // the candidate's update; H, g of the pose
    const Sums* at_pose;
};

struct Outcome {
    int status = 0;                 // 0, or 1 = "The problem is ILL-POSED" (the pose reached so far is returned)
    float pose[16];
    int iters[8] = {0};
    float H[36] = {0}, g[6] = {0};  // of the last trip
    double final_error = 0;         // at the pose reached, of the last level that recorded one
    bool any_trip = false;
};

inline float update_norm(const float* u) {
    float s2 = 0;
    for (int i = 0; i < 6; ++i) s2 += u[i] * u[i];
    return sqrtf(s2);
}

// Coarse to fine over n_pyr levels from `guess`.
//   begin_level(level) -> rc                 once per level, before its first evaluation
//   eval(level, pose, Sums&) -> rc           one device evaluation
//   error_of(const Sums&) -> double
//   on_trip(const Trip&)                     once per trip that got as far as a candidate
// Returns 0 with *out filled, or the first non-zero rc of a callable (then *out is not meaningful).
template <class BeginLevel, class Eval, class ErrorOf, class OnTrip>
int align(const Schedule& sch, int n_pyr, const float* guess, BeginLevel&& begin_level, Eval&& eval, ErrorOf&& error_of, OnTrip&& on_trip,
          Outcome* out) {
    Outcome& O = *out;
    float *pose_estim = O.pose, pose_estim_temp[16];
    memcpy(pose_estim, guess, sizeof(O.pose));
    int rc = 0;
    for (int level = n_pyr - 1; level >= 0 && O.status == 0; --level) {
        if ((rc = begin_level(level)) != 0) return rc;
        float lambda = sch.lambda0;
        const double step = sch.step;
        int it = 0;
        float update_pose[6] = {1, 1, 1, 1, 1, 1};
        Sums at_pose, cand;
        if ((rc = eval(level, pose_estim, at_pose)) != 0) return rc;      // the error; doubles as the H,g pass of the first trip (same pose)
        double error = error_of(at_pose), new_error = 0;
        double diff_error = error;
        while (it < sch.maxIters && update_norm(update_pose) > sch.tol_update && diff_error > sch.tol_residual) {
            O.any_trip = true;
            memcpy(O.H, at_pose.H, sizeof(O.H));          // calcHessGrad(pose_estim): the fused pass at pose_estim
            memcpy(O.g, at_pose.g, sizeof(O.g));
            float M[36];
            for (int k = 0; k < 36; ++k) M[k] = O.H[k];
            for (int i = 0; i < 6; ++i) M[i * 6 + i] = O.H[i * 6 + i] + lambda * O.H[i * 6 + i];
            if (gn::rank6(M) != 6 || !gn::lm_update(O.H, O.g, sch.undamped_first ? -1.f : lambda, pose_estim, pose_estim_temp, update_pose)) {
                O.status = 1;
                break;
            }
            auto try_candidate = [&]() -> bool {          // pose_estim_temp into cand, new_error, diff_error; false: the evaluation failed (rc)
                cand = Sums();
                if ((rc = eval(level, pose_estim_temp, cand)) != 0) return false;
                new_error = error_of(cand);
                diff_error = error - new_error;
                return true;
            };
            if (!try_candidate()) return rc;
            on_trip(Trip{level, it, lambda, error, new_error, update_pose, O.H, O.g, &at_pose});
            auto accept = [&]() {
                memcpy(pose_estim, pose_estim_temp, sizeof(O.pose));
                error = new_error;
                it = it + 1;
                at_pose = cand;
            };
            if (diff_error > 0) {
                lambda /= step;
                accept();
            } else {
                // LM_it advances on every retry; the reference's pinhole form advances it on a rejected retry only, which is the same
                // walk as long as LM_maxIters == 1 (an accepted retry has diff_error > 0 and leaves the loop either way)
                for (unsigned LM_it = 0; LM_it < sch.LM_maxIters && diff_error < 0; LM_it = LM_it + 1) {
                    lambda = lambda * step;
                    if (!gn::lm_update(O.H, O.g, lambda, pose_estim, pose_estim_temp, update_pose)) break;
                    if (!try_candidate()) return rc;
                    if (diff_error > 0) accept();
                }
            }
        }
        if (O.status == 1 && !sch.ill_posed_records_iters) break;
        O.iters[level & 7] = it;
        O.final_error = error;
    }
    return 0;
}

}  // namespace lm
