// lm_host_check.cpp -- the host Levenberg-Marquardt driver (rgbd360_amd/csrc/lm_host.h) on a closed-form problem, no device and no image:
//   g++ -O2 -ffp-contract=off -fsanitize=address,undefined -I rgbd360_amd/csrc tools/lm_host_check.cpp -o lm_host_check && ./lm_host_check
// The evaluator is a 6-parameter least-squares toy: 40 fixed 3-D point pairs q = T_true p, residual r = w (T p - q), Jacobian of the
// left-multiplied update J = w [I | -[T p]x], H = sum J^T J and g = sum J^T r in double, packed into one totals row (partial_row.h).
// It prints, per scripted scenario, every trip and retry the driver walked and how it ended; tests/test_lm_host_cpu.py reads the lines.
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "gn_math.h"
#include "lm_host.h"

namespace {

constexpr int kPoints = 40;
constexpr double kWeight = 50;      // 1 / sigma: puts the rig schedule's tol_residual = 0.1 (on the plain sum) well below the first errors

struct Toy {
    double p[kPoints][3], q[kPoints][3];
    // the scripted faults
    int rank3_from_call = 0;        // > 0: from this call on the rotational columns of J are dropped (H has rank 3)
    bool no_depth_pixel = false;    // nd = 0: the pinhole error is 0 / 0
    double worse_per_call = 0;      // added to e2d, times the call number within the level: every candidate is worse than the pose
    int fail_at_call = 0, fail_rc = 0;
    int calls = 0, level_calls = 0;

    Toy() {
        uint32_t s = 12345u;
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24); };
        const double v[6] = {0.05, -0.03, 0.04, 0.02, -0.03, 0.025};
        double T[16];
        gn::se3_exp(v, T);
        for (int i = 0; i < kPoints; ++i) {
            for (int k = 0; k < 3; ++k) p[i][k] = 4.0 * rnd() - 2.0;
            p[i][2] += 3.0;
            for (int k = 0; k < 3; ++k) q[i][k] = T[0 * 4 + k] * p[i][0] + T[1 * 4 + k] * p[i][1] + T[2 * 4 + k] * p[i][2] + T[12 + k];
        }
    }

    // level 1 sees every other point
    int eval(int level, const float* pose, lm::Sums& S) {
        ++calls;
        ++level_calls;
        if (fail_at_call && calls == fail_at_call) return fail_rc;
        double tot[r360::kNumPartials] = {0};
        const bool rank3 = rank3_from_call && calls >= rank3_from_call;
        int n = 0;
        for (int i = 0; i < kPoints; i += level + 1, ++n) {
            double y[3], r[3];
            for (int k = 0; k < 3; ++k) {
                y[k] = (double)pose[0 * 4 + k] * p[i][0] + (double)pose[1 * 4 + k] * p[i][1] + (double)pose[2 * 4 + k] * p[i][2] + (double)pose[12 + k];
                r[k] = kWeight * (y[k] - q[i][k]);
            }
            const double skew[3][3] = {{0, -y[2], y[1]}, {y[2], 0, -y[0]}, {-y[1], y[0], 0}};
            for (int row = 0; row < 3; ++row) {
                double J[6] = {0, 0, 0, 0, 0, 0};
                J[row] = kWeight;
                if (!rank3)
                    for (int k = 0; k < 3; ++k) J[3 + k] = -kWeight * skew[row][k];
                int k = 0;
                for (int a = 0; a < 6; ++a)
                    for (int c = a; c < 6; ++c, ++k) tot[r360::P_H + k] += J[a] * J[c];
                for (int a = 0; a < 6; ++a) tot[r360::P_G + a] += J[a] * r[row];
                tot[r360::P_E2D] += r[row] * r[row];
            }
        }
        if (level_calls > 1) tot[r360::P_E2D] += worse_per_call * level_calls;
        tot[r360::P_ND] = no_depth_pixel ? 0 : n;
        tot[r360::P_NVIS] = 3 * n;
        S.add_row(tot);
        return 0;
    }
};

std::string hex(const float* v, int n) {
    std::string s;
    char b[16];
    for (int i = 0; i < n; ++i) {
        uint32_t u;
        memcpy(&u, v + i, 4);
        snprintf(b, sizeof(b), "%08x", u);
        s += b;
    }
    return s;
}

// the pinhole path's error (both averages / the depth count) or the rig's (the plain sum)
double rms_error(const lm::Sums& S) { return sqrt(S.e2p / S.nd) + sqrt(S.e2d / S.nd); }
double sum_error(const lm::Sums& S) { return S.e2p + S.e2d; }

void run(const char* name, const lm::Schedule& sch, Toy toy, double (*error_of)(const lm::Sums&)) {
    printf("scenario %s\n", name);
    const double v0[6] = {0.1, 0.08, -0.06, 0.05, -0.04, 0.06};      // the perturbed start
    double G[16];
    gn::se3_exp(v0, G);
    float guess[16], pose_out[16];
    for (int k = 0; k < 16; ++k) {
        guess[k] = (float)G[k];
        pose_out[k] = -7.f;      // stays as it is unless the driver returns 0
    }
    // what this program follows beside the driver, to name each evaluation: the pose the level stands at and its error, the last pose
    // evaluated and its error, and the pose a retry of the current trip would evaluate (lambda * step)
    float cur[16], last[16], retry[16];
    double cur_error = 0, last_error = 0;
    bool level_start = false, retry_armed = false;
    float retry_lambda = 0;
    auto begin_level = [&](int) {
        level_start = true;
        toy.level_calls = 0;
        return 0;
    };
    auto eval = [&](int level, const float* pose, lm::Sums& S) {
        const int rc = toy.eval(level, pose, S);
        if (rc) return rc;
        memcpy(last, pose, sizeof(last));
        last_error = error_of(S);
        if (level_start) {
            memcpy(cur, pose, sizeof(cur));
            cur_error = last_error;
            level_start = false;
        } else if (retry_armed && memcmp(pose, retry, sizeof(retry)) == 0) {
            const bool accepted = cur_error - last_error > 0;
            printf("retry level %d lambda %.9g accepted %d\n", level, (double)retry_lambda, (int)accepted);
            if (accepted) {
                memcpy(cur, pose, sizeof(cur));
                cur_error = last_error;
            }
        }
        retry_armed = false;
        return 0;
    };
    auto on_trip = [&](const lm::Trip& t) {
        float tmp[16], u_gn[6], u_lm[6];
        const bool gn_ok = gn::lm_update(t.H, t.g, -1.f, cur, tmp, u_gn), lm_ok = gn::lm_update(t.H, t.g, t.lambda, cur, tmp, u_lm);
        const char* first = gn_ok && memcmp(u_gn, t.update, sizeof(u_gn)) == 0 ? "undamped" : lm_ok && memcmp(u_lm, t.update, sizeof(u_lm)) == 0 ? "damped" : "neither";
        const bool accepted = t.error - t.new_error > 0;
        printf("trip level %d it %d lambda %.9g first %s accepted %d rows %lld\n", t.level, t.it, (double)t.lambda, first, (int)accepted, t.at_pose->rows);
        if (accepted) {
            memcpy(cur, last, sizeof(cur));
            cur_error = last_error;
        } else {
            float u[6];
            retry_lambda = t.lambda * sch.step;
            retry_armed = gn::lm_update(t.H, t.g, retry_lambda, cur, retry, u);
        }
    };
    lm::Outcome O;
    const int rc = lm::align(sch, 2, guess, begin_level, eval, error_of, on_trip, &O);
    if (rc == 0) memcpy(pose_out, O.pose, sizeof(pose_out));
    printf("end rc %d status %d iters0 %d iters1 %d any_trip %d final_error %.17g calls %d pose %s\n", rc, rc ? -1 : O.status, rc ? -1 : O.iters[0],
           rc ? -1 : O.iters[1], rc ? -1 : (int)O.any_trip, rc ? 0.0 : O.final_error, toy.calls, hex(pose_out, 16).c_str());
}

}  // namespace

int main() {
    const lm::Schedule pin = lm::pinhole_schedule(), rig = lm::rig_schedule();
    printf("schedule pinhole lambda0 %.9g step %g maxIters %d LM_maxIters %u tol_residual %.17g tol_update %.17g undamped_first %d ill_posed_records_iters %d\n", (double)pin.lambda0,
           pin.step, pin.maxIters, pin.LM_maxIters, pin.tol_residual, pin.tol_update, (int)pin.undamped_first, (int)pin.ill_posed_records_iters);
    printf("schedule rig lambda0 %.9g step %g maxIters %d LM_maxIters %u tol_residual %.17g tol_update %.17g undamped_first %d ill_posed_records_iters %d\n", (double)rig.lambda0,
           rig.step, rig.maxIters, rig.LM_maxIters, rig.tol_residual, rig.tol_update, (int)rig.undamped_first, (int)rig.ill_posed_records_iters);
    Toy toy;
    run("converge/pinhole", pin, toy, rms_error);
    run("converge/rig", rig, toy, sum_error);
    // call 1 = the level's pose, call 2 = the first candidate (accepted, it = 1); the second trip meets its rank-3 H
    Toy r3 = toy;
    r3.rank3_from_call = 2;
    run("rank3/pinhole", pin, r3, rms_error);
    run("rank3/rig", rig, r3, sum_error);
    lm::Schedule pin_rec = pin, rig_norec = rig;      // the flag alone, on the other path's numbers
    pin_rec.ill_posed_records_iters = true;
    rig_norec.ill_posed_records_iters = false;
    run("rank3/pinhole+records", pin_rec, r3, rms_error);
    run("rank3/rig-records", rig_norec, r3, sum_error);
    Toy nan = toy;
    nan.no_depth_pixel = true;
    run("nan/pinhole", pin, nan, rms_error);
    Toy worse = toy;
    worse.worse_per_call = 1e6;
    run("worse/pinhole", pin, worse, rms_error);
    run("worse/rig", rig, worse, sum_error);
    Toy bad = toy;
    bad.fail_at_call = 2;
    bad.fail_rc = -1703;
    run("fail/pinhole", pin, bad, rms_error);
    run("fail/rig", rig, bad, sum_error);
    return 0;
}
