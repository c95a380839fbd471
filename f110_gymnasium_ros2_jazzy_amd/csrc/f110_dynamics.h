// f110_dynamics.h — the vehicle model: the input constraints, the kinematic and single-track
// right-hand sides, the PID and RaceCar.update_pose (Euler and RK4).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/f110.h"
#include "f110_math.h"
#include "f110_sincos.h"

namespace f110 {

// ------------------------------------------------------------- dynamics --
// accl_constraints, dynamic_models.py:29-60
F110_HD double accl_constraints(double vel, double accl, double v_switch, double a_max, double v_min,
                                double v_max) {
    double pos_limit = vel > v_switch ? a_max * v_switch / vel : a_max;
    if ((vel <= v_min && accl <= 0) || (vel >= v_max && accl >= 0))
        accl = 0.;
    else if (accl <= -a_max)
        accl = -a_max;
    else if (accl >= pos_limit)
        accl = pos_limit;
    return accl;
}

// steering_constraint, dynamic_models.py:62-87
F110_HD double steering_constraint(double sa, double sv, double s_min, double s_max, double sv_min,
                                   double sv_max) {
    if ((sa <= s_min && sv <= 0) || (sa >= s_max && sv >= 0))
        sv = 0.;
    else if (sv <= sv_min)
        sv = sv_min;
    else if (sv >= sv_max)
        sv = sv_max;
    return sv;
}

// vehicle_dynamics_ks, dynamic_models.py:90-121: the kinematic single-track
// right-hand side of x[5] = (x, y, steer, v, yaw) under the constrained input.
F110_HD void vehicle_dynamics_ks(const double x[5], double u0_in, double u1_in, const f110_params &p,
                                 double f[5]) {
    const double lwb = p.lf + p.lr;
    const double u0 = steering_constraint(x[2], u0_in, p.s_min, p.s_max, p.sv_min, p.sv_max);
    const double u1 = accl_constraints(x[3], u1_in, p.v_switch, p.a_max, p.v_min, p.v_max);
    double s4, c4;
    cr_sincos(x[4], s4, c4);
    f[0] = x[3] * c4;
    f[1] = x[3] * s4;
    f[2] = u0;
    f[3] = u1;
    double tn, c2;
    bool ok_t, ok_c;
    tan_cos_fast(x[2], kSinCosTab, tn, c2, ok_t, ok_c);
    if (!ok_t) tn = tan(x[2]);
    f[4] = x[3] / lwb * tn;
}

// vehicle_dynamics_st, dynamic_models.py:123-176 (KS branch :152-160 via
// vehicle_dynamics_ks :90-121).  Python's left-to-right order kept.  tn, c2: tan(x[2]) and
// cr_cos(x[2]), the kinematic model's (the caller may have them already, see update_pose_impl).
F110_HD void vehicle_dynamics_st_tc(const double x[7], double u0_in, double u1_in, const f110_params &p,
                                    double f[7], const double (*tab)[4], double tn, double c2) {
    const double mu = p.mu, C_Sf = p.C_Sf, C_Sr = p.C_Sr, lf = p.lf, lr = p.lr, h = p.h, m = p.m, I = p.I;
    double u0 = steering_constraint(x[2], u0_in, p.s_min, p.s_max, p.sv_min, p.sv_max);
    double u1 = accl_constraints(x[3], u1_in, p.v_switch, p.a_max, p.v_min, p.v_max);
    // Both models are evaluated for every car and the car's own is selected
    // (dynamic_models.py:263-283: the kinematic model below |v| = 0.5): the
    // transcendentals and divisions of the two are independent chains, so a
    // wave holding both kinds of car waits for the longer one instead of the
    // sum (this launch is latency-bound: one wave per SIMD).  f[0], f[1] take
    // one sincos of the car's own angle (the yaw, or yaw + slip).
    const bool kinematic = fabs(x[3]) < 0.5;
    const double ang = kinematic ? x[4] : x[6] + x[4];
    double sy, cy;
    const bool sc_ok = cr_sincos_fast(ang, sy, cy, tab);  // (cr_sincos below when not certain)
    // kinematic (vehicle_dynamics_ks re-applies the (idempotent) constraints to u)
    const double lwb = lf + lr;
    const double k0 = steering_constraint(x[2], u0, p.s_min, p.s_max, p.sv_min, p.sv_max);
    const double k1 = accl_constraints(x[3], u1, p.v_switch, p.a_max, p.v_min, p.v_max);
    const double kf4 = x[3] / lwb * tn;
    const double kf5 = u1 / lwb * tn + x[3] / (lwb * (c2 * c2)) * u0;
    // single track
    const double glr_m = kG * lr - u1 * h;
    const double glf_p = kG * lf + u1 * h;
    const double lrlf = lr + lf;
    const double t1 = -mu * m / (x[3] * I * lrlf) * (lf * lf * C_Sf * glr_m + lr * lr * C_Sr * glf_p) * x[5];
    const double t2 = mu * m / (I * lrlf) * (lr * C_Sr * glf_p - lf * C_Sf * glr_m) * x[6];
    const double t3 = mu * m / (I * lrlf) * lf * C_Sf * glr_m * x[2];
    const double s1 = (mu / (x[3] * x[3] * lrlf) * (C_Sr * glf_p * lr - C_Sf * glr_m * lf) - 1) * x[5];
    const double s2 = mu / (x[3] * lrlf) * (C_Sr * glf_p + C_Sf * glr_m) * x[6];
    const double s3 = mu / (x[3] * lrlf) * (C_Sf * glr_m) * x[2];
    if (!sc_ok) cr_sincos(ang, sy, cy, tab);  // rare: after the independent work above
    f[0] = x[3] * cy;
    f[1] = x[3] * sy;
    f[2] = kinematic ? k0 : u0;
    f[3] = kinematic ? k1 : u1;
    f[4] = kinematic ? kf4 : x[5];
    f[5] = kinematic ? kf5 : t1 + t2 + t3;
    f[6] = kinematic ? 0.0 : s1 - s2 + s3;
}

F110_HD void vehicle_dynamics_st(const double x[7], double u0_in, double u1_in, const f110_params &p,
                                 double f[7], const double (*tab)[4] = kSinCosTab) {
    double tn, c2;
    bool ok_t, ok_c;
    tan_cos_fast(x[2], tab, tn, c2, ok_t, ok_c);
    if (!ok_t) tn = tan(x[2]);
    if (!ok_c) c2 = cr_cos(x[2], tab);
    vehicle_dynamics_st_tc(x, u0_in, u1_in, p, f, tab, tn, c2);
}

// The steering angle and speed of RK4's four stages (xs[2], xs[3] of update_pose_impl) depend
// only on themselves: f[2] and f[3] are the constrained inputs, and the model choice |v| < 0.5
// reads the speed.  Their chains are a few compares and products, so they run first, and the
// kinematic model's tan / cos of the four steering angles -- a stage's largest independent work --
// are issued together (k_agents is one wave per SIMD: issue- and latency-bound) instead of one
// pair per stage.  Same operations as vehicle_dynamics_st's, so the same values.
F110_HD void steer_stage_trig(double s2, double s3, double sv, double accl, const f110_params &p, double dt,
                              const double (*tab)[4], double tn[4], double c2[4]) {
    double x2[4], x3[4];
    x2[0] = s2;
    x3[0] = s3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double u0 = steering_constraint(x2[j], sv, p.s_min, p.s_max, p.sv_min, p.sv_max);
        const double u1 = accl_constraints(x3[j], accl, p.v_switch, p.a_max, p.v_min, p.v_max);
        const bool kinematic = fabs(x3[j]) < 0.5;
        const double k0 = steering_constraint(x2[j], u0, p.s_min, p.s_max, p.sv_min, p.sv_max);
        const double k1 = accl_constraints(x3[j], u1, p.v_switch, p.a_max, p.v_min, p.v_max);
        const double f2 = kinematic ? k0 : u0, f3 = kinematic ? k1 : u1;
        x2[j + 1] = j < 2 ? s2 + dt * (f2 / 2) : s2 + dt * f2;  // the stages' xs = s + dt k/2, s + dt k
        x3[j + 1] = j < 2 ? s3 + dt * (f3 / 2) : s3 + dt * f3;
    }
    bool okt[4], okc[4], ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // the four (tan, cos) as one straight-line block
        tan_cos_fast(x2[j], tab, tn[j], c2[j], okt[j], okc[j]);
        ok = ok & okt[j] & okc[j];
    }
    if (!ok) {  // rare: an uncertain rounding
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            if (!okt[j]) tn[j] = tan(x2[j]);
            if (!okc[j]) c2[j] = cr_cos(x2[j], tab);
        }
    }
}

// pid, dynamic_models.py:178-221 (v_min = 1e-8 braking quirk included).
F110_HD void pid(double speed, double steer, double cur_speed, double cur_steer, double max_sv, double max_a,
                 double max_v, double min_v, double &accl, double &sv) {
    double steer_diff = steer - cur_steer;
    sv = fabs(steer_diff) > 1e-4 ? (steer_diff / fabs(steer_diff)) * max_sv : 0.0;
    double vel_diff = speed - cur_speed;
    double kp;
    if (cur_speed > 0.)
        kp = vel_diff > 0 ? 10.0 * max_a / max_v : 10.0 * max_a / (-min_v);
    else
        kp = vel_diff > 0 ? 2.0 * max_a / max_v : 2.0 * max_a / (-min_v);
    accl = kp * vel_diff;
}

// RaceCar.update_pose without the scan, base_classes.py:256-417.
// s[7] in/out; b0 = newest buffered steer, b1 = older; cnt = buffer fill.
// RaceCar.update_pose on a state array s (and an accumulator scratch acc) that
// are plain arrays (registers) or volatile LDS arrays (k_step1: every stage
// re-reads s and acc from LDS, so that only one vehicle_dynamics_st evaluation
// is in registers at a time).  Same operations in the same order either way.
template <class V>
F110_HD void update_pose_impl(V s, V acc, double &b0, double &b1, int &cnt, double raw_steer, double vel,
                              const f110_params &p, double dt, int integrator, const double (*tab)[4] = kSinCosTab) {
    double steer;
    if (cnt < 2) {  // :272-274
        steer = 0.0;
        b1 = b0;
        b0 = raw_steer;
        cnt += 1;
    } else {        // :275-278
        steer = b1;
        b1 = b0;
        b0 = raw_steer;
    }
    double accl, sv;
    pid(vel, steer, s[3], s[2], p.sv_max, p.a_max, p.v_max, p.v_min, accl, sv);
    sv = clip(sv, p.sv_min, p.sv_max);
    accl = clip(accl, -p.a_max, p.a_max);
    double k[7], xs[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) xs[i] = s[i];
    if (integrator == F110_INTEGRATOR_RK4) {  // :285-374
        // k1 + 2*k2 + 2*k3 + k4 is summed left to right as the stages come
        // (((k1 + 2k2) + 2k3) + k4: the reference's rounding order), so only
        // one stage's k is live at a time
        double tn[4], c2[4];
        steer_stage_trig(s[2], s[3], sv, accl, p, dt, tab, tn, c2);
        // the four stages as one loop body (one copy of the model's code: k_agents' instructions are
        // read from L2 once per wave), the same operations in the same order as written out
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            const double tns = st == 0 ? tn[0] : st == 1 ? tn[1] : st == 2 ? tn[2] : tn[3];
            const double c2s = st == 0 ? c2[0] : st == 1 ? c2[1] : st == 2 ? c2[2] : c2[3];
            vehicle_dynamics_st_tc(xs, sv, accl, p, k, tab, tns, c2s);
            if (st == 3) break;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                acc[i] = st == 0 ? k[i] : acc[i] + 2 * k[i];
                xs[i] = st < 2 ? s[i] + dt * (k[i] / 2) : s[i] + dt * k[i];
            }
        }
        const double w = dt * (1.0 / 6.0);
#pragma unroll
        for (int i = 0; i < 7; ++i) s[i] = s[i] + w * (acc[i] + k[i]);
    } else {                                  // :376-396
        vehicle_dynamics_st(xs, sv, accl, p, k, tab);
#pragma unroll
        for (int i = 0; i < 7; ++i) s[i] = s[i] + dt * k[i];
    }
    s[2] = clip(s[2], p.s_min, p.s_max);   // :400-401
    s[3] = clip(s[3], p.v_min, p.v_max);
    s[4] = wrap_angle(s[4]);               // :408
    double yr = s[5];                      // :410-412
    if (yr != yr) yr = 0.0;
    else if (isinf(yr)) yr = yr > 0 ? kYawRateCap : -kYawRateCap;
    s[5] = clip(yr, -kYawRateCap, kYawRateCap);
    double sl = s[6];                      // :414-417
    if (sl != sl) sl = 0.0;
    s[6] = clip(sl, -kSlipCap, kSlipCap);
}

F110_HD void update_pose(double s[7], double &b0, double &b1, int &cnt, double raw_steer, double vel,
                         const f110_params &p, double dt, int integrator, const double (*tab)[4] = kSinCosTab) {
    double acc[7];
    update_pose_impl<double *>(s, acc, b0, b1, cnt, raw_steer, vel, p, dt, integrator, tab);
}

}  // namespace f110
