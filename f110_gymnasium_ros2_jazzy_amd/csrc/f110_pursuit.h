// f110_pursuit.h — the row rule of the pure-pursuit opponent (private; include/f110.h, "pure-pursuit
// opponent"): what follows a car's projection onto the centerline.  k_pursuit (f110_pursuit.hip)
// and f110_host_pure_pursuit (f110_task_capi.cpp) both call it, so the device and the host
// statement differ in nothing but the platform's atan.  f64, left to right, no FMA.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/f110.h"
#include "f110_math.h"
#include "f110_sincos.h"

namespace f110 {

// The arguments f110_pure_pursuit and f110_host_pure_pursuit refuse (F110_E_INVALID); L is the
// track's length.  Written so that a NaN fails every test it enters.
inline bool pursuit_bad_args(const f110_pursuit_params *p, double L, const float *poses, int64_t n_rows,
                             int64_t pose_stride, const float *actions, int64_t action_stride) {
    if (!p || !poses || !actions || n_rows < 0 || pose_stride < 3 || action_stride < 2) return true;
    if (!(p->lookahead > 0.0 && p->lookahead < L)) return true;
    if (!(p->wheelbase > 0.0) || !(p->steer_limit > 0.0) || !(p->speed >= 0.0) || !(p->a_lat >= 0.0)) return true;
    return p->direction != 1 && p->direction != -1;
}

// The arclength the car aims at: lookahead ahead of its projection, wrapped once on a closed
// track, clamped to the ends of an open one (NaN stays NaN).
F110_HD double pursuit_query(const f110_pursuit_params &P, double s_proj, int closed, double L) {
    double sq = s_proj + (double)P.direction * P.lookahead;
    if (closed) {
        if (sq > L) sq -= L;
        if (sq < 0.0) sq += L;
    } else {
        sq = sq < 0.0 ? 0.0 : (sq > L ? L : sq);
    }
    return sq;
}

struct PursuitAction {
    double steer, v, tx, ty;  // the action and the target point
};

// The target at arclength sq on segment i (= seg_at(sq)) of the centerline xy / s, and the action
// of the car at (x, y, yaw) that aims at it; v: the row's speed cap.
F110_HD PursuitAction pursuit_action(const f110_pursuit_params &P, const double *xy, const double *s, int32_t i,
                                     double sq, double x, double y, double yaw, double v) {
    const double len = s[i + 1] - s[i];
    const double u = len == 0.0 ? 0.0 : (sq - s[i]) / len;
    const double ax = xy[2 * i], ay = xy[2 * i + 1];
    const double tx = ax + u * (xy[2 * i + 2] - ax), ty = ay + u * (xy[2 * i + 3] - ay);
    const double dx = tx - x, dy = ty - y;
    const double d2 = dx * dx + dy * dy;
    double sn, cs;
    cr_sincos(yaw, sn, cs);
    const double ly = -sn * dx + cs * dy;  // the target's lateral offset in the car's frame
    const double kappa = 2.0 * ly / d2;    // the arc through the car, tangent to its heading, and the target
    double steer = clip(atan(P.wheelbase * kappa), -P.steer_limit, P.steer_limit);
    if (P.a_lat > 0.0) {  // no faster than the lateral acceleration allows on that arc
        double ak = fabs(kappa);
        if (!(ak > 1e-9)) ak = 1e-9;
        double c = sqrt(P.a_lat / ak);
        c = c < P.v_floor ? P.v_floor : c;
        v = c > v ? v : c;
    }
    if (d2 <= 1e-12) steer = 0.0;  // on the target: no arc is defined
    return PursuitAction{steer, v, tx, ty};
}

}  // namespace f110
