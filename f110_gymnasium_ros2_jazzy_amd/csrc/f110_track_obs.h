// f110_track_obs.h — the row rule of the track observation (private; include/f110.h, "track
// observation"): what follows the cars' projections onto the centerline.  k_track_obs
// (f110_track_obs.hip) and f110_host_track_obs (f110_task_capi.cpp) both call it, and no libm
// function but sqrt enters, so the device and the host statement agree in every bit.  f64, left to
// right, no FMA.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/f110.h"
#include "f110_math.h"
#include "f110_race.h"

namespace f110 {

constexpr int kTrackObsOwn = 7;         // columns of the seat's own state and its place on the line
constexpr int kTrackObsMaxPreview = 8;  // f110_track_obs_params.preview
constexpr int kTrackObsGap = 3;         // columns of the other car
constexpr int kTrackObsMaxWidth = 28;   // 7 + 2*8 + 3 rounded up: every row fits a half-wave

static_assert(sizeof(f110_track_obs_params) == 120, "f110_track_obs_params: fourteen doubles, two int32");

// 7 + 2*n_preview + (has_other ? 3 : 0) rounded up to a multiple of 4
inline int32_t track_obs_width(int32_t n_preview, int has_other) {
    return (kTrackObsOwn + 2 * n_preview + (has_other ? kTrackObsGap : 0) + 3) / 4 * 4;
}

// The arguments f110_track_obs, f110_ctx_track_obs and f110_host_track_obs refuse (F110_E_INVALID),
// the track aside; L is its length.  Written so that a NaN fails every test it enters.
inline bool track_obs_bad_args(const f110_track_obs_params *p, double L, const double *state, int64_t n_envs,
                               int32_t n_agents, int32_t seat, int32_t other, const float *out, int64_t out_stride) {
    if (!p || !state || !out || n_envs < 0 || n_agents < 1 || n_agents > kMaxAgents) return true;
    if (seat < 0 || seat >= n_agents || other < -1 || other >= n_agents || other == seat) return true;
    if (!(p->v_scale > 0.0) || !(p->steer_scale > 0.0) || !(p->yaw_rate_scale > 0.0) || !(p->slip_scale > 0.0) ||
        !(p->lat_scale > 0.0) || !(p->gap_scale > 0.0))
        return true;
    if (p->n_preview < 0 || p->n_preview > kTrackObsMaxPreview) return true;
    for (int j = 0; j < p->n_preview; ++j)
        if (!(p->preview[j] > 0.0 && p->preview[j] < L)) return true;
    if (p->direction != 1 && p->direction != -1) return true;
    return out_stride < track_obs_width(p->n_preview, other >= 0);
}

// One car's column of the SoA state [7][EA] (f110_get_state's rows).
struct TrackObsCar {
    double x, y, delta, v, yaw, yaw_rate, slip;
};

F110_HD TrackObsCar track_obs_car(const double *state, int64_t EA, int64_t col) {
    return TrackObsCar{state[col],          state[EA + col],     state[2 * EA + col], state[3 * EA + col],
                       state[4 * EA + col], state[5 * EA + col], state[6 * EA + col]};
}

// Steps 5-7: the seat's scaled state, its lateral offset t on the line and the sine and cosine of
// its heading error against the tangent (tan_x, tan_y) of its segment; (sn, cs) = cr_sincos(yaw).
F110_HD void track_obs_own(const f110_track_obs_params &P, const TrackObsCar &c, double t, double tan_x, double tan_y,
                           double sn, double cs, double out[kTrackObsOwn]) {
    const double dir = (double)P.direction;
    const double tx = dir * tan_x, ty = dir * tan_y;
    out[0] = c.v / P.v_scale;
    out[1] = c.delta / P.steer_scale;
    out[2] = c.yaw_rate / P.yaw_rate_scale;
    out[3] = c.slip / P.slip_scale;
    out[4] = dir * t / P.lat_scale;
    out[5] = sn * tx - cs * ty;
    out[6] = cs * tx + sn * ty;
}

// Step 8's arclength: d ahead of the projection, wrapped once on a closed track, clamped to the
// ends of an open one (pursuit_query with d for the lookahead).
F110_HD double track_obs_query(const f110_track_obs_params &P, double d, double s_proj, int closed, double L) {
    double sq = s_proj + (double)P.direction * d;
    if (closed) {
        if (sq > L) sq -= L;
        if (sq < 0.0) sq += L;
    } else {
        sq = sq < 0.0 ? 0.0 : (sq > L ? L : sq);
    }
    return sq;
}

// Step 8's two columns: the point at arclength sq on segment k (= seg_at(sq)) of the centerline
// xy / s (pursuit_action's target), in the frame of the car at (x, y) with heading (sn, cs), over d.
F110_HD void track_obs_preview(const double *xy, const double *s, int32_t k, double sq, double d, double x, double y,
                               double sn, double cs, double &px, double &py) {
    const double len = s[k + 1] - s[k];
    const double u = len == 0.0 ? 0.0 : (sq - s[k]) / len;
    const double ax = xy[2 * k], ay = xy[2 * k + 1];
    const double tx = ax + u * (xy[2 * k + 2] - ax), ty = ay + u * (xy[2 * k + 3] - ay);
    const double dx = tx - x, dy = ty - y;
    px = (cs * dx + sn * dy) / d;
    py = (-sn * dx + cs * dy) / d;
}

// Step 9: the other car (projection s_o, t_o, speed v_o) against the seat (s_p, t, v).
F110_HD void track_obs_gap(const f110_track_obs_params &P, int closed, double L, double s_p, double t, double v,
                           double s_o, double t_o, double v_o, double out[kTrackObsGap]) {
    const double dir = (double)P.direction;
    const double g = race_wrap(dir * (s_o - s_p), closed, L);
    out[0] = clip(g / P.gap_scale, -1.0, 1.0);
    out[1] = dir * (t_o - t) / P.lat_scale;
    out[2] = (v_o - v) / P.v_scale;
}

}  // namespace f110
