// f110_task_capi.cpp — the context-free training entry points of include/f110.h: the track of the
// progress reward (f110_track_*), f110_reward, f110_gap_follow, f110_pure_pursuit with its host
// statement, the race statistics with theirs, the track observation with its own (and its entry on
// a context's live state, which needs both the track's and the context's internals), the scan
// observation's handle, the sensor randomization's handle, the collision batches and the episode
// statistics.  Argument checks and launches; the kernels are in f110_reward.hip, f110_opponent.hip,
// f110_pursuit.hip, f110_race.hip, f110_track_obs.hip, f110_scan_obs.hip, f110_sensor.hip,
// f110_batch.hip and f110_episode.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../../include/f110.h"
#include "../../include/f110_debug.h"
#include "f110_ctx.h"
#include "f110_env_rows.h"
#include "f110_host.h"
#include "f110_host_util.h"
#include "f110_pursuit.h"
#include "f110_scan_obs.h"
#include "f110_sensor.h"
#include "f110_step_args.h"
#include "f110_task_args.h"
#include "f110_track_obs.h"

using namespace f110;

// ---- training reward (rewards.py / track_progress.py) -----------------------
struct f110_track {
    DeviceArena arena;  // empty for a host-only track
    TrackView v{};
    std::vector<double> xy, s, tan, nrm, mid;  // host copies (f110_track_arrays, f110_host_pure_pursuit)
};

extern "C" int f110_track_create(f110_track **out, int32_t device, const double *xy, const double *w_right,
                                 const double *w_left, int32_t n, int32_t closed) {
    if (!out || !xy || n < 2 || ((w_right == nullptr) != (w_left == nullptr)))
        return fail(F110_E_INVALID, "f110_track_create: bad arguments (need >= 2 centerline points)");
    const bool host_only = device < 0;  // derived arrays only (f110_track_arrays), no device copy
    if (!host_only && hipSetDevice(device) != hipSuccess)
        return fail(F110_E_NODEVICE, "f110_track_create: no such HIP device");
    auto *t = new f110_track();
    t->arena.device = device;
    t->xy.assign(xy, xy + 2 * (size_t)n);
    track_arrays(xy, n, t->s, t->tan, t->nrm, t->mid);
    if (!host_only) {
        const TrackGrid g = track_grid(xy, n, t->mid);
        DeviceArena &a = t->arena;
        TrackView &v = t->v;
        if (!g.cstart.empty()) {
            v.gh = g.gh;
            v.gx0 = g.gx0;
            v.gy0 = g.gy0;
            v.gnx = g.gnx;
            v.gny = g.gny;
        }
        hipError_t e = a.upload(&v.xy, xy, 2 * (size_t)n);
        if (e == hipSuccess && !g.cstart.empty()) e = a.upload(&v.cell_start, g.cstart.data(), g.cstart.size());
        if (e == hipSuccess && !g.citems.empty()) e = a.upload(&v.cell_items, g.citems.data(), g.citems.size());
        if (e == hipSuccess && !g.cmid.empty()) e = a.upload(&v.cell_mid, g.cmid.data(), g.cmid.size());
        if (e == hipSuccess) e = a.upload(&v.s, t->s.data(), t->s.size());
        if (e == hipSuccess) e = a.upload(&v.tan, t->tan.data(), t->tan.size());
        if (e == hipSuccess) e = a.upload(&v.nrm, t->nrm.data(), t->nrm.size());
        if (e == hipSuccess) e = a.upload(&v.mid, t->mid.data(), t->mid.size());
        if (e == hipSuccess && w_right) e = a.upload(&v.wR, w_right, (size_t)n);
        if (e == hipSuccess && w_left) e = a.upload(&v.wL, w_left, (size_t)n);
        if (e != hipSuccess) {
            delete t;  // (the arena frees what was uploaded)
            return hip_fail("f110_track_create", e);
        }
    }
    t->v.n = n;
    t->v.closed = closed ? 1 : 0;
    t->v.L = t->s[(size_t)n - 1];
    *out = t;
    return F110_OK;
}

extern "C" int f110_track_destroy(f110_track *t) {
    delete t;
    return F110_OK;
}

extern "C" double f110_track_arrays(const f110_track *t, double *s, double *tan, double *nrm, double *mid) {
    if (!t) return 0.0;
    if (s) std::copy(t->s.begin(), t->s.end(), s);
    if (tan) std::copy(t->tan.begin(), t->tan.end(), tan);
    if (nrm) std::copy(t->nrm.begin(), t->nrm.end(), nrm);
    if (mid) std::copy(t->mid.begin(), t->mid.end(), mid);
    return t->v.L;
}

extern "C" int f110_reward(const f110_track *track, const f110_reward_params *params, const float *obs,
                           int64_t n_envs, int32_t obs_len, int32_t n_beams, f110_reward_state *state,
                           const uint8_t *reset_mask, double *rewards, void *stream) {
    if (!params || n_envs < 0 || (n_envs > 0 && (!obs || !state || !rewards)) || n_beams < 0 || n_beams > 2048 ||
        obs_len < n_beams + 8)
        return fail(F110_E_INVALID, "f110_reward: bad arguments (obs rows need n_beams + 8 entries, n_beams <= 2048)");
    if (params->use_progress && (!track || !track->v.mid))
        return fail(F110_E_INVALID, "f110_reward: use_progress needs a device track");
    RewardArgs a{};
    if (track) a.track = track->v;
    a.p = *params;
    a.obs = obs;
    a.E = n_envs;
    a.obs_len = obs_len;
    a.B = n_beams;
    a.state = state;
    a.reset_mask = reset_mask;
    a.rewards = rewards;
    HIP_TRY(launch_reward(a, (hipStream_t)stream));
    return F110_OK;
}

// ---- pure-pursuit opponent (f110_pursuit.hip; the row rule: f110_pursuit.h) ------------------
extern "C" void f110_default_pursuit_params(f110_pursuit_params *p) {
    if (!p) return;
    f110_params car;
    f110_default_params(&car);
    *p = f110_pursuit_params{};
    p->lookahead = 1.2;
    p->wheelbase = car.lf + car.lr;
    p->speed = 4.0;
    p->a_lat = 0.0;
    p->v_floor = 1.0;
    p->steer_limit = 0.4189;
    p->direction = 1;
}

extern "C" int f110_pure_pursuit(const f110_track *track, const f110_pursuit_params *params, const float *poses,
                                 int64_t n_rows, int64_t pose_stride, const double *row_speed,
                                 const uint8_t *row_mask, float *actions, int64_t action_stride, double *aux,
                                 void *stream) {
    if (!track || pursuit_bad_args(params, track->v.L, poses, n_rows, pose_stride, actions, action_stride))
        return fail(F110_E_INVALID, "f110_pure_pursuit: bad arguments (0 < lookahead < L, wheelbase and steer_limit "
                                    "> 0, speed and a_lat >= 0, direction +-1, pose_stride >= 3, action_stride >= 2)");
    if (!track->v.mid) return fail(F110_E_INVALID, "f110_pure_pursuit: needs a device track");
    PursuitArgs a{};
    a.track = track->v;
    a.p = *params;
    a.poses = poses;
    a.M = n_rows;
    a.pose_stride = pose_stride;
    a.action_stride = action_stride;
    a.row_speed = row_speed;
    a.row_mask = row_mask;
    a.actions = actions;
    a.aux = aux;
    HIP_TRY(launch_pursuit(a, (hipStream_t)stream));
    return F110_OK;
}

namespace {

struct HostProj {
    double s, t;
    int32_t seg;  // the segment (or, from the fallback, the node) s was taken from, as the device's Proj
};

// CenterlineProgress.project_xy (track_progress.py:58-97) over host arrays: the 5 midpoints of
// smallest squared distance by a full scan (ties: lower index), then project_xy's operations
// (f110_track_device.h) one for one.
HostProj host_project_xy(const TrackView &T, double x, double y) {
    constexpr int kTop5 = 5;
    double bd[kTop5];
    int32_t bi[kTop5];
    int have5 = 0;
    for (int32_t m = 0; m < T.n - 1; ++m) {
        const double dx = T.mid[2 * m] - x, dy = T.mid[2 * m + 1] - y;
        const double d2 = dx * dx + dy * dy;
        int k = have5;  // ascending index: an equal distance stays behind the earlier one
        while (k > 0 && d2 < bd[k - 1]) --k;
        if (k >= kTop5) continue;
        for (int j = std::min(have5, kTop5 - 1); j > k; --j) {
            bd[j] = bd[j - 1];
            bi[j] = bi[j - 1];
        }
        bd[k] = d2;
        bi[k] = m;
        if (have5 < kTop5) ++have5;
    }
    auto bdot = [](double a0, double a1, double b0, double b1) { return std::fma(a1, b1, a0 * b0); };
    bool have = false;
    double bn = 0.0, bs = 0.0, bt = 0.0;
    int32_t bseg = 0;
    for (int r = 0; r < have5; ++r) {
        const int32_t idx = bi[r];
        const double a0 = T.xy[2 * idx], a1 = T.xy[2 * idx + 1];
        const double ab0 = T.xy[2 * idx + 2] - a0, ab1 = T.xy[2 * idx + 3] - a1;
        const double L2 = bdot(ab0, ab1, ab0, ab1);
        if (L2 <= 1e-12) continue;
        const double ap0 = x - a0, ap1 = y - a1;
        double tp = bdot(ap0, ap1, ab0, ab1) / L2;
        tp = tp < 0.0 ? 0.0 : (tp > 1.0 ? 1.0 : tp);
        const double pr0 = a0 + tp * ab0, pr1 = a1 + tp * ab1;
        const double s_proj = T.s[idx] + tp * std::sqrt(L2);
        const double d0 = x - pr0, d1 = y - pr1;
        const double t_signed = bdot(d0, d1, T.nrm[2 * idx], T.nrm[2 * idx + 1]);
        const double nrm = std::sqrt(bdot(d0, d1, d0, d1));
        if (!have || nrm < bn) {
            have = true;
            bn = nrm;
            bs = s_proj;
            bt = t_signed;
            bseg = idx;
        }
    }
    if (!have) {  // degenerate fallback: nearest node (:93-95)
        double best = INFINITY;
        int32_t bj = 0;
        for (int32_t j = 0; j < T.n; ++j) {
            const double d0 = T.xy[2 * j] - x, d1 = T.xy[2 * j + 1] - y;
            const double d = std::sqrt(d0 * d0 + d1 * d1);
            if (d < best) {
                best = d;
                bj = j;
            }
        }
        return HostProj{T.s[bj], 0.0, bj};
    }
    return HostProj{bs, bt, bseg};
}

}  // namespace

extern "C" int f110_host_pure_pursuit(const f110_track *track, const f110_pursuit_params *params, const float *poses,
                                      int64_t n_rows, int64_t pose_stride, const double *row_speed,
                                      const uint8_t *row_mask, float *actions, int64_t action_stride, double *aux) {
    if (!track || pursuit_bad_args(params, track->v.L, poses, n_rows, pose_stride, actions, action_stride))
        return fail(F110_E_INVALID, "f110_host_pure_pursuit: bad arguments (0 < lookahead < L, wheelbase and "
                                    "steer_limit > 0, speed and a_lat >= 0, direction +-1, pose_stride >= 3, "
                                    "action_stride >= 2)");
    TrackView T = track->v;  // n, closed, L; the arrays on the host
    T.xy = track->xy.data();
    T.s = track->s.data();
    T.nrm = track->nrm.data();
    T.mid = track->mid.data();
    const f110_pursuit_params &P = *params;
    for (int64_t m = 0; m < n_rows; ++m) {
        if (row_mask && row_mask[m] == 0) continue;
        const float *p = poses + m * pose_stride;
        const double x = (double)p[0], y = (double)p[1], yaw = (double)p[2];
        float *act = actions + m * action_stride;
        double *ax = aux ? aux + 4 * m : nullptr;
        if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(yaw))) {
            act[0] = act[1] = 0.0f;
            if (ax) ax[0] = ax[1] = ax[2] = ax[3] = std::numeric_limits<double>::quiet_NaN();
            continue;
        }
        const HostProj pj = host_project_xy(T, x, y);
        const double sq = pursuit_query(P, pj.s, T.closed, T.L);
        // np.searchsorted(s, sq, side="right") - 1 clipped to [0, n-2]
        int64_t i = (std::upper_bound(T.s, T.s + T.n, sq) - T.s) - 1;
        i = std::max<int64_t>(0, std::min<int64_t>(i, T.n - 2));
        const PursuitAction r = pursuit_action(P, T.xy, T.s, (int32_t)i, sq, x, y, yaw, row_speed ? row_speed[m] : P.speed);
        act[0] = (float)r.steer;
        act[1] = (float)r.v;
        if (ax) {
            ax[0] = pj.s;
            ax[1] = pj.t + 0.0;  // (a zero as +0, as the kernel writes it)
            ax[2] = r.tx;
            ax[3] = r.ty;
        }
    }
    return F110_OK;
}

// ---- race statistics (f110_race.hip; the row rule: f110_race.h) ------------------------------
extern "C" void f110_default_race_params(f110_race_params *p) {
    if (!p) return;
    f110_params car;
    f110_default_params(&car);
    *p = f110_race_params{};
    p->pass_margin = car.length;
    p->direction = 1;
}

extern "C" int64_t f110_race_scratch_bytes(int64_t n_envs) {
    const int64_t n = n_envs > 0 ? n_envs : 1;
    return n * (int64_t)sizeof(RaceProj) + race_blocks(n) * (int64_t)sizeof(RacePart);
}

extern "C" int f110_race_stats(const f110_track *track, const f110_race_params *params, const float *ego,
                               const float *opp, int64_t stride, const uint8_t *terminated, const uint8_t *truncated,
                               const uint8_t *was_reset, int64_t n_envs, f110_race_state *state, double *cur,
                               double *last_progress, double *last_lead, int32_t *last_length, uint8_t *result,
                               f110_race_totals *totals, void *scratch, void *stream) {
    if (!track || !scratch || race_bad_args(params, ego, stride, terminated, was_reset, n_envs, state, result, totals))
        return fail(F110_E_INVALID, "f110_race_stats: bad arguments (a null pointer, stride < 4, n_envs < 0, "
                                    "pass_margin < 0 or NaN, direction other than +-1)");
    if (!track->v.mid) return fail(F110_E_INVALID, "f110_race_stats: needs a device track");
    RaceArgs a{};
    a.track = track->v;
    a.p = *params;
    a.ego = ego;
    a.opp = opp;
    a.stride = stride;
    a.E = n_envs;
    a.terminated = terminated;
    a.truncated = truncated;
    a.was_reset = was_reset;
    a.state = state;
    a.cur = cur;
    a.last_progress = last_progress;
    a.last_lead = last_lead;
    a.last_length = last_length;
    a.result = result;
    a.totals = totals;
    a.proj = static_cast<RaceProj *>(scratch);
    a.part = reinterpret_cast<RacePart *>(a.proj + (n_envs > 0 ? n_envs : 1));
    HIP_TRY(launch_race_stats(a, (hipStream_t)stream));
    return F110_OK;
}

extern "C" int f110_host_race_stats(const f110_track *track, const f110_race_params *params, const float *ego,
                                    const float *opp, int64_t stride, const uint8_t *terminated,
                                    const uint8_t *truncated, const uint8_t *was_reset, int64_t n_envs,
                                    f110_race_state *state, double *cur, double *last_progress, double *last_lead,
                                    int32_t *last_length, uint8_t *result, f110_race_totals *totals) {
    if (!track || race_bad_args(params, ego, stride, terminated, was_reset, n_envs, state, result, totals))
        return fail(F110_E_INVALID, "f110_host_race_stats: bad arguments (a null pointer, stride < 4, n_envs < 0, "
                                    "pass_margin < 0 or NaN, direction other than +-1)");
    TrackView T = track->v;  // n, closed, L; the arrays on the host
    T.xy = track->xy.data();
    T.s = track->s.data();
    T.nrm = track->nrm.data();
    T.mid = track->mid.data();
    const int has_opp = opp != nullptr;
    RacePart call = race_part_empty();
    for (int64_t e = 0; e < n_envs; ++e) {
        RaceRow r{};
        const float *cars[2] = {ego + e * stride, has_opp ? opp + e * stride : nullptr};
        for (int k = 0; k < 2; ++k) {
            if (!cars[k]) continue;
            const double x = (double)cars[k][0], y = (double)cars[k][1];
            r.col[k] = cars[k][3] != 0.0f;
            if (!(std::isfinite(x) && std::isfinite(y))) continue;
            const HostProj pj = host_project_xy(T, x, y);
            r.ok[k] = 1;
            r.s[k] = pj.s;
            if (k == 0) r.t0 = pj.t;
        }
        r.term = terminated[e];
        r.trunc = truncated ? truncated[e] : 0;
        r.was_reset = was_reset[e];
        r.has_opp = has_opp;
        f110_race_state &st = state[e];
        const int res = race_update(*params, T.closed, T.L, r, st);
        result[e] = (uint8_t)res;
        const double lead = race_lead(st, has_opp);
        if (cur) {
            cur[2 * e] = st.prog[0];
            cur[2 * e + 1] = lead;
        }
        if (res) {
            if (last_progress) last_progress[e] = st.prog[0];
            if (last_lead) last_lead[e] = lead;
            if (last_length) last_length[e] = st.len;
        }
        race_merge(call, race_part(res, st, has_opp));
    }
    race_totals_add(*totals, call);
    return F110_OK;
}

// ---- track observation (f110_track_obs.hip; the row rule: f110_track_obs.h) ------------------
extern "C" void f110_default_track_obs_params(f110_track_obs_params *p) {
    if (!p) return;
    *p = f110_track_obs_params{};
    p->v_scale = 20.0;
    p->steer_scale = 0.4189;
    p->yaw_rate_scale = kYawRateCap;
    p->slip_scale = kSlipCap;
    p->lat_scale = 1.0;
    p->gap_scale = 10.0;
    p->preview[0] = 1.0;
    p->preview[1] = 2.0;
    p->preview[2] = 4.0;
    p->preview[3] = 8.0;
    p->n_preview = 4;
    p->direction = 1;
}

extern "C" int32_t f110_track_obs_width(int32_t n_preview, int32_t has_other) {
    if (n_preview < 0 || n_preview > kTrackObsMaxPreview) return -1;
    return track_obs_width(n_preview, has_other != 0);
}

namespace {

const char kTrackObsBad[] = ": bad arguments (a null pointer, n_envs < 0, n_agents outside 1..8, seat / other outside "
                            "the agents or equal, out_stride < width, a scale <= 0, n_preview outside 0..8, a preview "
                            "distance outside (0, L), direction other than +-1)";

int track_obs_launch(const char *fn, const f110_track *track, const f110_track_obs_params *params, const double *state,
                     int64_t n_envs, int32_t n_agents, int32_t seat, int32_t other, float *out, int64_t out_stride,
                     void *stream) {
    if (!track || track_obs_bad_args(params, track->v.L, state, n_envs, n_agents, seat, other, out, out_stride))
        return fail(F110_E_INVALID, std::string(fn) + kTrackObsBad);
    if (!track->v.mid) return fail(F110_E_INVALID, std::string(fn) + ": needs a device track");
    TrackObsArgs a{};
    a.track = track->v;
    a.p = *params;
    a.state = state;
    a.E = n_envs;
    a.out_stride = out_stride;
    a.A = n_agents;
    a.seat = seat;
    a.other = other;
    a.width = track_obs_width(params->n_preview, other >= 0);
    a.out = out;
    HIP_TRY(launch_track_obs(a, (hipStream_t)stream));
    return F110_OK;
}

}  // namespace

extern "C" int f110_track_obs(const f110_track *track, const f110_track_obs_params *params, const double *state,
                              int64_t n_envs, int32_t n_agents, int32_t seat, int32_t other, float *out,
                              int64_t out_stride, void *stream) {
    return track_obs_launch("f110_track_obs", track, params, state, n_envs, n_agents, seat, other, out, out_stride,
                            stream);
}

// on the context's live state: its own buffer goes to the kernel, nothing is copied
extern "C" int f110_ctx_track_obs(f110_ctx *ctx, const f110_track *track, const f110_track_obs_params *params,
                                  int32_t seat, int32_t other, float *out, int64_t out_stride, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_ctx_track_obs: null context");
    if (track && track->v.mid && track->arena.device != ctx->arena.device)
        return fail(F110_E_INVALID, "f110_ctx_track_obs: the track is on another device than the context");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    return track_obs_launch("f110_ctx_track_obs", track, params, ctx->st, ctx->cfg.n_envs, ctx->cfg.n_agents, seat,
                            other, out, out_stride, stream);
}

extern "C" int f110_host_track_obs(const f110_track *track, const f110_track_obs_params *params, const double *state,
                                   int64_t n_envs, int32_t n_agents, int32_t seat, int32_t other, float *out,
                                   int64_t out_stride) {
    if (!track || track_obs_bad_args(params, track->v.L, state, n_envs, n_agents, seat, other, out, out_stride))
        return fail(F110_E_INVALID, std::string("f110_host_track_obs") + kTrackObsBad);
    TrackView T = track->v;  // n, closed, L; the arrays on the host
    T.xy = track->xy.data();
    T.s = track->s.data();
    T.tan = track->tan.data();
    T.nrm = track->nrm.data();
    T.mid = track->mid.data();
    const f110_track_obs_params &P = *params;
    const int np = P.n_preview;
    const int32_t width = track_obs_width(np, other >= 0);
    const int64_t EA = n_envs * n_agents;
    for (int64_t e = 0; e < n_envs; ++e) {
        float *row = out + e * out_stride;
        std::fill(row, row + width, 0.0f);  // a row that is not ok, three zeros for such an other car, the pad
        const TrackObsCar c = track_obs_car(state, EA, e * n_agents + seat);
        if (!(std::isfinite(c.x) && std::isfinite(c.y) && std::isfinite(c.yaw))) continue;
        const HostProj pj = host_project_xy(T, c.x, c.y);
        const int32_t i = pj.seg < T.n - 2 ? pj.seg : T.n - 2;
        double sn, cs;
        cr_sincos(c.yaw, sn, cs);
        double own[kTrackObsOwn];
        track_obs_own(P, c, pj.t, T.tan[2 * i], T.tan[2 * i + 1], sn, cs, own);
        for (int j = 0; j < kTrackObsOwn; ++j) row[j] = (float)own[j];
        for (int j = 0; j < np; ++j) {
            const double d = P.preview[j];
            const double sq = track_obs_query(P, d, pj.s, T.closed, T.L);
            // np.searchsorted(s, sq, side="right") - 1 clipped to [0, n-2]
            int64_t k = (std::upper_bound(T.s, T.s + T.n, sq) - T.s) - 1;
            k = std::max<int64_t>(0, std::min<int64_t>(k, T.n - 2));
            double px, py;
            track_obs_preview(T.xy, T.s, (int32_t)k, sq, d, c.x, c.y, sn, cs, px, py);
            row[kTrackObsOwn + 2 * j] = (float)px;
            row[kTrackObsOwn + 2 * j + 1] = (float)py;
        }
        if (other < 0) continue;
        const TrackObsCar o = track_obs_car(state, EA, e * n_agents + other);
        if (!(std::isfinite(o.x) && std::isfinite(o.y))) continue;
        const HostProj po = host_project_xy(T, o.x, o.y);
        double gap[kTrackObsGap];
        track_obs_gap(P, T.closed, T.L, pj.s, pj.t, c.v, po.s, po.t, o.v, gap);
        for (int j = 0; j < kTrackObsGap; ++j) row[kTrackObsOwn + 2 * np + j] = (float)gap[j];
    }
    return F110_OK;
}

// ---- scan observation (f110_scan_obs.hip; the row rule: f110_scan_obs.h) ----------------------
// (f110_default_scan_obs_params, f110_scan_obs_width and the host statement: f110_host.cpp)
struct f110_scan_obs {
    DeviceArena arena;
    ScanObsArgs a{};  // the shape, the ring and the heads; a push fills in its rows
    f110_scan_obs_params p{};
};

extern "C" int f110_scan_obs_create(f110_scan_obs **out, int32_t device, int64_t n_envs, int32_t n_beams,
                                    int32_t n_mid, int32_t n_tail, const f110_scan_obs_params *params) {
    const char *bad = !out ? "null out" : scan_obs_bad_shape(params, n_beams, n_mid, n_tail);
    if (!bad && (n_envs < 1 || n_envs >= (int64_t)1 << 31)) bad = "n_envs must be positive (and below 2^31)";
    if (bad) return fail(F110_E_INVALID, std::string("f110_scan_obs_create: ") + bad);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(F110_E_NODEVICE, "f110_scan_obs_create: no such HIP device");
    if (hipSetDevice(device) != hipSuccess) return fail(F110_E_NODEVICE, "f110_scan_obs_create: hipSetDevice");
    auto *so = new f110_scan_obs();
    so->arena.device = device;
    so->p = *params;
    ScanObsArgs &a = so->a;
    a.E = n_envs;
    a.B = n_beams;
    a.M = n_mid;
    a.T = n_tail;
    a.K = params->n_bins;
    a.F = params->n_frames;
    a.S = params->stride;
    a.D = scan_obs_depth(*params);
    a.reduce = params->reduce;
    a.keep_mid = params->keep_mid;
    const size_t N = (size_t)n_envs;
    hipError_t e = so->arena.alloc(&a.ring, N * a.D * a.K, /*zero=*/true);
    if (e == hipSuccess) e = so->arena.alloc(&a.head, N, /*zero=*/false);
    if (e == hipSuccess) e = hipMemset(a.head, 0xff, N * sizeof(int32_t));  // every head -1: empty
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        delete so;  // (the arena frees what was allocated)
        return hip_fail("f110_scan_obs_create", e, F110_E_ALLOC);
    }
    *out = so;
    return F110_OK;
}

extern "C" int f110_scan_obs_destroy(f110_scan_obs *so) {
    delete so;
    return F110_OK;
}

extern "C" int f110_scan_obs_push(f110_scan_obs *so, const float *rows, int64_t row_stride, const uint8_t *reset,
                                  float *out, int64_t out_stride, void *stream) {
    if (!so) return fail(F110_E_INVALID, "f110_scan_obs_push: null handle");
    ScanObsArgs a = so->a;
    const char *bad = scan_obs_bad_push(a.E, a.B + a.M + a.T, scan_obs_width(so->p, a.M, a.T), rows, row_stride, out,
                                        out_stride);
    if (bad) return fail(F110_E_INVALID, std::string("f110_scan_obs_push: ") + bad);
    if (hipSetDevice(so->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_scan_obs_push: hipSetDevice");
    a.rows = rows;
    a.row_stride = row_stride;
    a.reset = reset;
    a.out = out;
    a.out_stride = out_stride;
    a.vec4 = (row_stride % 4 == 0 && ((uintptr_t)rows & 15u) == 0) ? 1 : 0;
    hipError_t e = launch_scan_obs(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_scan_obs_push", e);
    return F110_OK;
}

extern "C" int f110_scan_obs_reset(f110_scan_obs *so, const uint8_t *env_mask, void *stream) {
    if (!so) return fail(F110_E_INVALID, "f110_scan_obs_reset: null handle");
    if (hipSetDevice(so->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_scan_obs_reset: hipSetDevice");
    hipError_t e = launch_scan_obs_reset(so->a.head, env_mask, so->a.E, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_scan_obs_reset", e);
    return F110_OK;
}

extern "C" int f110_scan_obs_arrays(f110_scan_obs *so, float **ring, int32_t **head) {
    if (!so) return fail(F110_E_INVALID, "f110_scan_obs_arrays: null handle");
    if (ring) *ring = so->a.ring;
    if (head) *head = so->a.head;
    return F110_OK;
}

// ---- sensor randomization (f110_sensor.hip; the row rule: f110_sensor.h) ----------------------
// (f110_default_sensor_params and the host statement: f110_host.cpp)
struct f110_sensor {
    DeviceArena arena;
    SensorArgs a{};  // the shape, the seed, the ranges, the mask, the parameter rows and the counters
};

extern "C" int f110_sensor_create(f110_sensor **out, int32_t device, int64_t n_envs, int32_t n_beams, int32_t n_mid,
                                  int32_t n_tail, float range_max, uint64_t seed, int64_t env_offset,
                                  const uint8_t *env_mask, const f110_sensor_params *params) {
    const char *bad = !out ? "null out"
                           : sensor_bad_shape(params, n_envs, n_beams, n_mid, n_tail, range_max, env_offset);
    if (bad) return fail(F110_E_INVALID, std::string("f110_sensor_create: ") + bad);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(F110_E_NODEVICE, "f110_sensor_create: no such HIP device");
    if (hipSetDevice(device) != hipSuccess) return fail(F110_E_NODEVICE, "f110_sensor_create: hipSetDevice");
    auto *sn = new f110_sensor();
    sn->arena.device = device;
    SensorArgs &a = sn->a;
    a.E = n_envs;
    a.B = n_beams;
    a.M = n_mid;
    a.T = n_tail;
    a.range_max = range_max;
    a.seed = seed;
    a.env_offset = env_offset;
    a.p = *params;
    const size_t N = (size_t)n_envs;
    hipError_t e = sn->arena.alloc(&a.param_rows, N * kSensorRowFloats, /*zero=*/true);
    if (e == hipSuccess) e = sn->arena.alloc(&a.step, N, /*zero=*/true);
    if (e == hipSuccess) e = sn->arena.alloc(&a.episode, N, /*zero=*/false);
    if (e == hipSuccess) e = hipMemset(a.episode, 0xff, N * sizeof(int32_t));  // every episode -1: no apply yet
    if (e == hipSuccess && env_mask) e = sn->arena.upload(&a.mask, env_mask, N);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        delete sn;  // (the arena frees what was allocated)
        return hip_fail("f110_sensor_create", e, F110_E_ALLOC);
    }
    *out = sn;
    return F110_OK;
}

extern "C" int f110_sensor_destroy(f110_sensor *sn) {
    delete sn;
    return F110_OK;
}

extern "C" int f110_sensor_apply(f110_sensor *sn, const float *rows, int64_t row_stride, const uint8_t *reset,
                                 float *out, int64_t out_stride, void *stream) {
    if (!sn) return fail(F110_E_INVALID, "f110_sensor_apply: null handle");
    SensorArgs a = sn->a;
    const char *bad = sensor_bad_apply(a.E, a.B + a.M + a.T, rows, row_stride, out, out_stride);
    if (bad) return fail(F110_E_INVALID, std::string("f110_sensor_apply: ") + bad);
    if (hipSetDevice(sn->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_sensor_apply: hipSetDevice");
    a.rows = rows;
    a.row_stride = row_stride;
    a.reset = reset;
    a.out = out;
    a.out_stride = out_stride;
    hipError_t e = launch_sensor(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_sensor_apply", e);
    return F110_OK;
}

extern "C" int f110_sensor_reset(f110_sensor *sn, const uint8_t *env_mask, void *stream) {
    if (!sn) return fail(F110_E_INVALID, "f110_sensor_reset: null handle");
    if (hipSetDevice(sn->arena.device) != hipSuccess) return fail(F110_E_HIP, "f110_sensor_reset: hipSetDevice");
    hipError_t e = launch_sensor_reset(sn->a.episode, sn->a.step, env_mask, sn->a.E, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("f110_sensor_reset", e);
    return F110_OK;
}

extern "C" int f110_sensor_arrays(f110_sensor *sn, float **param_rows, int32_t **episode, int32_t **step) {
    if (!sn) return fail(F110_E_INVALID, "f110_sensor_arrays: null handle");
    if (param_rows) *param_rows = sn->a.param_rows;
    if (episode) *episode = sn->a.episode;
    if (step) *step = sn->a.step;
    return F110_OK;
}

// ---- gap-follow opponent, collision batches -----------------------------------
extern "C" int f110_gap_follow(const float *scans, int64_t n_scans, int64_t scan_stride, int32_t n_beams,
                               double angle_min, double angle_increment, float *actions, int64_t action_stride,
                               int32_t *gaps, void *stream) {
    if (n_scans < 0 || n_beams <= 0 || (n_scans > 0 && (!scans || !actions)) || scan_stride < n_beams ||
        action_stride < 2)
        return fail(F110_E_INVALID, "f110_gap_follow: bad arguments");
    if (gap_follow_lds_bytes(n_beams) > 160 * 1024) return fail(F110_E_INVALID, "f110_gap_follow: n_beams too large");
    GapFollowArgs a;
    a.scans = scans;
    a.M = n_scans;
    a.scan_stride = scan_stride;
    a.action_stride = action_stride;
    a.actions = actions;
    a.gaps = gaps;
    a.angle_min = angle_min;
    a.angle_increment = angle_increment;
    a.B = n_beams;
    HIP_TRY(launch_gap_follow(a, (hipStream_t)stream));
    return F110_OK;
}

extern "C" int f110_collision_batch(const double *v1, const double *v2, int64_t M, uint8_t *out, void *stream) {
    if (M < 0 || (M > 0 && (!v1 || !v2 || !out))) return fail(F110_E_INVALID, "f110_collision_batch: bad arguments");
    HIP_TRY(launch_collision_batch(v1, v2, M, out, (hipStream_t)stream));
    return F110_OK;
}

extern "C" int f110_collision_multiple(const double *verts, int64_t M, int32_t N, double *collisions, double *idx,
                                       void *stream) {
    if (M < 0 || N < 1 || N > kMaxMultiBodies || (M > 0 && (!verts || !collisions || !idx)))
        return fail(F110_E_INVALID, "f110_collision_multiple: bad arguments (1 <= N <= 64)");
    HIP_TRY(launch_collision_multiple(verts, M, N, collisions, idx, (hipStream_t)stream));
    return F110_OK;
}

// ----------------------------------------------------- episode statistics --
extern "C" int64_t f110_episode_scratch_bytes(int64_t n_envs) {
    return (n_envs > 0 ? episode_blocks(n_envs) : 1) * (int64_t)sizeof(EpisodePart);
}

extern "C" int f110_episode_stats(const double *rewards, const uint8_t *terminated, const uint8_t *truncated,
                                  const uint8_t *was_reset, int64_t n_envs, f110_episode_state *state,
                                  double *last_return, int32_t *last_length, uint8_t *finished,
                                  f110_episode_totals *totals, void *scratch, void *stream) {
    const int rc = check_episode_args("f110_episode_stats", rewards, terminated, was_reset, n_envs, state, totals);
    if (rc != F110_OK) return rc;
    if (!scratch) return fail(F110_E_INVALID, "f110_episode_stats: null scratch");
    EpisodeArgs a{};
    a.rewards = rewards;
    a.terminated = terminated;
    a.truncated = truncated;
    a.was_reset = was_reset;
    a.E = n_envs;
    a.state = state;
    a.last_return = last_return;
    a.last_length = last_length;
    a.finished = finished;
    a.totals = totals;
    a.part = static_cast<EpisodePart *>(scratch);
    HIP_TRY(launch_episode_stats(a, (hipStream_t)stream));
    return F110_OK;
}
