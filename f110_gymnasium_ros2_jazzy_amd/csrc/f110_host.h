// f110_host.h — the pure host functions of f110_host.cpp that the handle files call (private).
// None of them makes a HIP runtime call or touches a handle; tests/host_check links them alone.
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "../../include/f110.h"
#include "f110_env_rows.h"
#include "f110_host_util.h"
#include "f110_map.h"

namespace f110 {

// ---- map views and EDT tables ----------------------------------------------
// (inline: the per-step path of f110_ctx.cpp builds its views without a call into another file)
inline MapView make_map_view(const double *dt, int32_t H, int32_t W, double res, const double origin[3]) {
    MapView m;
    m.dt = dt;
    m.H = H;
    m.W = W;
    m.n = (int64_t)H * W;
    m.res = res;
    m.ox = origin[0];
    m.oy = origin[1];
    m.oc = std::cos(origin[2]);  // laser_models.py:421-422 (np.sin/np.cos of the yaml yaw)
    m.os = std::sin(origin[2]);
    m.wres = (double)W * res;
    m.hres = (double)H * res;
    m.inv_res = 1.0 / res;
    return m;
}

inline TiledMapView make_tiled_view(const MapView &m, const double *dt_tiled) {
    TiledMapView t;
    t.dt = dt_tiled;
    t.H = m.H;
    t.W = m.W;
    t.wt = (m.W + 3) / 4;
    t.oob = tiled_index(t.wt, m.H - 1, m.W - 1);
    t.res = m.res;
    t.inv_res = m.inv_res;
    t.ox = m.ox;
    t.oy = m.oy;
    t.oc = m.oc;
    t.os = m.os;
    t.wres = m.wres;
    t.hres = m.hres;
    return t;
}

bool fx_eligible(int32_t H, int32_t W, double res, const double origin[3], double eps, const uint32_t *edt_k, int32_t wpb);
std::vector<double> host_dt(const uint32_t *edt_k, size_t N, double res);
std::vector<double> host_padded_table(int32_t H, int32_t W, int32_t pad, const std::vector<double> &d, size_t &Wp,
                                      size_t &Hp);
std::vector<double> host_rowmajor_table(int32_t H, int32_t W, const std::vector<double> &d, size_t &Wp, size_t &Hp);

// ---- the size rules ---------------------------------------------
struct RayRules {
    int32_t lanes, refill, heavy_first, fxs_lds;
};
RayRules ray_rules(int64_t own, int64_t device_cars, int32_t contexts, int32_t kernel, bool pad_allowed);

// ---- per-env vehicle params ---------------------------------------------------
extern const char *const kParamNames[19];
static_assert(sizeof(f110_params) == 19 * sizeof(double), "f110_params is 19 doubles");

inline const double *fields(const f110_params &p) { return reinterpret_cast<const double *>(&p); }

// One row against its agent's params: every value finite, width / length / lidar_max the agent's.
// F110_OK, or F110_E_INVALID with the message "<who>: <field><where()> ..." (where: only built then).
template <class Where>
int check_param_row(const char *who, const f110_params &row, const f110_params &agent, Where where) {
    for (int k = 0; k < 19; ++k) {
        const double v = fields(row)[k];
        if (!std::isfinite(v))
            return fail(F110_E_INVALID, std::string(who) + ": " + kParamNames[k] + where() + " is not finite");
        if (k >= kDynFields && v != fields(agent)[k])
            return fail(F110_E_INVALID, std::string(who) + ": " + kParamNames[k] + where() +
                                            " differs from the agent's (the car boxes and the obs scale do not vary per env)");
    }
    return F110_OK;
}

int check_param_ranges(const char *who, const f110_params *lo, const f110_params *hi, const f110_params *agents,
                       int32_t n_agents);

// ---- spawn randomization --------------------------------------------------------
// f110_set_spawn_randomization's validation (n_spawn: the rows of the spawn table, 0 = none)
int check_spawn_ranges(const char *who, const f110_spawn_range *ranges, int32_t n_agents, int32_t n_spawn);

// ---- episode limits and statistics -------------------------------------------
int check_episode_limits(const char *who, int64_t max_steps, double stall_speed, int32_t stall_steps);
int check_episode_args(const char *who, const double *rewards, const uint8_t *terminated, const uint8_t *was_reset,
                       int64_t n_envs, const f110_episode_state *state, const f110_episode_totals *totals);

// ---- f110_track's derived arrays (track_progress.py) and midpoint grid -----------
void track_arrays(const double *xy, int32_t n, std::vector<double> &s, std::vector<double> &tan,
                  std::vector<double> &nrm, std::vector<double> &mid);
struct TrackGrid {  // TrackView's g* fields and cell arrays; cstart empty: no grid
    double gh = 0, gx0 = 0, gy0 = 0;
    int32_t gnx = 0, gny = 0;
    std::vector<int32_t> cstart, citems;
    std::vector<double> cmid;
};
TrackGrid track_grid(const double *xy, int32_t n, const std::vector<double> &mid);

// ---- n-step returns -------------------------------------------------------------
int check_nstep_args(const char *fn, int64_t n_envs, int32_t n_step, double gamma, int32_t obs_dim, int32_t act_dim);
int check_nstep_capacity(const char *fn, int64_t n_envs, int32_t n_step, int64_t capacity);
void nstep_powers(double gamma, int n, double *pw);  // pw[0..n], sequential products

// ---- action repeat ----------------------------------------------------------------
int check_repeat_args(const char *fn, int64_t n_envs, int32_t repeat, double gamma, int32_t obs_dim, int32_t act_dim);
int check_repeat_capacity(const char *fn, int64_t n_envs, int64_t capacity);

}  // namespace f110
