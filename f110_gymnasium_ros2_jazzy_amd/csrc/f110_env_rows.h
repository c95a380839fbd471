// f110_env_rows.h — the per-env row rules that kernels and the pure host hooks share: the
// per-env vehicle params' draw, the truncation flag, the episode statistics and the obs scan entry.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/f110.h"
#include "f110_math.h"
#include "f110_rng.h"

namespace f110 {

// ------------------------------------------------- per-env vehicle params --
// The 16 dynamics fields of f110_params (mu .. v_max, the struct's leading doubles) are the ones a
// context may hold per car (f110_set_env_params); width, length and lidar_max stay per agent.
constexpr int kDynFields = 16;
static_assert(offsetof(f110_params, width) == kDynFields * sizeof(double), "the dynamics fields lead f110_params");

// Domain randomization (f110_set_param_randomization): field k of a resetting car is
// lo[k] + u * (hi[k] - lo[k]) with u = r * 2^-32 for a Philox4x32 word r (no FMA: the library is
// built with contraction off).  Keyed by (seed, global env id) like spawn_draw; counter =
// (episode, tag 0xD0A17 -- not spawn_draw's 0x5BA3E --, agent * 4 + k / 4), word k % 4 of the block:
// four Philox blocks per car.  episode counts from the env's last explicit reset (0 for f110_reset,
// the finished episode's number + 1 for an autoreset), as the spawn draws do.  hi == lo gives lo.
// range: the agent's (lo[16], hi[16]).
F110_HD void param_draw(uint64_t seed, uint64_t env, int agent, uint64_t episode, const double *range,
                        double out[kDynFields]) {
    const uint32_t k0 = (uint32_t)seed ^ (uint32_t)env;
    const uint32_t k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(env >> 32) ^ 0xA5A5A5A5u;
#pragma unroll
    for (int j = 0; j < kDynFields / 4; ++j) {
        const U4 c = {(uint32_t)episode, (uint32_t)(episode >> 32), 0xD0A17u, (uint32_t)(agent * 4 + j)};
        const U4 r = philox(c, k0, k1);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 4 * j + q;
            const double lo = range[k], hi = range[kDynFields + k];
            const double u = (double)w[q] * (1.0 / 4294967296.0);
            out[k] = lo + u * (hi - lo);
        }
    }
}

// ------------------------------------------------------- episode limits --
// f110_set_episode_limits' flag for an env that did not terminate in the step: n = its steps since
// the reset, s = its stall counter after this step's update (include/f110.h).
F110_HD uint8_t truncation_code(uint64_t n, int32_t s, int64_t max_steps, int32_t stall_steps) {
    if (max_steps && n >= (uint64_t)max_steps) return 1;
    if (stall_steps && s >= stall_steps) return 2;
    return 0;
}

// --------------------------------------------------- episode statistics --
// One env's row of f110_episode_stats (the semantics of include/f110.h; k_episode and
// f110_host_episode_stats both call it).  Returns 0: the env does not finish, 1: it finishes
// terminated, 2: truncated; in the last two st.ret / st.len are the episode's return and length.
F110_HD int episode_update(double reward, int term, int trunc, int was_reset, f110_episode_state &st) {
    if (was_reset) {
        st.ret = 0.0;
        st.len = 0;
        st.closed = 0;
        return 0;
    }
    if (st.closed) return 0;
    st.ret += reward;
    st.len += 1;
    if (!(term || trunc)) return 0;
    st.closed = 1;
    return term ? 1 : 2;
}

// The envs finishing in one call (or one block's, or one env's share of them): what the totals add.
// n == 0: empty (mn / mx unused).
struct EpisodePart {
    int64_t n, n_term, n_trunc, len;
    double sum, mn, mx;
};

F110_HD EpisodePart episode_part(int code, const f110_episode_state &st) {
    EpisodePart p = {0, 0, 0, 0, 0.0, 0.0, 0.0};
    if (code) {
        p.n = 1;
        p.n_term = code == 1;
        p.n_trunc = code == 2;
        p.len = st.len;
        p.sum = p.mn = p.mx = st.ret;
    }
    return p;
}

// a += b, in this operand order (the fixed summation order is built from it)
F110_HD void episode_merge(EpisodePart &a, const EpisodePart &b) {
    if (b.n) {
        a.mn = a.n ? (b.mn < a.mn ? b.mn : a.mn) : b.mn;
        a.mx = a.n ? (b.mx > a.mx ? b.mx : a.mx) : b.mx;
    }
    a.n += b.n;
    a.n_term += b.n_term;
    a.n_trunc += b.n_trunc;
    a.len += b.len;
    a.sum += b.sum;
}

F110_HD void episode_totals_add(f110_episode_totals &t, const EpisodePart &b) {
    EpisodePart a = {t.episodes, t.terminated, t.truncated, t.length_sum, t.return_sum, t.return_min, t.return_max};
    episode_merge(a, b);
    t.episodes = a.n;
    t.terminated = a.n_term;
    t.truncated = a.n_trunc;
    t.length_sum = a.len;
    t.return_sum = a.sum;
    t.return_min = a.mn;
    t.return_max = a.mx;
}

// ------------------------------------------------------------- obs scan entry --
// F110Env._pack_flat_obs's scan entry (f110_env.py:557-560) from the float32 range: NaN -> lidar_max,
// +-inf -> lidar_max / 0, clip to [0, lidar_max], one IEEE f32 divide by lidar_max.  The step's
// packers (obs_scan_value(double, .), f110_step_device.h), f110_agent_obs and f110_host_agent_obs
// all call it.
F110_HD float obs_scan_value(float v, float lmax) {
    if (v != v) v = lmax;
    else if (__builtin_isinf(v)) v = v > 0 ? lmax : 0.0f;
    v = v < 0.0f ? 0.0f : (v > lmax ? lmax : v);
    return v / lmax;
}

}  // namespace f110
