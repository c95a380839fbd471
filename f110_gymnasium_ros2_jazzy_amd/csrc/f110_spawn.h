// f110_spawn.h — the spawn randomization's row rule (f110_set_spawn_randomization, include/f110.h):
// what a resetting car draws, the table row its base pose comes from and the perturbed, cleared
// pose.  k_agents<., ., SPAWN> and the host statement (f110_host_spawn_rows) both call it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/f110.h"
#include "f110_map.h"
#include "f110_math.h"
#include "f110_rng.h"
#include "f110_sincos.h"

namespace f110 {

static_assert(sizeof(f110_spawn_range) == 72, "f110_spawn_range: 6 doubles, 2 int32, 2 doubles");

// One car's draws: the lateral offset d, the heading offset dth, the start speed v0, the gap
// magnitude in table rows and whether it counts backwards.
struct SpawnDraws {
    double d, dth, v0;
    uint32_t mag;
    bool behind;
};

// Philox4x32-10 under param_draw's key (seed, global env id); counter = (episode, tag 0x5FA17 -- not
// spawn_draw's 0x5BA3E nor param_draw's 0xD0A17 --, agent * 2 + j).  Block j = 0: gap magnitude,
// behind, lateral, heading; block j = 1, word 0: speed.  Reals are lo + u * (hi - lo), u = r * 2^-32
// (no FMA: contraction is off); hi == lo gives lo.  episode as param_draw's: 0 for f110_reset, the
// finished episode's number + 1 for an autoreset.
F110_HD SpawnDraws spawn_draws(uint64_t seed, uint64_t env, int agent, uint64_t episode, const f110_spawn_range &r) {
    const uint32_t k0 = (uint32_t)seed ^ (uint32_t)env;
    const uint32_t k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(env >> 32) ^ 0xA5A5A5A5u;
    const U4 c0 = {(uint32_t)episode, (uint32_t)(episode >> 32), 0x5FA17u, (uint32_t)(agent * 2)};
    const U4 c1 = {(uint32_t)episode, (uint32_t)(episode >> 32), 0x5FA17u, (uint32_t)(agent * 2 + 1)};
    const U4 a = philox(c0, k0, k1), b = philox(c1, k0, k1);
    const double inv = 1.0 / 4294967296.0;
    SpawnDraws w;
    w.mag = (uint32_t)r.gap[0] + a.x % ((uint32_t)r.gap[1] - (uint32_t)r.gap[0] + 1u);
    w.behind = (double)a.y * inv < r.behind;
    w.d = r.lateral[0] + ((double)a.z * inv) * (r.lateral[1] - r.lateral[0]);
    w.dth = r.heading[0] + ((double)a.w * inv) * (r.heading[1] - r.heading[0]);
    w.v0 = r.speed[0] + ((double)b.x * inv) * (r.speed[1] - r.speed[0]);
    return w;
}

// gap == {0, 0}: the agent keeps its own column of the env's row
F110_HD bool spawn_own_column(const f110_spawn_range &r) { return r.gap[0] == 0 && r.gap[1] == 0; }

// (k +- mag) mod n for a row k < n of a table of n >= 1 rows
F110_HD uint32_t spawn_shift_row(uint32_t k, uint32_t mag, bool behind, uint32_t n) {
    const uint32_t m = mag % n;
    return behind ? (k + (n - m)) % n : (k + m) % n;
}

// The lateral offset accepted at base (px, py) with (sn, cs) of the base yaw: the first of d, d/2,
// d/4, d/8 whose position reads an EDT value >= clearance (an off-map position reads the map's last
// cell, cell_index), else 0.  The four lookups are independent loads.
F110_HD double spawn_clear_offset(const MapView &m, double px, double py, double sn, double cs, double d,
                                  double clearance) {
    const double t[4] = {d, d * 0.5, d * 0.25, d * 0.125};
    double v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = m.dt[cell_index(m, px + t[i] * (-sn), py + t[i] * cs)];
    double acc = 0.0;
#pragma unroll
    for (int i = 3; i >= 0; --i) acc = v[i] >= clearance ? t[i] : acc;
    return acc;
}

// The state a reset starts from: base pose (px, py, th) perturbed by the draws and cleared against
// the EDT; f32: the pose rounded as F110_F32 resets round it (the speed stays f64).
// out = (x, y, yaw, v0).
F110_HD void spawn_pose(const MapView &m, double px, double py, double th, const SpawnDraws &w, double clearance,
                        bool f32, double out[4], const double (*tab)[4] = kSinCosTab) {
    double sn, cs;
    cr_sincos(th, sn, cs, tab);
    const double d = spawn_clear_offset(m, px, py, sn, cs, w.d, clearance);
    double x = px + d * (-sn), y = py + d * cs, yaw = th + w.dth;
    if (f32) {
        x = (double)(float)x;
        y = (double)(float)y;
        yaw = (double)(float)yaw;
    }
    out[0] = x;
    out[1] = y;
    out[2] = yaw;
    out[3] = w.v0;
}

}  // namespace f110
